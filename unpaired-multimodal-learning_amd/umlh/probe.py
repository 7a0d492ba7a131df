"""Linear probes on the HIP kernels of umlh_kernels_probe.hip (C ABI: ``umlh_masked_mean``, ``umlh_probe_*``).

``masked_mean`` is the length-masked mean pooling of the reference's MultiBench ``evaluate`` (train.py:120-125) and, with
``lengths=None``, the plain ``mean(axis=1)`` of ``evaluate_raw_data``.  ``LogisticProbe`` is the binary
``LogisticRegression`` that ``evaluate`` fits (train.py:97-99): ``kind='lbfgs'`` for ``LogisticRegression(max_iter=200)``,
``kind='liblinear'`` for ``make_pipeline(StandardScaler(), LogisticRegression(max_iter=1000, solver='liblinear'))``.  It
returns the optimum of sklearn's objective, not sklearn's last iterate.  ``KNeighborsProbe`` is the ``KNeighborsClassifier()``
of the same factory (train.py:99-100) on the kernels of umlh_kernels_knn.hip (``umlh_knn_*``).  ``SoftmaxProbe`` is what the
same ``LogisticRegression(max_iter=200)`` becomes on more than two classes, a multinomial regression, fitted by the device-side
L-BFGS of umlh_kernels_softmax_probe.hip (``umlh_softmax_probe_*``); ``logistic_probe`` picks between the two.  Every call enqueues on
``torch.cuda.current_stream`` and returns without synchronising; only the ``n_iter_`` / ``converged_`` / ``score``
accessors read device memory back.  Inputs follow ``umlh.align``: fp32 CUDA tensors with unit column stride are used in
place (the row stride is passed on), other float dtypes are upcast, CPU tensors copied.  There is no CPU compute path.
"""
from __future__ import annotations

import torch

from . import _glue as glue
from ._lib import UmlhError, check, load_library

KINDS = {"lbfgs": 0, "liblinear": 1}
MAX_FEATURES = 1024


def _device() -> torch.device:
    return glue.device("umlh.align", "the metrics run only as HIP kernels")


MAX_NEIGHBORS = 24


def masked_mean(z: torch.Tensor, lengths: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """[B, T, Z] -> fp32 [B, Z] on the device: sum_{t < len_b} z[b, t] / len_b (len_b clipped to 0..T; 0 gives NaN as the
    reference's 0/0).  ``lengths=None``: the mean over T.  ``out``: an fp32 device view [B, Z] with unit column stride to
    write into (a column block of a wider matrix, for instance)."""
    if not isinstance(z, torch.Tensor) or z.ndim != 3:
        raise ValueError(f"masked_mean: expected a 3-D tensor [B, T, Z], got {getattr(z, 'shape', type(z))}")
    if not z.is_floating_point():
        raise ValueError(f"masked_mean: expected a floating-point tensor, got {z.dtype}")
    B, T, Z = z.shape
    if B < 1 or T < 1 or Z < 1:
        raise ValueError(f"masked_mean: empty input {tuple(z.shape)}")
    dev = _device()
    z = z.detach().to(device=dev, dtype=torch.float32)
    if z.stride(2) != 1 or z.stride(0) < Z or z.stride(1) < Z:
        z = z.contiguous()
    if lengths is not None:
        if lengths.numel() != B:
            raise ValueError(f"masked_mean: {lengths.numel()} lengths for {B} sequences")
        lengths = lengths.detach().reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    if out is None:
        out = torch.empty((B, Z), dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, Z) and out.stride(1) == 1 and out.stride(0) >= Z):
        raise ValueError("masked_mean: out must be an fp32 device view [B, Z] with unit column stride")
    check(load_library().umlh_masked_mean(z.data_ptr(), B, T, Z, z.stride(0), z.stride(1), glue.ptr(lengths), out.data_ptr(),
                                          out.stride(0), glue.stream(dev)), "umlh_masked_mean")
    return out


def column_stats(x: torch.Tensor) -> torch.Tensor:
    """StandardScaler().fit(x) as a float64 device tensor [2, d]: column means, then population standard deviations with
    values below 10 eps replaced by 1."""
    dev = _device()
    x = glue.features(x, "column_stats", dev)
    n, d = x.shape
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_probe_scratch_bytes", dev, n=n, d=d, max_iter=0)
    stats = torch.empty((2, d), dtype=torch.float64, device=dev)
    check(lib.umlh_probe_column_stats(x.data_ptr(), n, d, x.stride(0), stats.data_ptr(), scratch.data_ptr(), nbytes, glue.stream(dev)),
          "umlh_probe_column_stats")
    return stats


def _labels(y, n, dev, what):
    if not isinstance(y, torch.Tensor):
        y = torch.as_tensor(y)
    if y.numel() != n:
        raise ValueError(f"{what}: {y.numel()} labels for {n} rows")
    return y.detach().reshape(-1).to(device=dev, dtype=torch.int32).contiguous()


class LogisticProbe:
    """Binary L2-regularised logistic regression fitted by the device-side Newton iteration of ``umlh_probe_fit``.

    ``fit`` only enqueues; ``coef_`` ([1, d] float64) and ``intercept_`` ([1] float64) are device tensors (in the
    standardised space for ``kind='liblinear'``, as sklearn's pipeline keeps them).  ``record()`` reads the device record
    back: ``n_iter_``, ``converged_`` (0 = budget spent, 1 = max|gradient| <= gtol, 2 = the objective's precision floor),
    ``max_grad_``, ``objective_``."""

    def __init__(self, kind: str = "lbfgs", C: float = 1.0, max_iter: int = 30, gtol: float = 0.0, keep_objectives: bool = False):
        if kind not in KINDS:
            raise ValueError(f"LogisticProbe: kind={kind!r} not in {sorted(KINDS)}")
        if not C > 0:
            raise ValueError(f"LogisticProbe: C={C} must be positive")
        if not 1 <= int(max_iter) <= 1000:
            raise ValueError(f"LogisticProbe: max_iter={max_iter} outside 1..1000")
        if not gtol >= 0:
            raise ValueError(f"LogisticProbe: gtol={gtol} must be >= 0")
        self.kind, self.C, self.max_iter, self.gtol, self.keep_objectives = kind, float(C), int(max_iter), float(gtol), keep_objectives
        self._coef = self._record = self._stats = self._objectives = self._keep = self._host = None

    def fit(self, X: torch.Tensor, y, check_classes: bool = True) -> "LogisticProbe":
        """Enqueues the fit.  ``check_classes`` reads one flag back to raise ``ValueError`` when ``y`` holds a single class
        (as sklearn does) or a label other than 0/1; pass False when the labels are known to be sound and the caller wants
        no host synchronisation."""
        dev = _device()
        x = glue.features(X, "LogisticProbe.fit", dev)
        n, d = x.shape
        if n < 2:
            raise ValueError(f"LogisticProbe.fit: needs at least 2 rows, got {n}")
        if d > MAX_FEATURES:
            raise ValueError(f"LogisticProbe.fit: d={d} above {MAX_FEATURES}")
        yy = _labels(y, n, dev, "LogisticProbe.fit")
        if check_classes:
            lo, hi = (int(v) for v in torch.stack([yy.min(), yy.max()]).tolist())
            if lo < 0 or hi > 1:
                raise ValueError(f"LogisticProbe.fit: labels must be 0/1, got values in [{lo}, {hi}]")
            if lo == hi:
                raise ValueError(f"This solver needs samples of at least 2 classes in the data, but the data contains only one class: {lo}")
        lib = load_library()
        self._stats = column_stats(x) if self.kind == "liblinear" else None
        scratch, nbytes = glue.scratch("umlh_probe_scratch_bytes", dev, n=n, d=d, max_iter=self.max_iter)
        self._coef = torch.empty(d + 1, dtype=torch.float64, device=dev)
        self._record = torch.empty(24, dtype=torch.uint8, device=dev)
        self._objectives = torch.empty(self.max_iter + 1, dtype=torch.float64, device=dev) if self.keep_objectives else None
        check(lib.umlh_probe_fit(x.data_ptr(), n, d, x.stride(0), yy.data_ptr(), glue.ptr(self._stats), KINDS[self.kind], self.C,
                                 self.max_iter, self.gtol, self._coef.data_ptr(), self._record.data_ptr(),
                                 glue.ptr(self._objectives), scratch.data_ptr(), nbytes, glue.stream(dev)), "umlh_probe_fit")
        self._keep = (x, yy, scratch)          # this fit's own operands and scratch, alive as long as the probe
        self._host = None
        return self

    def _fitted(self):
        if self._coef is None:
            raise UmlhError("LogisticProbe: fit() has not been called")

    @property
    def coef_(self) -> torch.Tensor:
        self._fitted()
        return self._coef[:-1].reshape(1, -1)

    @property
    def intercept_(self) -> torch.Tensor:
        self._fitted()
        return self._coef[-1:]

    @property
    def stats_(self):
        """None, or the [2, d] float64 StandardScaler statistics of the 'liblinear' kind."""
        return self._stats

    def record(self) -> dict:
        self._fitted()
        if self._host is None:
            raw = self._record.cpu().numpy()
            self._host = {"n_iter": int(raw[0:4].view("<i4")[0]), "converged": int(raw[4:8].view("<i4")[0]),
                          "max_grad": float(raw[8:16].view("<f8")[0]), "objective": float(raw[16:24].view("<f8")[0])}
        return self._host

    n_iter_ = property(lambda self: self.record()["n_iter"])
    converged_ = property(lambda self: self.record()["converged"])
    max_grad_ = property(lambda self: self.record()["max_grad"])
    objective_ = property(lambda self: self.record()["objective"])

    @property
    def objectives_(self) -> torch.Tensor:
        """The objective after 0, 1, ... accepted steps (float64 device tensor); needs ``keep_objectives=True``."""
        self._fitted()
        if self._objectives is None:
            raise UmlhError("LogisticProbe: constructed without keep_objectives=True")
        return self._objectives[: self.n_iter_ + 1]

    def _score(self, X, y, want_decision, want_correct):
        self._fitted()
        dev = _device()
        x = glue.features(X, "LogisticProbe", dev)
        n, d = x.shape
        if d != self._coef.numel() - 1:
            raise ValueError(f"LogisticProbe: {d} features, fitted on {self._coef.numel() - 1}")
        yy = _labels(y, n, dev, "LogisticProbe.score") if want_correct else None
        dec = torch.empty(n, dtype=torch.float32, device=dev) if want_decision else None
        correct = torch.empty((), dtype=torch.int64, device=dev) if want_correct else None
        check(load_library().umlh_probe_score(x.data_ptr(), n, d, x.stride(0), glue.ptr(self._stats), self._coef.data_ptr(),
                                              glue.ptr(yy), glue.ptr(correct), glue.ptr(dec), glue.stream(dev)), "umlh_probe_score")
        return dec, correct, n

    def decision_function(self, X: torch.Tensor) -> torch.Tensor:
        """fp32 device tensor [N]: w . x + b (on the standardised features for 'liblinear')."""
        return self._score(X, None, True, False)[0]

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        """int64 device tensor [N]: 1 where the decision value is > 0 (sklearn's rule), else 0."""
        return (self.decision_function(X) > 0).to(torch.int64)

    def correct(self, X: torch.Tensor, y) -> torch.Tensor:
        """The number of correct predictions as a 0-d int64 device tensor (no host synchronisation)."""
        return self._score(X, y, False, True)[1]

    def score(self, X: torch.Tensor, y) -> float:
        """Mean accuracy = correct / N as a Python float."""
        _, correct, n = self._score(X, y, False, True)
        return int(correct.item()) / n


class KNeighborsProbe:
    """``KNeighborsClassifier(n_neighbors=k)`` with sklearn's defaults (Euclidean metric, uniform weights) on
    ``umlh_knn_search`` / ``umlh_knn_vote``.  Neighbours are ordered by (squared distance, train index): exact ties go to the
    smaller index.  A vote tie goes to the smallest label value.  Labels are integers >= 0 of any values (multi-class).
    ``splits`` (0 = auto) is the number of column chunks of the candidate pass; no result depends on it.

    ``fit`` keeps the fp32 device matrix (in place when it has unit column stride; the row stride travels) and int32 labels and
    makes no host synchronisation; nothing else does either, except ``score``."""

    def __init__(self, n_neighbors: int = 5, splits: int = 0):
        if not 1 <= int(n_neighbors) <= MAX_NEIGHBORS:
            raise ValueError(f"KNeighborsProbe: n_neighbors={n_neighbors} outside 1..{MAX_NEIGHBORS}")
        if int(splits) < 0:
            raise ValueError(f"KNeighborsProbe: splits={splits} must be >= 0")
        self.n_neighbors, self.splits = int(n_neighbors), int(splits)
        self._x = self._y = None

    def fit(self, X: torch.Tensor, y) -> "KNeighborsProbe":
        dev = _device()
        x = glue.features(X, "KNeighborsProbe.fit", dev)
        if x.shape[0] < self.n_neighbors:
            raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {self.n_neighbors}, n_samples_fit = {x.shape[0]}")
        self._x, self._y = x, _labels(y, x.shape[0], dev, "KNeighborsProbe.fit")
        return self

    def _search(self, X, want_dist):
        if self._x is None:
            raise UmlhError("KNeighborsProbe: fit() has not been called")
        dev = _device()
        x = glue.features(X, "KNeighborsProbe", dev)
        (nt, d), nq, k = self._x.shape, x.shape[0], self.n_neighbors
        if x.shape[1] != d:
            raise ValueError(f"KNeighborsProbe: {x.shape[1]} features, fitted on {d}")
        scratch, nbytes = glue.scratch("umlh_knn_scratch_bytes", dev, n_train=nt, n_query=nq, d=d, k=k, splits=self.splits)
        idx = torch.empty((nq, k), dtype=torch.int32, device=dev)
        dist = torch.empty((nq, k), dtype=torch.float32, device=dev) if want_dist else None
        check(load_library().umlh_knn_search(self._x.data_ptr(), nt, self._x.stride(0), x.data_ptr(), nq, x.stride(0), d, k, self.splits,
                                             idx.data_ptr(), glue.ptr(dist), scratch.data_ptr(), nbytes, glue.stream(dev)),
              "umlh_knn_search")
        return idx, dist, dev

    def _vote(self, X, y, want_pred, want_correct):
        idx, _, dev = self._search(X, False)
        nq = idx.shape[0]
        yy = _labels(y, nq, dev, "KNeighborsProbe.score") if want_correct else None
        pred = torch.empty(nq, dtype=torch.int32, device=dev) if want_pred else None
        correct = torch.empty((), dtype=torch.int64, device=dev) if want_correct else None
        check(load_library().umlh_knn_vote(idx.data_ptr(), nq, self.n_neighbors, self._y.data_ptr(), self._y.numel(), glue.ptr(yy),
                                           glue.ptr(pred), None, glue.ptr(correct), glue.stream(dev)), "umlh_knn_vote")
        return pred, correct, nq

    def kneighbors(self, X: torch.Tensor, return_distance: bool = True):
        """(dist fp32 [N, k], idx int64 [N, k]) device tensors, or idx alone with ``return_distance=False``."""
        idx, dist, _ = self._search(X, return_distance)
        return (dist, idx.to(torch.int64)) if return_distance else idx.to(torch.int64)

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        """int64 device tensor [N]: the most frequent label among the k neighbours, ties to the smallest label value."""
        return self._vote(X, None, True, False)[0].to(torch.int64)

    def correct(self, X: torch.Tensor, y) -> torch.Tensor:
        """The number of correct predictions as a 0-d int64 device tensor (no host synchronisation)."""
        return self._vote(X, y, False, True)[1]

    def score(self, X: torch.Tensor, y) -> float:
        """Mean accuracy = correct / N as a Python float."""
        _, correct, n = self._vote(X, y, False, True)
        return int(correct.item()) / n


class SoftmaxProbe:
    """Multinomial L2-regularised logistic regression (sklearn's ``LogisticRegression`` on more than two classes) fitted to its
    optimum by the device-side L-BFGS of ``umlh_softmax_probe_fit``: the objective is
    ``sum_i (logsumexp_c z_ic - z_iy) + |W[:, :d]|^2 / (2 C)``, intercepts not penalised.

    ``gtol=None`` means ``1e-4 * n`` (sklearn's ``tol=1e-4`` on its mean-loss gradient, restated for the sum).
    ``standardize=True`` fits on StandardScaler-ed features; ``coef_`` / ``intercept_`` then live in the standardised space (as
    sklearn's pipeline keeps them) while ``decision_function`` / ``predict`` / ``score`` take RAW features: the scaler is folded
    into the weights they use (``umlh_softmax_probe_fold``).  ``fit`` only enqueues, apart from the one read-back of
    ``unique(y)``; ``record()`` reads the device record back: ``n_iter_``, ``converged_`` (0 = budget spent or NaN, 1 =
    max|gradient| <= gtol, 2 = the precision floor), ``max_grad_``, ``objective_``."""

    MAX_FEATURES, MAX_CLASSES = 2048, 4096

    def __init__(self, C: float = 1.0, max_iter: int = 200, gtol: float | None = None, history: int = 10, standardize: bool = False,
                 keep_objectives: bool = False):
        if not C > 0:
            raise ValueError(f"SoftmaxProbe: C={C} must be positive")
        if not 1 <= int(max_iter) <= 1000:
            raise ValueError(f"SoftmaxProbe: max_iter={max_iter} outside 1..1000")
        if gtol is not None and not gtol >= 0:
            raise ValueError(f"SoftmaxProbe: gtol={gtol} must be >= 0")
        if not 1 <= int(history) <= 32:
            raise ValueError(f"SoftmaxProbe: history={history} outside 1..32")
        self.C, self.max_iter, self.gtol, self.history = float(C), int(max_iter), gtol, int(history)
        self.standardize, self.keep_objectives = bool(standardize), bool(keep_objectives)
        self._coef = self._record = self._stats = self._objectives = self._keep = self._host = self._w = self._b = self._classes = None

    def fit(self, X: torch.Tensor, y, coef_init=None, check_classes: bool = True, n_classes: int | None = None) -> "SoftmaxProbe":
        """Enqueues the fit.  ``classes_ = unique(y)`` and the labels are remapped to 0..K-1 (one read-back), unless
        ``check_classes=False`` and ``n_classes=K`` say that the labels are 0..K-1 with every class present (an absent class has
        no finite optimum).  ``coef_init``: a [K, d + 1] tensor ([weights | intercept]) or a fitted ``SoftmaxProbe`` of the same
        shape to start from."""
        dev = _device()
        x = glue.features(X, "SoftmaxProbe.fit", dev)
        n, d = x.shape
        if n < 2:
            raise ValueError(f"SoftmaxProbe.fit: needs at least 2 rows, got {n}")
        if d > self.MAX_FEATURES:
            raise ValueError(f"SoftmaxProbe.fit: d={d} above {self.MAX_FEATURES}")
        if not isinstance(y, torch.Tensor):
            y = torch.as_tensor(y)
        if y.numel() != n:
            raise ValueError(f"SoftmaxProbe.fit: {y.numel()} labels for {n} rows")
        if y.is_floating_point() or y.dtype == torch.bool:
            raise ValueError(f"SoftmaxProbe.fit: expected integer labels, got {y.dtype}")
        y = y.detach().reshape(-1).to(device=dev, dtype=torch.int64)
        if not check_classes and n_classes is not None:
            k = int(n_classes)
            classes = torch.arange(k, dtype=torch.int64, device=dev)
            yy = y.to(torch.int32).contiguous()
        else:
            classes = torch.unique(y)
            k = int(classes.numel())
            if n_classes is not None and int(n_classes) != k:
                raise ValueError(f"SoftmaxProbe.fit: n_classes={n_classes}, the labels hold {k} classes")
            yy = torch.searchsorted(classes, y).to(torch.int32).contiguous()
        if k < 2:
            raise ValueError(f"This solver needs samples of at least 2 classes in the data, but the data contains only one class: "
                             f"{int(classes[0]) if k else None}")
        if k > self.MAX_CLASSES or n * k >= 2 ** 31:
            raise ValueError(f"SoftmaxProbe.fit: {k} classes for {n} rows (need at most {self.MAX_CLASSES} classes and n * classes < 2^31)")
        if isinstance(coef_init, SoftmaxProbe):
            coef_init._fitted()
            coef_init = coef_init._coef
        if coef_init is not None:
            if not isinstance(coef_init, torch.Tensor) or tuple(coef_init.shape) != (k, d + 1):
                raise ValueError(f"SoftmaxProbe.fit: coef_init must be a [{k}, {d + 1}] tensor, got {getattr(coef_init, 'shape', type(coef_init))}")
            coef = coef_init.detach().to(device=dev, dtype=torch.float32).clone().contiguous()
        else:
            coef = torch.empty((k, d + 1), dtype=torch.float32, device=dev)
        lib = load_library()
        self._stats = column_stats(x) if self.standardize else None
        gtol = 1e-4 * n if self.gtol is None else float(self.gtol)
        scratch, nbytes = glue.scratch("umlh_softmax_probe_scratch_bytes", dev, n=n, d=d, n_class=k, max_iter=self.max_iter,
                                       history=self.history)
        self._record = torch.empty(24, dtype=torch.uint8, device=dev)
        self._objectives = torch.empty(self.max_iter + 1, dtype=torch.float64, device=dev) if self.keep_objectives else None
        check(lib.umlh_softmax_probe_fit(x.data_ptr(), n, d, x.stride(0), yy.data_ptr(), glue.ptr(self._stats), k, self.C, self.max_iter,
                                         self.history, gtol, 1 if coef_init is not None else 0, coef.data_ptr(), d + 1,
                                         self._record.data_ptr(), glue.ptr(self._objectives), scratch.data_ptr(), nbytes,
                                         glue.stream(dev)), "umlh_softmax_probe_fit")
        self._w = torch.empty((k, d), dtype=torch.float32, device=dev)
        self._b = torch.empty(k, dtype=torch.float32, device=dev)
        check(lib.umlh_softmax_probe_fold(coef.data_ptr(), d + 1, k, d, glue.ptr(self._stats), self._w.data_ptr(), d, self._b.data_ptr(),
                                          glue.stream(dev)), "umlh_softmax_probe_fold")
        self._coef, self._classes = coef, classes
        self._keep = (x, yy, scratch)          # this fit's own operands and scratch, alive as long as the probe
        self._host = None
        return self

    def _fitted(self):
        if self._coef is None:
            raise UmlhError("SoftmaxProbe: fit() has not been called")

    @property
    def coef_(self) -> torch.Tensor:
        self._fitted()
        return self._coef[:, :-1]

    @property
    def intercept_(self) -> torch.Tensor:
        self._fitted()
        return self._coef[:, -1]

    @property
    def classes_(self) -> torch.Tensor:
        self._fitted()
        return self._classes

    @property
    def stats_(self):
        """None, or the [2, d] float64 StandardScaler statistics of ``standardize=True``."""
        return self._stats

    @property
    def raw_weight_(self) -> torch.Tensor:
        """fp32 [K, d]: the weights on RAW features (``coef_`` with the scaler folded in; ``coef_`` itself without one)."""
        self._fitted()
        return self._w

    @property
    def raw_bias_(self) -> torch.Tensor:
        self._fitted()
        return self._b

    record = LogisticProbe.record
    n_iter_ = property(lambda self: self.record()["n_iter"])
    converged_ = property(lambda self: self.record()["converged"])
    max_grad_ = property(lambda self: self.record()["max_grad"])
    objective_ = property(lambda self: self.record()["objective"])

    @property
    def objectives_(self) -> torch.Tensor:
        """The objective at the start and the value the line search accepted for each step (float64 device tensor); needs
        ``keep_objectives=True``."""
        self._fitted()
        if self._objectives is None:
            raise UmlhError("SoftmaxProbe: constructed without keep_objectives=True")
        return self._objectives[: self.n_iter_ + 1]

    def _features(self, X, what):
        self._fitted()
        dev = _device()
        x = glue.features(X, what, dev)
        if x.shape[1] != self._w.shape[1]:
            raise ValueError(f"{what}: {x.shape[1]} features, fitted on {self._w.shape[1]}")
        return x, dev

    def decision_function(self, X: torch.Tensor) -> torch.Tensor:
        """fp32 device tensor [N, K]: the logits of raw features (``umlh_gemm_f32`` + ``umlh_bias_act``)."""
        x, dev = self._features(X, "SoftmaxProbe.decision_function")
        (n, d), k = x.shape, self._w.shape[0]
        out = torch.empty((n, k), dtype=torch.float32, device=dev)
        lib = load_library()
        check(lib.umlh_gemm_f32(x.data_ptr(), self._w.data_ptr(), out.data_ptr(), n, k, d, x.stride(0), d, k, 0, 0, None, None, 1.0, 1, None,
                                glue.stream(dev)), "umlh_gemm_f32")
        check(lib.umlh_bias_act(out.data_ptr(), self._b.data_ptr(), n, k, 0, glue.stream(dev)), "umlh_bias_act")
        return out

    def predict_topk(self, X: torch.Tensor, k: int = 5) -> torch.Tensor:
        """int64 device tensor [N, k]: the k most likely ``classes_`` values per row, best first (``umlh.report.topk_classes``:
        exact ties go to the smaller class).  A row containing NaN has no ranking: its slots hold -1."""
        from .report import topk_classes
        x, _ = self._features(X, "SoftmaxProbe.predict_topk")
        cls = topk_classes(x, self._w, self._b, k=k)[0].to(torch.int64)
        return torch.where(cls >= 0, self._classes[cls.clamp_min(0)], cls)

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        """int64 device tensor [N]: the most likely class value, ties to the smaller class as ``np.argmax``."""
        return self.predict_topk(X, 1)[:, 0]

    def correct(self, X: torch.Tensor, y) -> torch.Tensor:
        """The number of correct predictions as a 0-d int64 device tensor (``topk_classes`` + ``class_report``; no host
        synchronisation).  A label that is not one of ``classes_`` counts as wrong."""
        from .report import class_report, topk_classes
        x, dev = self._features(X, "SoftmaxProbe.correct")
        if not isinstance(y, torch.Tensor):
            y = torch.as_tensor(y)
        if y.numel() != x.shape[0]:
            raise ValueError(f"SoftmaxProbe.correct: {y.numel()} labels for {x.shape[0]} rows")
        y = y.detach().reshape(-1).to(device=dev, dtype=torch.int64)
        k = self._classes.numel()
        idx = torch.searchsorted(self._classes, y).clamp_max(k - 1)
        idx = torch.where(self._classes[idx] == y, idx, torch.full_like(idx, -1))
        cls = topk_classes(x, self._w, self._b, k=1)[0]
        return class_report(cls, idx, k)["hit1"].sum()

    def score(self, X: torch.Tensor, y) -> float:
        """Mean accuracy = correct / N as a Python float."""
        n = X.shape[0]
        return int(self.correct(X, y).item()) / n


def logistic_probe(kind: str = "lbfgs", n_classes: int = 2):
    """The probe of the reference's ``make_classifier('logistic', ...)`` for ``n_classes`` classes: ``LogisticProbe(kind)`` for
    two, ``SoftmaxProbe()`` for more with ``kind='lbfgs'``.  sklearn's one-vs-rest ``liblinear`` on more than two classes is not
    built."""
    if kind not in KINDS:
        raise ValueError(f"logistic_probe: kind={kind!r} not in {sorted(KINDS)}")
    if int(n_classes) < 2:
        raise ValueError(f"logistic_probe: n_classes={n_classes} < 2")
    if int(n_classes) == 2:
        return LogisticProbe(kind)
    if kind == "liblinear":
        raise ValueError("logistic_probe: kind='liblinear' with more than 2 classes (sklearn's one-vs-rest) is not built")
    return SoftmaxProbe()
