"""Linear probes on the HIP kernels of umlh_kernels_probe.hip (C ABI: ``umlh_masked_mean``, ``umlh_probe_*``).

``masked_mean`` is the length-masked mean pooling of the reference's MultiBench ``evaluate`` (train.py:120-125) and, with
``lengths=None``, the plain ``mean(axis=1)`` of ``evaluate_raw_data``.  ``LogisticProbe`` is the binary
``LogisticRegression`` that ``evaluate`` fits (train.py:97-99): ``kind='lbfgs'`` for ``LogisticRegression(max_iter=200)``,
``kind='liblinear'`` for ``make_pipeline(StandardScaler(), LogisticRegression(max_iter=1000, solver='liblinear'))``.  It
returns the optimum of sklearn's objective, not sklearn's last iterate.  ``KNeighborsProbe`` is the ``KNeighborsClassifier()``
of the same factory (train.py:99-100) on the kernels of umlh_kernels_knn.hip (``umlh_knn_*``).  Every call enqueues on
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
