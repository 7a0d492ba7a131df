"""Representation-alignment metrics on the HIP kernels of umlh_kernels_align.hip (C ABI: ``umlh_align_*``).

``knn`` is the reference's ``compute_nearest_neighbors`` (vision_language/metrics.py:272-285), ``mutual_knn`` its
``AlignmentMetrics.mutual_knn`` (:55-84) and ``cka`` its ``AlignmentMetrics.cka(kernel_metric='ip', unbiased=False)``
(:96-119, :252-255).  Every call enqueues on ``torch.cuda.current_stream`` and returns device tensors without
synchronising.  Inputs: fp32 CUDA tensors with unit column stride are used in place (the row stride is passed on);
other float dtypes are upcast and CPU tensors copied to the current device.  There is no CPU compute path.
``measure_pairs`` (C ABI: ``umlh_align_pairs``) gives ``cka_terms`` and ``mutual_knn`` of many pairs in at most ten launches,
bit for bit the values of the single calls.

The kernels of umlh_kernels_align_ext.hip add the rest of the reference's ``AlignmentMetrics``: ``unbiased_cka`` (:122-125
with hsic_unbiased :230-249), ``rbf_cka`` (``cka(kernel_metric='rbf')``, biased and unbiased, :103-119), ``cknna`` (:180-227),
``cycle_knn`` (:39-51), ``lcs_knn`` (:88-92) and ``edit_distance_knn`` (:164-176), and ``measure`` dispatches the reference's
metric names and keyword arguments to all of them.  Not built: the ``distance_agnostic`` / biased CKNNA.

The kernels of umlh_kernels_outlier.hip (C ABI: ``umlh_row_abs_quantile``, ``umlh_abs_kth``, ``umlh_clamp_rows``,
``umlh_knn_accuracy``) are the module-level preprocessing of that file: ``remove_outliers`` (:327-341) with its
two thresholds ``row_abs_quantile`` and ``abs_kth`` (a radix select, no sort), ``prepare_features`` (clamp and
``F.normalize(dim=-1)`` in one launch) and ``knn_accuracy`` (``compute_knn_accuracy``, :258-269).  These take inputs of any
``ndim >= 2``: the trailing dimensions are flattened from dim 1 as a view when the tensor is contiguous.

``svcca`` (:129-160) runs on the kernels of umlh_kernels_spectral.hip (C ABI: ``umlh_svcca``) in closed form: see its
docstring and DESIGN section 13.  ``measure("svcca", ...)`` is not routed to it yet and still raises NotImplementedError.
"""
from __future__ import annotations

import math

import torch

from . import _glue as glue
from . import spectral
from ._lib import ALIGN_MAX_PAIRS, AlignPair, UmlhError, check, load_library

MAX_TOPK = 32


def _device() -> torch.device:
    return glue.device("umlh.align", "the metrics run only as HIP kernels")


def _check_topk(topk: int, n: int, what: str) -> None:
    if not 1 <= topk <= MAX_TOPK:
        raise ValueError(f"{what}: topk={topk} outside 1..{MAX_TOPK}")
    if topk >= n:
        raise ValueError(f"{what}: topk={topk} needs more than topk rows (got N={n})")


def _check_pair(a, b, what: str, splits: int, min_rows: int = 1) -> None:
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)) or a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
        raise ValueError(f"{what}: features of shapes {tuple(getattr(a, 'shape', ()))} and {tuple(getattr(b, 'shape', ()))} "
                         "(need 2-D with the same N)")
    if splits < 0:
        raise ValueError(f"{what}: splits={splits} < 0")
    if a.shape[0] < min_rows:
        raise ValueError(f"{what}: N={a.shape[0]} rows, the unbiased HSIC divides by N - 3 (need N >= {min_rows})")


def knn(feats: torch.Tensor, topk: int, splits: int = 0, return_scores: bool = False):
    """Per row i, the ``topk`` columns j != i with the largest raw inner product feats_i . feats_j, ordered by
    (score desc, index asc): int32 [N, topk] on the device (and the fp32 scores when ``return_scores``)."""
    if not isinstance(feats, torch.Tensor) or feats.ndim != 2:
        raise ValueError(f"knn: expected a 2-D tensor [N, d], got {getattr(feats, 'shape', type(feats))}")
    n = feats.shape[0]
    _check_topk(int(topk), n, "knn")
    if splits < 0:
        raise ValueError(f"knn: splits={splits} < 0")
    dev = _device()
    x = glue.features(feats, "knn", dev)
    lib = load_library()
    d = x.shape[1]
    scratch, nbytes = glue.scratch("umlh_align_scratch_bytes", dev, n=n, d_a=d, d_b=d, topk=topk, splits=splits)
    out = torch.empty((n, topk), dtype=torch.int32, device=dev)
    scores = torch.empty((n, topk), dtype=torch.float32, device=dev) if return_scores else None
    check(lib.umlh_align_knn(x.data_ptr(), n, d, x.stride(0), topk, splits, out.data_ptr(), glue.ptr(scores), scratch.data_ptr(),
                             nbytes, glue.stream(dev)), "umlh_align_knn")
    return (out, scores) if return_scores else out


def mutual_knn_lists(knn_a: torch.Tensor, knn_b: torch.Tensor) -> torch.Tensor:
    """Mean over rows of |knn_a(i) n knn_b(i)| / k for two int32 [N, k] neighbour lists: a 0-d float64 device tensor."""
    if knn_a.shape != knn_b.shape or knn_a.ndim != 2:
        raise ValueError(f"mutual_knn: neighbour lists of shapes {tuple(knn_a.shape)} and {tuple(knn_b.shape)}")
    dev = _device()
    n, topk = knn_a.shape
    _check_topk(topk, n, "mutual_knn")
    ka = knn_a.to(device=dev, dtype=torch.int32).contiguous()
    kb = knn_b.to(device=dev, dtype=torch.int32).contiguous()
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_align_scratch_bytes", dev, n=n, d_a=1, d_b=1, topk=0, splits=0)
    out = torch.empty((), dtype=torch.float64, device=dev)
    check(lib.umlh_align_mutual_knn(ka.data_ptr(), kb.data_ptr(), n, topk, out.data_ptr(), scratch.data_ptr(), nbytes,
                                    glue.stream(dev)), "umlh_align_mutual_knn")
    return out


def mutual_knn(a: torch.Tensor, b: torch.Tensor, topk: int = 10, splits: int = 0) -> torch.Tensor:
    """AlignmentMetrics.mutual_knn(a, b, topk): a 0-d float64 device tensor."""
    _check_pair(a, b, "mutual_knn", splits)
    _check_topk(int(topk), a.shape[0], "mutual_knn")
    return mutual_knn_lists(knn(a, topk, splits), knn(b, topk, splits))


def cka_terms(a: torch.Tensor, b: torch.Tensor, splits: int = 0) -> torch.Tensor:
    """float64 device tensor [4] = {cka, hsic_kl, hsic_kk, hsic_ll} (biased HSIC, linear kernel, no normalisation)."""
    _check_pair(a, b, "cka", splits)
    dev = _device()
    xa, xb = glue.features(a, "cka", dev), glue.features(b, "cka", dev)
    n = xa.shape[0]
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_align_scratch_bytes", dev, n=n, d_a=xa.shape[1], d_b=xb.shape[1], topk=0, splits=splits)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    check(lib.umlh_align_cka(xa.data_ptr(), xa.stride(0), xa.shape[1], xb.data_ptr(), xb.stride(0), xb.shape[1], n, splits,
                             out.data_ptr(), scratch.data_ptr(), nbytes, glue.stream(dev)), "umlh_align_cka")
    return out


def cka(a: torch.Tensor, b: torch.Tensor, splits: int = 0) -> torch.Tensor:
    """AlignmentMetrics.cka(a, b, kernel_metric='ip'): a 0-d float64 device tensor."""
    return cka_terms(a, b, splits)[0]


# ---- many pairs in one fixed train of launches (umlh_align_pairs) ----
_PAIR_SCRATCH = {}      # (device, stream, splits, member signature) -> (uint8 device tensor, its size)


def _pair_scratch(dev, items, n, splits, signature):
    """Scratch of one umlh_align_pairs call, leased per (device, stream, group signature): calls on one stream run in order."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, splits) + signature
    hit = _PAIR_SCRATCH.get(key)
    if hit is None:
        nbytes = load_library().umlh_align_pairs_scratch(items, n, splits)
        if nbytes == 0:
            raise UmlhError(f"umlh_align_pairs_scratch: invalid arguments n_items={n} splits={splits} members={signature}")
        if len(_PAIR_SCRATCH) >= 16:
            _PAIR_SCRATCH.clear()
        hit = _PAIR_SCRATCH[key] = (torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes)
    return hit


def measure_pairs(pairs, topk: int = 10, cka: bool = True, splits: int = 0, return_lists: bool = False):
    """``cka_terms(a, b)`` and ``mutual_knn(a, b, topk)`` of many feature pairs at once: a float64 device tensor [G, 5] =
    {cka, hsic_kl, hsic_kk, hsic_ll, mutual_knn} per pair, every word bit for bit what the single calls give with the same
    ``splits``.  The whole group takes at most ten launches, whatever G is (more than 64 pairs: consecutive groups of 64).

    ``pairs``: a list of ``(a, b)`` or ``(a, b, {"topk": ..., "cka": ...})``; the dict overrides the call's ``topk`` / ``cka`` for
    that pair.  ``topk=0`` skips the mutual k-NN and ``cka=False`` the CKA of a pair: its columns are NaN.  Pairs may differ in
    every shape and may share tensors.  ``return_lists``: also a list with, per pair, ``(knn_a, scores_a, knn_b, scores_b)`` as
    ``knn(..., return_scores=True)`` returns them (None for a pair without lists)."""
    what = "measure_pairs"
    pairs = list(pairs)
    if not pairs:
        raise ValueError(f"{what}: no pairs")
    if splits < 0:
        raise ValueError(f"{what}: splits={splits} < 0")
    members = []
    for i, pr in enumerate(pairs):
        who = f"{what}: member {i}"
        if not isinstance(pr, (tuple, list)) or len(pr) not in (2, 3) or (len(pr) == 3 and not isinstance(pr[2], dict)):
            raise ValueError(f"{who}: expected (a, b) or (a, b, {{'topk': ..., 'cka': ...}})")
        opts = dict(pr[2]) if len(pr) == 3 else {}
        unknown = set(opts) - {"topk", "cka"}
        if unknown:
            raise ValueError(f"{who}: unknown options {sorted(unknown)}")
        k, c = int(opts.get("topk", topk)), bool(opts.get("cka", cka))
        _check_pair(pr[0], pr[1], who, splits)
        if k != 0:
            _check_topk(k, pr[0].shape[0], who)
        if k == 0 and not c:
            raise ValueError(f"{who}: cka=False and topk=0 ask for nothing")
        members.append((pr[0], pr[1], k, c))
    dev = _device()
    lib = load_library()
    if all(k != 0 and c for _, _, k, c in members):                  # every word is written: no fill
        out = torch.empty((len(members), 5), dtype=torch.float64, device=dev)
    else:
        out = torch.full((len(members), 5), math.nan, dtype=torch.float64, device=dev)
    lists = []
    for g0 in range(0, len(members), ALIGN_MAX_PAIRS):
        group = members[g0:g0 + ALIGN_MAX_PAIRS]
        items = (AlignPair * len(group))()
        keep, sig = [], []
        for i, (it, (a, b, k, c)) in enumerate(zip(items, group)):
            xa, xb = glue.features(a, f"{what}: member {g0 + i}", dev), glue.features(b, f"{what}: member {g0 + i}", dev)
            n = xa.shape[0]
            it.a, it.lda, it.d_a = xa.data_ptr(), xa.stride(0), xa.shape[1]
            it.b, it.ldb, it.d_b = xb.data_ptr(), xb.stride(0), xb.shape[1]
            it.n, it.cka, it.topk = n, int(c), k
            it.out5 = out[g0 + i].data_ptr()
            got = None
            if return_lists and k:
                got = (torch.empty((n, k), dtype=torch.int32, device=dev), torch.empty((n, k), dtype=torch.float32, device=dev),
                       torch.empty((n, k), dtype=torch.int32, device=dev), torch.empty((n, k), dtype=torch.float32, device=dev))
                it.knn_a, it.scores_a, it.knn_b, it.scores_b = (t.data_ptr() for t in got)
            lists.append(got)
            keep.append((xa, xb))
            sig.append((n, it.d_a, it.d_b, k, int(c), got is not None))
        scratch, nbytes = _pair_scratch(dev, items, len(group), splits, tuple(sig))
        check(lib.umlh_align_pairs(items, len(group), splits, scratch.data_ptr(), nbytes, glue.stream(dev)), "umlh_align_pairs")
    return (out, lists) if return_lists else out


# ---- unbiased / RBF CKA, CKNNA and the list statistics (umlh_kernels_align_ext.hip) ----
KIND_CKA_UNBIASED, KIND_CKA_RBF, KIND_CKNNA, KIND_LIST_STATS = range(4)


def unbiased_cka_terms(a: torch.Tensor, b: torch.Tensor, splits: int = 0) -> torch.Tensor:
    """float64 device tensor [4] = {cka, hsic_kl, hsic_kk, hsic_ll} with the unbiased HSIC of the linear kernel."""
    _check_pair(a, b, "unbiased_cka", splits, 4)
    dev = _device()
    xa, xb = glue.features(a, "unbiased_cka", dev), glue.features(b, "unbiased_cka", dev)
    n = xa.shape[0]
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_align_ext_scratch_bytes", dev, kind=KIND_CKA_UNBIASED, n=n, d_a=xa.shape[1], d_b=xb.shape[1],
                                   topk=0, splits=splits)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    check(lib.umlh_align_cka_unbiased(xa.data_ptr(), xa.stride(0), xa.shape[1], xb.data_ptr(), xb.stride(0), xb.shape[1], n, splits,
                                      out.data_ptr(), scratch.data_ptr(), nbytes, glue.stream(dev)), "umlh_align_cka_unbiased")
    return out


def unbiased_cka(a: torch.Tensor, b: torch.Tensor, splits: int = 0) -> torch.Tensor:
    """AlignmentMetrics.unbiased_cka(a, b): a 0-d float64 device tensor."""
    return unbiased_cka_terms(a, b, splits)[0]


def rbf_cka_terms(a: torch.Tensor, b: torch.Tensor, sigma: float = 1.0, unbiased: bool = False, splits: int = 0) -> torch.Tensor:
    """float64 device tensor [4] = {cka, hsic_kl, hsic_kk, hsic_ll} for K_ij = exp(-|a_i - a_j|^2 / (2 sigma^2))."""
    _check_pair(a, b, "rbf_cka", splits, 4 if unbiased else 1)
    sigma = float(sigma)
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise ValueError(f"rbf_cka: sigma={sigma} (need a finite sigma > 0)")
    dev = _device()
    xa, xb = glue.features(a, "rbf_cka", dev), glue.features(b, "rbf_cka", dev)
    n = xa.shape[0]
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_align_ext_scratch_bytes", dev, kind=KIND_CKA_RBF, n=n, d_a=xa.shape[1], d_b=xb.shape[1],
                                   topk=0, splits=splits)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    check(lib.umlh_align_cka_rbf(xa.data_ptr(), xa.stride(0), xa.shape[1], xb.data_ptr(), xb.stride(0), xb.shape[1], n, sigma,
                                 int(bool(unbiased)), splits, out.data_ptr(), scratch.data_ptr(), nbytes, glue.stream(dev)),
          "umlh_align_cka_rbf")
    return out


def rbf_cka(a: torch.Tensor, b: torch.Tensor, sigma: float = 1.0, unbiased: bool = False, splits: int = 0) -> torch.Tensor:
    """AlignmentMetrics.cka(a, b, kernel_metric='rbf', rbf_sigma=sigma, unbiased=unbiased): a 0-d float64 device tensor."""
    return rbf_cka_terms(a, b, sigma, unbiased, splits)[0]


def _check_cknna_topk(topk: int, n: int) -> None:
    if topk < 2:
        raise ValueError(f"CKNNA requires topk >= 2 (topk={topk})")
    _check_topk(topk, n, "cknna")
    if n < 4:
        raise ValueError(f"cknna: N={n} rows, the unbiased HSIC divides by N - 3 (need N >= 4)")


def cknna_terms(a: torch.Tensor, b: torch.Tensor, topk: int, splits: int = 0) -> torch.Tensor:
    """float64 device tensor [4] = {cknna, sim_kl, sim_kk, sim_ll} (unbiased, not distance agnostic)."""
    _check_pair(a, b, "cknna", splits)
    topk = int(topk)
    n = a.shape[0]
    _check_cknna_topk(topk, n)
    ka, sa = knn(a, topk, splits, return_scores=True)
    kb, sb = knn(b, topk, splits, return_scores=True)
    dev = ka.device
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_align_ext_scratch_bytes", dev, kind=KIND_CKNNA, n=n, d_a=1, d_b=1, topk=topk, splits=0)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    check(lib.umlh_align_cknna(ka.data_ptr(), sa.data_ptr(), kb.data_ptr(), sb.data_ptr(), n, topk, out.data_ptr(),
                               scratch.data_ptr(), nbytes, glue.stream(dev)), "umlh_align_cknna")
    return out


def cknna(a: torch.Tensor, b: torch.Tensor, topk: int, splits: int = 0) -> torch.Tensor:
    """AlignmentMetrics.cknna(a, b, topk): a 0-d float64 device tensor."""
    return cknna_terms(a, b, topk, splits)[0]


def list_stats(knn_a: torch.Tensor, knn_b: torch.Tensor, return_rows: bool = False):
    """float64 device tensor [3] = {cycle_knn, lcs_knn, edit_distance_knn} of two int32 [N, k] neighbour lists (and the
    per-row int32 [N, 3] = {hit, LCS length, Levenshtein distance} when ``return_rows``)."""
    if not (isinstance(knn_a, torch.Tensor) and isinstance(knn_b, torch.Tensor)) or knn_a.shape != knn_b.shape or knn_a.ndim != 2:
        raise ValueError(f"list_stats: neighbour lists of shapes {tuple(getattr(knn_a, 'shape', ()))} and "
                         f"{tuple(getattr(knn_b, 'shape', ()))}")
    n, topk = knn_a.shape
    _check_topk(topk, n, "list_stats")
    dev = _device()
    ka = knn_a.to(device=dev, dtype=torch.int32).contiguous()
    kb = knn_b.to(device=dev, dtype=torch.int32).contiguous()
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_align_ext_scratch_bytes", dev, kind=KIND_LIST_STATS, n=n, d_a=1, d_b=1, topk=topk, splits=0)
    out = torch.empty(3, dtype=torch.float64, device=dev)
    rows = torch.empty((n, 3), dtype=torch.int32, device=dev) if return_rows else None
    check(lib.umlh_align_list_stats(ka.data_ptr(), kb.data_ptr(), n, topk, glue.ptr(rows), out.data_ptr(), scratch.data_ptr(), nbytes,
                                    glue.stream(dev)), "umlh_align_list_stats")
    return (out, rows) if return_rows else out


def _list_stat(a, b, topk, splits, which, what):
    _check_pair(a, b, what, splits)
    _check_topk(int(topk), a.shape[0], what)
    return list_stats(knn(a, topk, splits), knn(b, topk, splits))[which]


def cycle_knn(a: torch.Tensor, b: torch.Tensor, topk: int, splits: int = 0) -> torch.Tensor:
    """AlignmentMetrics.cycle_knn(a, b, topk): the share of rows i found among knn_a[knn_b[i]]; a 0-d float64 device tensor."""
    return _list_stat(a, b, topk, splits, 0, "cycle_knn")


def lcs_knn(a: torch.Tensor, b: torch.Tensor, topk: int, splits: int = 0) -> torch.Tensor:
    """AlignmentMetrics.lcs_knn(a, b, topk): the mean LCS length of the two neighbour lists (not divided by topk)."""
    return _list_stat(a, b, topk, splits, 1, "lcs_knn")


def edit_distance_knn(a: torch.Tensor, b: torch.Tensor, topk: int, splits: int = 0) -> torch.Tensor:
    """AlignmentMetrics.edit_distance_knn(a, b, topk): 1 - mean Levenshtein distance of the two neighbour lists / topk."""
    return _list_stat(a, b, topk, splits, 2, "edit_distance_knn")


SUPPORTED_METRICS = ("cycle_knn", "mutual_knn", "lcs_knn", "cka", "unbiased_cka", "cknna", "svcca", "edit_distance_knn")


def _cka_any(feats_A, feats_B, kernel_metric="ip", rbf_sigma=1.0, unbiased=False):
    if kernel_metric == "ip":
        return unbiased_cka(feats_A, feats_B) if unbiased else cka(feats_A, feats_B)
    if kernel_metric == "rbf":
        return rbf_cka(feats_A, feats_B, rbf_sigma, unbiased)
    raise ValueError(f"Invalid kernel metric {kernel_metric}")


def _cknna_any(feats_A, feats_B, topk=None, distance_agnostic=False, unbiased=True):
    if distance_agnostic:
        raise NotImplementedError("cknna(distance_agnostic=True) is not built: the reference itself raises there (it calls "
                                  ".item() on an N x N tensor)")
    if not unbiased:
        raise NotImplementedError("cknna(unbiased=False) is not built: it needs a top-k that includes self and the dense "
                                  "centred HSIC")
    if topk is None:
        raise ValueError("cknna: topk is required (1 < topk <= 32)")
    return cknna(feats_A, feats_B, topk)


def svcca_terms(a: torch.Tensor, b: torch.Tensor, cca_dim: int = 10):
    """``(value, rho[q], evals[2, q])`` of ``svcca`` with q = cca_dim: the mean canonical correlation (0-d), the canonical
    correlations (descending, clamped to [0, 1]) and the top-q eigenvalues of the two standardised Grams; float64 device tensors."""
    _check_pair(a, b, "svcca", 0)
    n, d_a = spectral.check_view(a, "svcca")
    _, d_b = spectral.check_view(b, "svcca")
    q = spectral.check_q(cca_dim, min(n, d_a, d_b), "svcca")
    dev = _device()
    xa, xb = spectral.rows_in_place(a, dev), spectral.rows_in_place(b, dev)
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_subspace_scratch_bytes", dev, n=n, d_a=d_a, d_b=d_b, q=q)
    out = torch.empty((), dtype=torch.float64, device=dev)
    rho = torch.empty(q, dtype=torch.float64, device=dev)
    evals = torch.empty((2, q), dtype=torch.float64, device=dev)
    check(lib.umlh_svcca(xa.data_ptr(), xb.data_ptr(), n, d_a, d_b, xa.stride(0), xb.stride(0), q, out.data_ptr(), rho.data_ptr(),
                         evals.data_ptr(), scratch.data_ptr(), nbytes, glue.stream(dev)), "umlh_svcca")
    return out, rho, evals


def svcca(a: torch.Tensor, b: torch.Tensor, cca_dim: int = 10) -> torch.Tensor:
    """AlignmentMetrics.svcca(a, b, cca_dim) (MultiBench/metrics.py:129-160) in closed form: a 0-d float64 device tensor.

    The reference standardises every column ((x - mean) / (unbiased std + 1e-8)), takes the top-q left singular vectors of each
    view with a randomised SVD and runs scikit-learn's CCA on them.  Those bases are centred and orthonormal and CCA does not
    change under an invertible map of either one, so its value is the mean singular value of U_a^T U_b.  This is computed
    from the two d x d standardised Grams, their top-q eigenpairs and the d_a x d_b cross-Gram, all in fp64; nothing N x q is
    formed.  2 <= N < 2^31, d <= 512, cca_dim <= min(N, d_a, d_b, 64).

    * The value equals the reference's when sigma_q > sigma_(q+1) in both standardised views.  At a tie the subspace is not
      unique: the reference's value then depends on its random test matrix; this one is deterministic but arbitrary.
    * NaN when the numerical rank of a view is below q (lambda_q <= d 2^-53 lambda_1, an all-constant view included; the
      reference returns noise there) and when an input holds a NaN or Inf.
    * The reference's 1e-10 * randn jitter (:153-154) has no counterpart."""
    return svcca_terms(a, b, cca_dim)[0]


def _svcca(*args, **kwargs):
    raise NotImplementedError("svcca is not routed through measure(): call umlh.align.svcca(a, b, cca_dim), the closed-form "
                              "fp64 HIP path")


def measure(metric: str, feats_A: torch.Tensor, feats_B: torch.Tensor, **kwargs) -> float:
    """AlignmentMetrics.measure(metric, feats_A, feats_B, **kwargs) (metrics.py:28-35) with the reference's metric names and
    keyword arguments (topk, kernel_metric, rbf_sigma, unbiased, distance_agnostic); a Python float like its ``.item()``."""
    if metric not in SUPPORTED_METRICS:
        raise ValueError(f"Unrecognized metric: {metric}")
    fn = {"cycle_knn": cycle_knn, "mutual_knn": mutual_knn, "lcs_knn": lcs_knn, "edit_distance_knn": edit_distance_knn,
          "cka": _cka_any, "unbiased_cka": lambda a, b, **kw: _cka_any(a, b, **{**kw, "unbiased": True}),
          "cknna": _cknna_any, "svcca": _svcca}[metric]
    return float(fn(feats_A, feats_B, **kwargs).item())


# ---- outlier clamp and feature preparation (umlh_kernels_outlier.hip) ----
KIND_ROW_QUANTILE, KIND_ABS_KTH, KIND_KNN_ACCURACY = range(3)
ROW_QUANTILE_WAVE_COLS = 1024      # UMLH_ROW_QUANTILE_WAVE_COLS: up to here a wave per row, four rows per workgroup
ROW_QUANTILE_LDS_COLS = 15360      # UMLH_ROW_QUANTILE_LDS_COLS: up to here the row is read once and kept in LDS
MAX_ELEMENTS = 1 << 40


def _check_feats(feats, what: str) -> None:
    if not isinstance(feats, torch.Tensor) or feats.ndim < 2:
        raise ValueError(f"{what}: expected a tensor [N, ...] with ndim >= 2, got {getattr(feats, 'shape', type(feats))}")
    if not feats.is_floating_point():
        raise ValueError(f"{what}: expected a floating-point tensor, got {feats.dtype}")
    if feats.numel() == 0:
        raise ValueError(f"{what}: empty features {tuple(feats.shape)}")
    if feats.numel() >= MAX_ELEMENTS or feats.numel() // feats.shape[0] >= 1 << 31:
        raise ValueError(f"{what}: features {tuple(feats.shape)} outside the envelope (row width < 2^31, elements < 2^40)")


def _check_q(q, what: str, upper_ok: bool) -> float:
    q = float(q)
    if not (0.0 <= q < 1.0 or (upper_ok and q == 1.0)):
        raise ValueError(f"{what}: q={q} outside [0, 1{']' if upper_ok else ')'}")
    return q


def _rows(feats: torch.Tensor, what: str, dev: torch.device, width: int | None = None) -> torch.Tensor:
    """``feats`` as an fp32 device matrix [N, prod(rest)] (or [numel / width, width]): a view where the layout allows."""
    if feats.ndim == 2 and (width is None or width == feats.shape[1]):
        return glue.features(feats, what, dev)
    t = feats.detach().to(device=dev, dtype=torch.float32).contiguous()      # no copy when already fp32, on dev and contiguous
    return t.view(t.shape[0], -1) if width is None else t.view(-1, width)


def row_abs_quantile(feats: torch.Tensor, q: float, return_order_stats: bool = False):
    """``(q_val, mean64, quant)``: per row of ``feats.abs().flatten(start_dim=1)`` the interpolated quantile ``quant`` fp32 [N]
    (``torch.quantile(..., q, dim=1)``, interpolated in double from the two exact order statistics), its mean over rows in double
    (0-d float64) and that mean rounded once (0-d fp32, the clamp bound of ``remove_outliers``); with ``return_order_stats`` also
    ``lo_val, hi_val`` fp32 [N], the order statistics floor(q (d-1)) and the next.  0 <= q < 1."""
    _check_feats(feats, "row_abs_quantile")
    q = _check_q(q, "row_abs_quantile", False)
    dev = _device()
    x = _rows(feats, "row_abs_quantile", dev)
    n, d = x.shape
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_outlier_scratch_bytes", dev, kind=KIND_ROW_QUANTILE, n=n, d=d)
    quant = torch.empty(n, dtype=torch.float32, device=dev)
    lo = torch.empty(n, dtype=torch.float32, device=dev) if return_order_stats else None
    hi = torch.empty(n, dtype=torch.float32, device=dev) if return_order_stats else None
    mean64 = torch.empty((), dtype=torch.float64, device=dev)
    q_val = torch.empty((), dtype=torch.float32, device=dev)
    check(lib.umlh_row_abs_quantile(x.data_ptr(), n, d, x.stride(0), q, glue.ptr(lo), glue.ptr(hi), quant.data_ptr(),
                                    mean64.data_ptr(), q_val.data_ptr(), scratch.data_ptr(), nbytes, glue.stream(dev)),
          "umlh_row_abs_quantile")
    return (q_val, mean64, quant, lo, hi) if return_order_stats else (q_val, mean64, quant)


def abs_kth(feats: torch.Tensor, k: int) -> torch.Tensor:
    """``feats.view(-1).abs().sort().values[k]`` without the sort: a 0-d fp32 device tensor, bit-exact; NaNs order last."""
    _check_feats(feats, "abs_kth")
    k = int(k)
    if not 0 <= k < feats.numel():
        raise ValueError(f"abs_kth: k={k} outside 0..{feats.numel() - 1}")
    dev = _device()
    x = _rows(feats, "abs_kth", dev)
    n, d = x.shape
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_outlier_scratch_bytes", dev, kind=KIND_ABS_KTH, n=n, d=d)
    out = torch.empty((), dtype=torch.float32, device=dev)
    check(lib.umlh_abs_kth(x.data_ptr(), n, d, x.stride(0), k, out.data_ptr(), scratch.data_ptr(), nbytes, glue.stream(dev)),
          "umlh_abs_kth")
    return out


def _threshold(feats: torch.Tensor, q: float, exact: bool, what: str) -> torch.Tensor:
    """The clamp bound of ``remove_outliers`` as a 0-d fp32 device tensor (metrics.py:331-336); argument errors before any GPU use."""
    if exact:
        k = int(q * feats.numel())
        if not 0 <= k < feats.numel():
            raise ValueError(f"{what}: exact index int(q * numel) = {k} outside 0..{feats.numel() - 1}")
        return abs_kth(feats, k)
    return row_abs_quantile(feats, q)[0]


def _clamp(feats: torch.Tensor, q_val: torch.Tensor, normalize: bool, out, what: str) -> torch.Tensor:
    dev = q_val.device
    width = feats.shape[-1]
    x = _rows(feats, what, dev, width)
    n, d = x.shape
    if out is None:
        res = torch.empty(feats.shape, dtype=torch.float32, device=dev)
    else:
        if not isinstance(out, torch.Tensor) or out.shape != feats.shape or out.dtype != torch.float32 or out.device != dev:
            raise ValueError(f"{what}: out must be an fp32 tensor of shape {tuple(feats.shape)} on {dev}")
        if not (out.is_contiguous() or (out.ndim == 2 and out.stride(1) == 1 and out.stride(0) >= d)):
            raise ValueError(f"{what}: out must be contiguous or a 2-D tensor with unit column stride")
        res = out
    o = res if res.ndim == 2 else res.view(-1, width)
    if o.data_ptr() == x.data_ptr() and o.stride(0) != x.stride(0):
        raise ValueError(f"{what}: out aliases the input with another row stride")
    check(load_library().umlh_clamp_rows(x.data_ptr(), n, d, x.stride(0), q_val.data_ptr(), int(bool(normalize)), o.data_ptr(),
                                         o.stride(0), glue.stream(dev)), "umlh_clamp_rows")
    return res


def remove_outliers(feats: torch.Tensor, q: float, exact: bool = False, max_threshold=None, out: torch.Tensor | None = None):
    """``remove_outliers(feats, q, exact, max_threshold)`` (metrics.py:327-341): ``feats.clamp(-q_val, q_val)`` with ``q_val`` the
    mean over rows of the q-quantile of |feats| (``exact``: the element ``int(q * numel)`` of all sorted |feats|); an fp32 device
    tensor of ``feats``' shape, nothing is read back.  ``q == 1`` returns ``feats`` itself.  ``max_threshold`` is accepted and has
    no effect, as in the reference, which computes ``max(max_threshold, q_val)`` into a local it never uses (:338-339).  ``out``:
    where to write (``out=feats`` for fp32 device features clamps in place)."""
    _check_feats(feats, "remove_outliers")
    q = _check_q(q, "remove_outliers", True)
    if q == 1.0:
        return feats
    return _clamp(feats, _threshold(feats, q, bool(exact), "remove_outliers"), False, out, "remove_outliers")


def prepare_features(feats: torch.Tensor, q: float = 0.95, exact: bool = False, normalize: bool = True) -> torch.Tensor:
    """``F.normalize(remove_outliers(feats, q, exact), dim=-1)`` (what the reference's ``__main__`` and its callers do before
    measuring) with the clamp and the normalisation in one launch after the selection; ``normalize=False``: the clamp alone.
    ``q == 1`` keeps every value (an infinite bound).  An fp32 device tensor of ``feats``' shape."""
    _check_feats(feats, "prepare_features")
    q = _check_q(q, "prepare_features", True)
    if q == 1.0:
        q_val = torch.full((), math.inf, dtype=torch.float32, device=_device())
    else:
        q_val = _threshold(feats, q, bool(exact), "prepare_features")
    return _clamp(feats, q_val, bool(normalize), None, "prepare_features")


def knn_accuracy(knn_lists: torch.Tensor, whole_table: bool = False) -> torch.Tensor:
    """The share of rows i of an integer tensor [N, k] or [N, k, k] that contain the value i (``compute_knn_accuracy`` of
    metrics.py:258-269 on the [N, k, k] its caller passes); a 0-d float64 device tensor (integer hit count / N).
    ``whole_table``: the share of the indices 0 .. N-1 found anywhere in the tensor instead, which is what the reference's
    expression evaluates to for a 2-D list (its ``arange(n).view(-1, 1, 1)`` broadcasts [N, k] to [N, N, k])."""
    if not isinstance(knn_lists, torch.Tensor) or knn_lists.ndim < 2 or knn_lists.is_floating_point() or knn_lists.dtype == torch.bool:
        raise ValueError(f"knn_accuracy: expected an integer tensor [N, k] or [N, k, k], got {getattr(knn_lists, 'shape', type(knn_lists))} "
                         f"{getattr(knn_lists, 'dtype', '')}")
    if knn_lists.numel() == 0:
        raise ValueError(f"knn_accuracy: empty list {tuple(knn_lists.shape)}")
    dev = _device()
    k = knn_lists.to(device=dev, dtype=torch.int32).contiguous()
    n = k.shape[0]
    m, ld = (k.numel(), 0) if whole_table else (k.numel() // n, k.numel() // n)
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_outlier_scratch_bytes", dev, kind=KIND_KNN_ACCURACY, n=n, d=m)
    out = torch.empty((), dtype=torch.float64, device=dev)
    check(lib.umlh_knn_accuracy(k.data_ptr(), n, m, ld, out.data_ptr(), scratch.data_ptr(), nbytes, glue.stream(dev)), "umlh_knn_accuracy")
    return out
