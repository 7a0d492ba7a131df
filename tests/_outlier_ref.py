"""numpy float64 statement of the outlier-clamp contracts (include/umlh.h, section "outlier clamp and feature preparation";
the reference: vision_language/metrics.py:327-341 remove_outliers, :258-269 compute_knn_accuracy), the wrong variants a test
must tell apart from them, and the bounds the tests hold results to.

Contracts
  order statistics   s = np.sort(|x|) per flattened row (fp32, exact; NaN last); lo = floor(pos), hi = min(lo + 1, d - 1)
  interpolation      pos = q (d - 1) in double; quant = fp32(s[lo] + (s[hi] - s[lo]) (pos - lo)) formed in double; NaN for a row
                     that holds a NaN; mean64 = sum(quant) / n in double; q_val = fp32(mean64)
  exact bound        np.sort(|x|.ravel())[int(q * numel)]
  clamp              torch.clamp with tensor bounds: NaN x stays, NaN bound -> NaN, else min(max(x, -q), q) with std::max / std::min's
                     choice among equals
  normalisation      F.normalize(dim=-1): v / max(|v|_2, 1e-12), in float64

Bounds (measured by tests/test_outliers_cpu.py on the golden cases, which asserts that this table is what it measures; each is
8 x the worst value, rounded up to a power of two)

  quantity                                                          worst measured       bound
  row quantile, reference (pos in fp32) vs this statement, rel.      2^-19.7 (1.18e-06)   QUANT_BOUND = 2^-16
  q_val,        reference vs this statement, relative                2^-20.8 (5.59e-07)   QVAL_BOUND  = 2^-17
  normalise, fp32 numpy evaluation vs float64, max|.| / max|ref|     2^-22.9 (1.24e-07)   NORM_BOUND  = 2^-19

The first two are the reference's own rounding: torch.quantile forms pos = q (d - 1) and the interpolation weight in fp32, so the
weight carries an error of about 2^-24 pos, which (s[hi] - s[lo]) / s[lo] scales (worst on the 1100-wide and the heavy-tailed
cases).  The kernels are held to this statement bit for bit, not to these bounds; the bounds are for comparisons with the
reference's recorded values.

lo_val, hi_val, the exact-mode bound and the clamp are bit-equal to this statement; so is the clamped output whenever the bound
itself is (every exact case)."""
import math

import numpy as np

QUANT_BOUND = 2.0 ** -16
QVAL_BOUND = 2.0 ** -17
NORM_BOUND = 2.0 ** -19


def pow2_ceil(v: float) -> float:
    return 2.0 ** math.ceil(math.log2(v))


def rows2d(x):
    x = np.asarray(x)
    return x.reshape(x.shape[0], -1)


def positions(q: float, d: int):
    """(lo, hi, frac) of the quantile position pos = q (d - 1), all from Python floats (double)."""
    pos = float(q) * (d - 1)
    lo = min(int(math.floor(pos)), d - 1)
    return lo, min(lo + 1, d - 1), pos - lo


def interpolate(lo_val, hi_val, frac):
    a, b = np.asarray(lo_val, np.float64), np.asarray(hi_val, np.float64)
    with np.errstate(invalid="ignore"):
        return (a + (b - a) * frac).astype(np.float32)


def row_quantile(x, q):
    """dict(lo_val, hi_val, quant [n] fp32, mean64 float64, q_val fp32) of the contract."""
    x2 = rows2d(x).astype(np.float32)
    n, d = x2.shape
    s = np.sort(np.abs(x2), axis=1)
    lo, hi, frac = positions(q, d)
    quant = interpolate(s[:, lo], s[:, hi], frac)
    quant[np.isnan(x2).any(axis=1)] = np.nan
    mean64 = np.float64(quant.astype(np.float64).sum() / n)
    return {"lo_val": s[:, lo], "hi_val": s[:, hi], "quant": quant, "mean64": mean64, "q_val": np.float32(mean64)}


def abs_kth(x, k):
    return np.sort(np.abs(np.asarray(x, np.float32)).ravel())[k]


def exact_index(q, numel):
    return int(q * numel)


def clamp(x, q_val):
    x = np.asarray(x, np.float32)
    q = np.float32(q_val)
    if np.isnan(q):
        return np.full_like(x, np.nan)
    with np.errstate(invalid="ignore"):
        v = np.where(x < -q, -q, x)
        v = np.where(q < v, q, v)
    return v.astype(np.float32)


def normalize64(v, eps=1e-12):
    v = np.asarray(v, np.float64)
    nrm = np.sqrt((v * v).sum(axis=-1, keepdims=True))
    return v / np.maximum(nrm, eps)


def normalize32(v, eps=1e-12):
    """The same formulas evaluated in fp32 numpy: the yardstick of NORM_BOUND."""
    v = np.asarray(v, np.float32)
    nrm = np.sqrt((v * v).sum(axis=-1, keepdims=True, dtype=np.float32))
    return v / np.maximum(nrm, np.float32(eps))


def threshold(x, q, exact):
    return abs_kth(x, exact_index(q, np.asarray(x).size)) if exact else row_quantile(x, q)["q_val"]


def remove_outliers(x, q, exact=False):
    return clamp(x, threshold(x, q, exact))


def prepare_features(x, q, exact=False):
    return normalize64(remove_outliers(x, q, exact))


def knn_accuracy(knn):
    """the share of rows i that contain i"""
    k = rows2d(knn)
    return np.float64((k == np.arange(k.shape[0])[:, None]).any(axis=1).sum()) / k.shape[0]


def knn_accuracy_reference(knn):
    """compute_knn_accuracy as the reference evaluates it: knn == arange(n).view(-1, 1, 1) broadcasts a 2-D list [n, k] to
    [n, n, k], so there row i is compared with the WHOLE table (the share of indices found anywhere in it); for [n, k, k] it is
    knn_accuracy."""
    k = np.asarray(knn)
    if k.ndim == 2:
        return np.float64(np.isin(np.arange(k.shape[0]), k).sum()) / k.shape[0]
    return knn_accuracy(k)


def rel_diff(a, b):
    """max |a - b| / |b| over the finite entries (0 where both are 0); NaN patterns must agree."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN patterns differ"
    m = np.isfinite(a) & np.isfinite(b) & (b != 0)
    rest = ~m & ~np.isnan(b)
    assert np.array_equal(a[rest], b[rest]), "non-finite or zero entries differ"
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m]))) if m.any() else 0.0


def max_rel(got, ref):
    """max |got - ref| / max |ref| (the normalise metric)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(got - ref).max() / (scale if scale > 0 else 1.0))


# ---- wrong variants: each must miss a bound by at least 8 x on some golden case ----
def wrong_signed_quantile(x, q):
    """quantile of x instead of |x|"""
    x2 = rows2d(x).astype(np.float32)
    lo, hi, frac = positions(q, x2.shape[1])
    s = np.sort(x2, axis=1)
    quant = interpolate(s[:, lo], s[:, hi], frac)
    return np.float32(quant.astype(np.float64).mean())


def wrong_pos_qd(x, q):
    """pos = q d instead of q (d - 1)"""
    x2 = rows2d(x).astype(np.float32)
    d = x2.shape[1]
    pos = float(q) * d
    lo = min(int(math.floor(pos)), d - 1)
    hi = min(lo + 1, d - 1)
    s = np.sort(np.abs(x2), axis=1)
    quant = interpolate(s[:, lo], s[:, hi], pos - lo)
    return np.float32(quant.astype(np.float64).mean())


def wrong_nearest_rank(x, q):
    """nearest rank instead of interpolation"""
    x2 = rows2d(x).astype(np.float32)
    d = x2.shape[1]
    s = np.sort(np.abs(x2), axis=1)
    return np.float32(s[:, min(int(round(float(q) * (d - 1))), d - 1)].astype(np.float64).mean())


def wrong_per_row_bound(x, q):
    """every row clamped at its own quantile instead of the mean over rows"""
    x = np.asarray(x, np.float32)
    quant = row_quantile(x, q)["quant"]
    out = np.stack([clamp(r, b) for r, b in zip(rows2d(x), quant)])
    return out.reshape(x.shape)


def wrong_exact_index(x, q):
    """exact index k - 1"""
    return abs_kth(x, max(exact_index(q, np.asarray(x).size) - 1, 0))


def wrong_normalize_first(x, q, exact=False):
    """normalise before the clamp"""
    return clamp(normalize64(np.asarray(x, np.float32)).astype(np.float32), threshold(x, q, exact)).astype(np.float64)
