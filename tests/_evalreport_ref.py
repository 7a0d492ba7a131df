"""Float64 restatement of the class-wise validation report (umlh.topk_classes / umlh.class_report, umlh_eval_topk /
umlh_eval_classwise of include/umlh.h), numpy only.  The reference project has no class-wise code: this file is the yardstick.

Logits are z_ij = scale * (x_i . w_j + b_j) in float64 from the fp32 inputs; a row's list is its k classes with the largest z
ordered by (z descending, class index ascending); a class whose z is NaN is never listed and the slots left open hold class -1
and a NaN logit.  ``report`` counts, per true class, the rows (support), the rows whose first listed class is the label (hit1),
the rows whose label is anywhere in the list (hitk) and, optionally, the confusion matrix (row = true class, column = first
listed class); rows with a label outside [0, C) count in misc[0] alone, rows with a valid label but no first class (-1) in
support and misc[1] alone.

SHARPNESS.  The device picks kc = min(k + 8, C) candidates from an fp32 score and re-ranks them in fp64, so a row's list is
certain only if all of its k best classes reach the candidate set: a row is sharp when
    u_(k) - u_(kc+1)  >  TAU * (|x| max_j |w_j| + max_j |b_j|)            (float64, u = the unscaled x.w_j + b_j, negated for a
negative scale, sorted descending; C <= kc: every class is a candidate, every row is sharp).  Inside the candidate set the device
order is fp64 and must match outright.  TAU is 8 x the largest relative error, against that same magnitude, that an fp32 numpy
evaluation of x.w + b reaches against float64 over CASES, rounded up to a power of two (the convention of _knn_ref.py and
_encoder_ref.py).  tests/test_evalreport_cpu.py re-measures it: the largest error of a case is at most 2^-22.92 (case 04, 257 x
256 classes x d = 64; most cases lie between 2^-25 and 2^-23), and 8 x 2^-22.92 = 2^-19.92 rounds up to 2^-19.  At
2^-19 no row of any case is non-sharp.
"""
import itertools

import numpy as np

TAU = 2.0 ** -19
CAP = 0.02                   # at most this fraction of a case's rows may be non-sharp
MARGIN = 8                   # candidates the device keeps beyond k

TOPK_VARIANTS = ("tie_larger_index", "bias_dropped", "scale_sign_ignored")
REPORT_VARIANTS = ("confusion_transposed", "hitk_short", "bad_labels_counted")

# ---- the shape grid: every value of every axis, every (k, C) pair and every (d, layout) pair appears (checked by the CPU test) ----
NS = (1, 31, 32, 33, 257)                                    # the 32-row strip edges; more than one strip
KS = (1, 5, 24)
C_OF_K = ("k", "k+8", "k+9", 255, 256, 257, 513)             # no (k+1)-th class; kc = C; the first C > kc; tile edges; three tiles
DS = (1, 3, 8, 9, 64, 515)
SCALES = (None, 100.0, -2.5)
LAYOUTS = ("dense", "strided")                               # strided: ld > d and a base offset of one float (the 4-byte load path)


def _cases():
    out = []
    for i, (layout, (k, c)) in enumerate(itertools.product(LAYOUTS, itertools.product(KS, C_OF_K))):
        C = {"k": k, "k+8": k + 8, "k+9": k + 9}.get(c, c)
        out.append(dict(name=f"{i:02d}", seed=100 + i, n=NS[i % 5], C=C, d=DS[i % 6], k=k, bias=bool((i // 2) % 2),
                        scale=SCALES[(i // 3) % 3], layout=layout))
    return out


CASES = _cases()


def case_data(case):
    """(x [n, d], w [C, d], b [C] or None) fp32 of a case: standard normal features and weights, a bias of the logits' size."""
    rng = np.random.default_rng(case["seed"])
    x = rng.standard_normal((case["n"], case["d"])).astype(np.float32)
    w = rng.standard_normal((case["C"], case["d"])).astype(np.float32)
    b = (np.sqrt(case["d"]) * rng.standard_normal(case["C"])).astype(np.float32) if case["bias"] else None
    return x, w, b


def integer_cases():
    """name -> (x, w, b, scale, k): small integers, so every product, sum and logit is exact in fp32 and in fp64 and ties are
    certain -- heavy duplicates, an all-equal row (x = 0: every class ties), identical weight rows."""
    rng = np.random.default_rng(7)
    out = {}
    x = rng.integers(-2, 3, (70, 6)).astype(np.float32)
    w = rng.integers(-1, 2, (300, 6)).astype(np.float32)
    out["duplicates"] = (x, w, rng.integers(-1, 2, 300).astype(np.float32), None, 5)
    x0 = x.copy()
    x0[3] = 0
    x0[40] = 0
    out["all_equal_row"] = (x0, w, None, 100.0, 24)
    wi = rng.integers(-3, 4, (530, 9)).astype(np.float32)
    wi[17] = wi[400] = wi[2]
    wi[511:514] = wi[255]
    out["identical_weight_rows"] = (rng.integers(-3, 4, (33, 9)).astype(np.float32), wi, rng.integers(-2, 3, 530).astype(np.float32), -2.5, 5)
    return out


def logits64(x, w, b=None, scale=None):
    """float64 [n, C]: scale * (x @ w.T + b)."""
    u = np.asarray(x, np.float64) @ np.asarray(w, np.float64).T
    if b is not None:
        u = u + np.asarray(b, np.float64)[None, :]
    return u if scale is None else float(scale) * u


def topk(x, w, b=None, scale=None, k=5, variant=None):
    """(cls int64 [n, k], z float64 [n, k]) by (z desc, class index asc); NaN logits are never listed (class -1, NaN).
    ``variant``: one of TOPK_VARIANTS, a deliberately wrong statement."""
    z = logits64(x, w, None if variant == "bias_dropped" else b, abs(scale) if variant == "scale_sign_ignored" and scale is not None else scale)
    n, C = z.shape
    key = np.where(np.isnan(z), -np.inf, z)
    cols = np.broadcast_to(np.arange(C), z.shape)
    order = np.lexsort((-cols if variant == "tie_larger_index" else cols, -key), axis=1)[:, :k]
    cls, val = order.astype(np.int64), np.take_along_axis(z, order, 1)
    cls[np.isnan(val)] = -1
    return cls, val


def report(cls, labels, C, confusion=False, variant=None):
    """dict of int64 arrays: support, hit1, hitk [C], misc [2] and, when asked for, confusion [C, C]."""
    cls, y = np.asarray(cls, np.int64), np.asarray(labels, np.int64)
    if variant == "bad_labels_counted":
        y = np.clip(y, 0, C - 1)
    ok = (y >= 0) & (y < C)
    pred = cls[:, 0]
    has = ok & (pred >= 0) & (pred < C)
    lists = cls[:, :-1] if variant == "hitk_short" else cls
    out = {"support": np.bincount(y[ok], minlength=C), "hit1": np.bincount(y[has & (pred == y)], minlength=C),
           "hitk": np.bincount(y[has & (lists == y[:, None]).any(1)], minlength=C),
           "misc": np.array([(~ok).sum(), (ok & ~has).sum()], np.int64)}
    if confusion:
        a, p = (pred[has], y[has]) if variant == "confusion_transposed" else (y[has], pred[has])
        out["confusion"] = np.bincount(a * C + p, minlength=C * C).reshape(C, C)
    return {k_: v.astype(np.int64) for k_, v in out.items()}


def magnitude(x, w, b=None):
    """float64 [n]: |x| max_j |w_j| + max_j |b_j|, what the rounding of the fp32 score is relative to."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    m = np.sqrt((x64 * x64).sum(1)) * np.sqrt((w64 * w64).sum(1)).max()
    return m + (np.abs(np.asarray(b, np.float64)).max() if b is not None else 0.0)


def sharp(x, w, b, k, scale=None, tau=TAU):
    """bool [n]: the k-th best unscaled value beats the (kc + 1)-th by more than tau * magnitude (all rows when C <= kc)."""
    C = len(w)
    kc = min(k + MARGIN, C)
    if C <= kc:
        return np.ones(len(x), bool)
    u = logits64(x, w, b)
    u = np.sort(-u if scale is not None and scale < 0 else u, axis=1)[:, ::-1]          # descending in the device's order
    return u[:, k - 1] - u[:, kc] > tau * magnitude(x, w, b)


def stage1_error(x, w, b=None):
    """The largest error of an fp32 numpy evaluation of x.w + b against float64, relative to ``magnitude``."""
    x32, w32 = np.asarray(x, np.float32), np.asarray(w, np.float32)
    u32 = x32 @ w32.T
    if b is not None:
        u32 = u32 + np.asarray(b, np.float32)[None, :]
    return float((np.abs(u32.astype(np.float64) - logits64(x32, w32, b)) / magnitude(x, w, b)[:, None]).max())


def labels_for(n, C, seed, stray=True):
    """int64 [n]: labels in [0, C) with, when ``stray`` and n >= 4, one -1 and one C among them."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, n).astype(np.int64)
    if stray and n >= 4:
        y[1], y[n - 2] = -1, C
    return y
