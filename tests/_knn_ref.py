"""Float64 restatement of the k-nearest-neighbour probe (umlh.KNeighborsProbe / umlh_knn_search / umlh_knn_vote), numpy only.

What KNeighborsClassifier(n_neighbors=k) computes with its defaults (Euclidean metric, uniform weights), with this project's
tie rules written out: neighbours ordered by (squared distance ascending, train index ascending), the vote's count ties to
the smallest label value.  Squared distances are direct differences sum_k (q_k - t_k)^2 in float64, never |q|^2 + |t|^2 - 2 q.t.

SHARPNESS.  The device picks its candidates from an fp32 score, so a query whose k-th and (k+1)-th neighbours are closer than
that score can resolve may legitimately return either.  A query is sharp when
    d2_(k+1) - d2_(k)  >  TAU * (|q|^2 + max_t |t|^2)          (float64; n_train == k: there is no (k+1)-th, every query is sharp)
TAU is 8 x the largest relative error, against that same scale, that an fp32 numpy evaluation of the stage-1 score form
|t|^2 - 2 q.t reaches over all committed cases, rounded up to a power of two (the convention of the encoder tests).
tests/test_knn_cpu.py re-measures it: the largest error per case of tests/golden/knn_probe*.npz is 2^-22.7 .. 2^-22.5, and
8 x 2^-22.5 = 2^-19.5 rounds up to 2^-19.  At 2^-19 no query of any committed case is non-sharp.
"""
import numpy as np

TAU = 2.0 ** -19
CAP = 0.02                   # at most this fraction of a case's queries may be non-sharp

VARIANTS = ("tie_larger_index", "vote_larger_label", "inner_product", "no_tnorm", "self_exclusion")


def sqdist(q, t, chunk=64):
    """float64 [nq, nt]: sum_k (q_k - t_k)^2 from direct differences."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    out = np.empty((len(q), len(t)))
    for s in range(0, len(q), chunk):
        df = q[s:s + chunk, None, :] - t[None, :, :]
        out[s:s + chunk] = np.einsum("qtk,qtk->qt", df, df)
    return out


def _order(values, larger_index=False):
    """Row-wise order by (value asc, index asc) -- or index desc among equal values for the wrong variant."""
    n = values.shape[1]
    cols = np.broadcast_to(np.arange(n), values.shape)
    return np.lexsort((-cols if larger_index else cols, values), axis=1)


def kneighbors(q, t, k, variant=None):
    """(d2 float64 [nq, k], idx int64 [nq, k]).  ``variant``: one of VARIANTS, a deliberately wrong statement."""
    q64, t64 = np.asarray(q, np.float64), np.asarray(t, np.float64)
    d2 = sqdist(q64, t64)
    rank_by = d2
    if variant == "inner_product":
        rank_by = -(q64 @ t64.T)
    elif variant == "no_tnorm":
        rank_by = -2.0 * (q64 @ t64.T)
    elif variant == "self_exclusion":
        rank_by = d2.copy()
        m = min(rank_by.shape)
        rank_by[np.arange(m), np.arange(m)] = np.inf
    idx = _order(rank_by, larger_index=(variant == "tie_larger_index"))[:, :k]
    return np.take_along_axis(d2, idx, 1), idx


def vote(neigh_labels, larger_label=False):
    """(pred int64 [n], count int64 [n]) of label rows [n, k]: the most frequent value, ties to the smallest value."""
    lab = np.asarray(neigh_labels, np.int64)
    pred, cnt = np.empty(len(lab), np.int64), np.empty(len(lab), np.int64)
    for i, row in enumerate(lab):
        vals, counts = np.unique(row, return_counts=True)                    # vals ascending
        best = counts.max()
        winners = vals[counts == best]
        pred[i], cnt[i] = (winners[-1] if larger_label else winners[0]), best
    return pred, cnt


def predict(q, t, labels, k, variant=None):
    _, idx = kneighbors(q, t, k, variant)
    return vote(np.asarray(labels)[idx], larger_label=(variant == "vote_larger_label"))[0]


def scale(q, t):
    """float64 [nq]: |q|^2 + max_t |t|^2, the magnitude the stage-1 score's rounding is relative to."""
    q64, t64 = np.asarray(q, np.float64), np.asarray(t, np.float64)
    return (q64 * q64).sum(1) + (t64 * t64).sum(1).max()


def sharp(q, t, k, tau=TAU):
    """bool [nq]: the gap between the k-th and (k+1)-th squared distance exceeds tau * scale."""
    if len(t) == k:
        return np.ones(len(q), bool)
    d2 = np.sort(sqdist(q, t), axis=1)
    return d2[:, k] - d2[:, k - 1] > tau * scale(q, t)


def stage1_error(q, t):
    """The largest error of an fp32 numpy evaluation of |t|^2 - 2 q.t against float64, relative to ``scale``."""
    q32, t32 = np.asarray(q, np.float32), np.asarray(t, np.float32)
    s32 = (t32 * t32).sum(1, dtype=np.float32)[None, :] - np.float32(2) * (q32 @ t32.T)
    q64, t64 = q32.astype(np.float64), t32.astype(np.float64)
    s64 = (t64 * t64).sum(1)[None, :] - 2.0 * (q64 @ t64.T)
    return float((np.abs(s32.astype(np.float64) - s64) / scale(q, t)[:, None]).max())


def integer_case(n_train=300, n_query=64, d=6, classes=3, seed=11):
    """Features in -2..2: every product, sum and squared distance is exact in fp32, and ties are certain."""
    rng = np.random.default_rng(seed)
    t = rng.integers(-2, 3, (n_train, d)).astype(np.float32)
    q = rng.integers(-2, 3, (n_query, d)).astype(np.float32)
    return t, rng.integers(0, classes, n_train).astype(np.int32), q, rng.integers(0, classes, n_query).astype(np.int32)
