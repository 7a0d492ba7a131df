"""float64 numpy restatement of the reference's alignment metrics (vision_language/metrics.py): linear CKA with the biased
HSIC (:96-119, :252-255), compute_nearest_neighbors (:272-285, raw inner product, self excluded) and mutual_knn (:55-84),
with the project's tie rule: neighbours ordered by (score desc, index asc).  Large kNN runs in row blocks; no N x N array."""
import numpy as np

TAU_SCALE = 2.0 ** -20      # decidability margin: tau_i = 2^-20 * |x_i| * max_j |x_j|

# (n, d_a, d_b) at which a 32-column tile body can go wrong unseen by the recorded cases: different tile counts per view with one
# row left in the last 32-row block and d_a rounded up to 36; a one-column view against three tiles; fewer rows than one
# 8-row group (three of the four waves idle)
TILE_EDGES = [(97, 33, 31), (33, 1, 65), (5, 64, 32)]


def tile_edge_pair(n, da, db):
    """Two float32 views of one 4-dimensional latent plus noise, off the origin; seeded by the shape."""
    g = np.random.default_rng(10000 * n + 100 * da + db)
    z = g.standard_normal((n, 4))
    a = z @ g.standard_normal((4, da)) + 0.5 * g.standard_normal((n, da)) + 1.0
    b = z @ g.standard_normal((4, db)) + 0.5 * g.standard_normal((n, db)) - 2.0
    return a.astype(np.float32), b.astype(np.float32)


def cka64(a, b):
    """(cka, hsic_kl, hsic_kk, hsic_ll) in float64 from the column-centred features: trace(K H L H) = |Ac^T Bc|_F^2."""
    ac = np.asarray(a, np.float64)
    bc = np.asarray(b, np.float64)
    ac = ac - ac.mean(0)
    bc = bc - bc.mean(0)
    kl = float(np.square(ac.T @ bc).sum())
    kk = float(np.square(ac.T @ ac).sum())
    ll = float(np.square(bc.T @ bc).sum())
    return kl / (np.sqrt(kk * ll) + 1e-6), kl, kk, ll


def _sorted_rows(scores, idx):
    order = np.lexsort((idx, -scores), axis=-1)
    return np.take_along_axis(scores, order, -1), np.take_along_axis(idx, order, -1)


def knn64(x, topk, block=1024):
    """(knn int64 [N, topk], top scores float64 [N, topk + 1]) under the order (score desc, index asc), self excluded."""
    x64 = np.asarray(x, np.float64)
    n = x64.shape[0]
    m = min(n - 1, topk + 8)
    out_i = np.empty((n, topk), np.int64)
    out_s = np.empty((n, min(topk + 1, n - 1)), np.float64)
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        s = x64[r0:r1] @ x64.T
        rows = np.arange(r1 - r0)
        s[rows, r0 + rows] = -np.inf
        part = np.argpartition(-s, m - 1, axis=1)[:, :m] if m < n else np.argsort(-s, axis=1)[:, :m]
        cs, ci = _sorted_rows(np.take_along_axis(s, part, 1), part)
        # a tie across the candidate boundary: that row is ordered again in full
        outside = s.copy()
        np.put_along_axis(outside, part, -np.inf, 1)
        redo = np.nonzero(outside.max(1) >= cs[:, out_s.shape[1] - 1])[0]
        for r in redo:
            fs, fi = _sorted_rows(s[r][None, :], np.arange(n)[None, :])
            cs[r, :m], ci[r, :m] = fs[0, :m], fi[0, :m]
        out_i[r0:r1] = ci[:, :topk]
        out_s[r0:r1] = cs[:, :out_s.shape[1]]
    return out_i, out_s


def mutual64(knn_a, knn_b):
    """mean over rows of |knn_a(i) n knn_b(i)| / k, counts as integers, the mean in float64."""
    ka, kb = np.asarray(knn_a), np.asarray(knn_b)
    hits = (ka[:, :, None] == kb[:, None, :]).any(-1).sum(1)
    return float(hits.sum()) / (ka.shape[0] * ka.shape[1])


def tau(x):
    x64 = np.asarray(x, np.float64)
    nrm = np.sqrt(np.square(x64).sum(1))
    return TAU_SCALE * nrm * nrm.max()


def set_decidable(top_scores, t, topk):
    """rows whose k-th and (k+1)-th float64 scores are further apart than tau_i"""
    return (top_scores[:, topk - 1] - top_scores[:, topk]) > t


def list_decidable(top_scores, t, topk):
    """rows whose top k+1 float64 scores are pairwise further apart than tau_i"""
    gaps = top_scores[:, :topk] - top_scores[:, 1:topk + 1]
    return (gaps > t[:, None]).all(1)
