"""float64 numpy restatement of the reference's remaining alignment metrics (vision_language/metrics.py): the unbiased HSIC
(:230-249) of the linear and the RBF kernel (:96-125), the biased RBF CKA, CKNNA (:180-227) and the neighbour-list
statistics cycle_knn (:39-51), lcs_knn (:88-92) and edit_distance_knn (:164-176).  Written from the formulas, dense where
the reference is dense; ``pair_sums64_blocked`` evaluates the kernel sums in row blocks for large N.  Neighbour lists come from
``_align_ref.knn64`` and so follow the project's tie rule (score descending, index ascending).

edit_distance_knn has no recorded reference value (the reference calls torchaudio's edit distance); ``levenshtein`` below,
the textbook unit-cost DP, is its yardstick."""
import numpy as np

import _align_ref as R


def normalize_rows(x):
    """Rows scaled to unit L2 norm in fp32, as torch.nn.functional.normalize(x, dim=-1) does (eps 1e-12): the reference's
    own demo setting for sigma = 1."""
    x = np.asarray(x, np.float32)
    nrm = np.sqrt(np.square(x).sum(1, keepdims=True, dtype=np.float32), dtype=np.float32)
    return (x / np.maximum(nrm, np.float32(1e-12))).astype(np.float32)


def hsic_unbiased64(K, L):
    """Song et al. eq. 5 as the reference writes it; the first term is sum K~ . L~^T (it matters for CKNNA's masked kernels)."""
    m = K.shape[0]
    Kt = np.array(K, np.float64)
    Lt = np.array(L, np.float64)
    np.fill_diagonal(Kt, 0.0)
    np.fill_diagonal(Lt, 0.0)
    v = (Kt * Lt.T).sum() + Kt.sum() * Lt.sum() / ((m - 1) * (m - 2)) - 2.0 * (Kt.sum(0) * Lt.sum(1)).sum() / (m - 2)
    return float(v / (m * (m - 3)))


def hsic_biased64(K, L):
    """trace(K H L H), H = I - 1/m, for symmetric K, L."""
    m = K.shape[0]
    K = np.asarray(K, np.float64)
    L = np.asarray(L, np.float64)
    return float((K * L).sum() - 2.0 / m * (K.sum(1) * L.sum(1)).sum() + K.sum() * L.sum() / (m * m))


def _ratio(kl, kk, ll):
    with np.errstate(invalid="ignore"):
        return float(kl / (np.sqrt(kk * ll) + 1e-6)), kl, kk, ll


def unbiased_cka64(a, b):
    """(cka, hsic_kl, hsic_kk, hsic_ll), linear kernel, unbiased HSIC.  The features are centred first: the unbiased HSIC of a
    linear kernel does not change under a translation, and the centred Gram matrices do not cancel."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    a = a - a.mean(0)
    b = b - b.mean(0)
    K, L = a @ a.T, b @ b.T
    return _ratio(hsic_unbiased64(K, L), hsic_unbiased64(K, K), hsic_unbiased64(L, L))


def sq_dists64(x, y):
    """|x_i - y_j|^2 in float64, from the differences of centred rows (no cancellation), clamped at 0."""
    d = np.square(x).sum(1)[:, None] + np.square(y).sum(1)[None, :] - 2.0 * (x @ y.T)
    return np.maximum(d, 0.0)


def rbf_kernel64(x, sigma):
    x = np.asarray(x, np.float64)
    x = x - x.mean(0)
    K = np.exp(-sq_dists64(x, x) / (2.0 * sigma * sigma))
    np.fill_diagonal(K, 1.0)
    return K


def rbf_cka64(a, b, sigma, unbiased):
    """(cka, hsic_kl, hsic_kk, hsic_ll) with K = exp(-|a_i - a_j|^2 / (2 sigma^2)), dense."""
    K, L = rbf_kernel64(a, sigma), rbf_kernel64(b, sigma)
    h = hsic_unbiased64 if unbiased else hsic_biased64
    return _ratio(h(K, L), h(K, K), h(L, L))


def pair_sums64_blocked(a, b, sigma=None, block=512):
    """(sum K.L, sum K.K, sum L.L, K1, L1) over i != j from row blocks of the two kernels, no N x N array: the RBF kernel of
    width sigma, or the linear kernel of the centred features when sigma is None."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    a = a - a.mean(0)
    b = b - b.mean(0)
    n = a.shape[0]
    pair = np.zeros(3)
    k1, l1 = np.zeros(n), np.zeros(n)
    for r0 in range(0, n, block):
        r1 = min(n, r0 + block)
        if sigma is None:
            K, L = a[r0:r1] @ a.T, b[r0:r1] @ b.T
        else:
            K = np.exp(-sq_dists64(a[r0:r1], a) / (2.0 * sigma * sigma))
            L = np.exp(-sq_dists64(b[r0:r1], b) / (2.0 * sigma * sigma))
        rows = np.arange(r1 - r0)
        K[rows, r0 + rows] = 0.0
        L[rows, r0 + rows] = 0.0
        pair += (K * L).sum(), (K * K).sum(), (L * L).sum()
        k1[r0:r1], l1[r0:r1] = K.sum(1), L.sum(1)
    return pair, k1, l1


def cka64_from_sums(sums, unbiased):
    """(cka, hsic_kl, hsic_kk, hsic_ll) from pair_sums64_blocked's sums; the biased form puts the unit diagonal of an RBF
    kernel back."""
    pair, k1, l1 = sums
    m = float(k1.shape[0])
    if not unbiased:
        pair, k1, l1 = pair + m, k1 + 1.0, l1 + 1.0

    def hsic(tr, r, s):
        if unbiased:
            return (tr + r.sum() * s.sum() / ((m - 1) * (m - 2)) - 2.0 * (r * s).sum() / (m - 2)) / (m * (m - 3))
        return tr - 2.0 / m * (r * s).sum() + r.sum() * s.sum() / (m * m)

    return _ratio(hsic(pair[0], k1, l1), hsic(pair[1], k1, k1), hsic(pair[2], l1, l1))


def rbf_cka64_blocked(a, b, sigma, unbiased, block=512):
    return cka64_from_sums(pair_sums64_blocked(a, b, sigma, block), unbiased)


def unbiased_cka64_blocked(a, b, block=512):
    return cka64_from_sums(pair_sums64_blocked(a, b, None, block), True)


def median_sigma(a, b):
    """The mean over the two views of the median pairwise distance (i < j), in float64."""
    out = []
    for x in (a, b):
        x = np.asarray(x, np.float64)
        x = x - x.mean(0)
        d = np.sqrt(sq_dists64(x, x))
        out.append(np.median(d[np.triu_indices(x.shape[0], 1)]))
    return float(np.mean(out))


def cknna64(a, b, topk):
    """(cknna, sim_kl, sim_kk, sim_ll): unbiased HSIC of the raw Gram matrices masked by the shared neighbour sets."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    n = a.shape[0]
    K, L = a @ a.T, b @ b.T
    ka, _ = R.knn64(a, topk)
    kb, _ = R.knn64(b, topk)
    rows = np.arange(n)[:, None]
    ma, mb = np.zeros((n, n)), np.zeros((n, n))
    ma[rows, ka] = 1.0
    mb[rows, kb] = 1.0

    def sim(X, Y, mx, my):
        mask = mx * my
        return hsic_unbiased64(mask * X, mask * Y)

    return _ratio(sim(K, L, ma, mb), sim(K, K, ma, ma), sim(L, L, mb, mb))


def lcs_length(x, y):
    """length of the longest common subsequence"""
    prev = [0] * (len(y) + 1)
    for xi in x:
        cur = [0]
        for j, yj in enumerate(y, 1):
            cur.append(prev[j - 1] + 1 if xi == yj else max(prev[j], cur[j - 1]))
        prev = cur
    return prev[-1]


def levenshtein(x, y):
    """insertions, deletions and substitutions at unit cost"""
    prev = list(range(len(y) + 1))
    for i, xi in enumerate(x, 1):
        cur = [i]
        for j, yj in enumerate(y, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (xi != yj)))
        prev = cur
    return prev[-1]


def list_rows(knn_a, knn_b):
    """int64 [N, 3] = {cycle hit, LCS length, Levenshtein distance} per row of two [N, k] neighbour lists."""
    ka, kb = np.asarray(knn_a).astype(np.int64), np.asarray(knn_b).astype(np.int64)
    n = ka.shape[0]
    out = np.zeros((n, 3), np.int64)
    out[:, 0] = (ka[kb] == np.arange(n)[:, None, None]).reshape(n, -1).any(1)
    la, lb = ka.tolist(), kb.tolist()
    for i in range(n):
        out[i, 1] = lcs_length(la[i], lb[i])
        out[i, 2] = levenshtein(la[i], lb[i])
    return out


def list_means(rows, topk):
    """(cycle_knn, lcs_knn, edit_distance_knn) from the per-row integers: integer sums, one division each."""
    n = rows.shape[0]
    s = rows.sum(0)
    return float(s[0]) / n, float(s[1]) / n, 1.0 - (float(s[2]) / n) / topk
