"""Reference module of the multinomial logistic probe (umlh_softmax_probe_*, umlh.probe.SoftmaxProbe): the float64 statement of
the objective and its gradient, the blob data of the test cases, a numpy restatement of the device algorithm in the device's
number formats (fp32 iterate, logits and residuals; every sum in double), and the derived bounds the GPU tests assert.

Objective (sklearn's lbfgs objective for three or more classes, written as a sum):
    f(W) = sum_i (logsumexp_c z_ic - z_{i,y_i}) + (1 / (2C)) sum_{c, j < d} W_cj^2,   z_ic = W_c . [x_i, 1]
A row whose label lies outside [0, K) contributes nothing.  With `stats` (mean | scale, 2d doubles) the features are
standardised as the kernels do it: (float)(((double)x - mean) * (1.0 / scale)).
"""
import hashlib

import numpy as np

LS_STEPS = [4.0, 2.0] + [2.0 ** -j for j in range(12)]      # trial step lengths; 4 and 2 only on a history-free iteration
ARMIJO = 1e-4
PAIR_TOL = 1e-12

# case id -> n, d, K, ldx, standardize (columns scaled over two decades), seed
CASES = {
    "n257_d5_k3": dict(n=257, d=5, K=3, ldx=5, standardize=False, seed=11),
    "n600_d33_k7_ld40": dict(n=600, d=33, K=7, ldx=40, standardize=False, seed=12),
    "n2048_d64_k130": dict(n=2048, d=64, K=130, ldx=64, standardize=False, seed=13),
    "n1600_d512_k100": dict(n=1600, d=512, K=100, ldx=512, standardize=False, seed=14),
    "n900_d20_k5_std": dict(n=900, d=20, K=5, ldx=20, standardize=True, seed=15),
}
C_REG = 1.0


def make_case(name):
    """(x fp32 [n, d], y int32 [n]): overlapping Gaussian blobs, balanced shuffled labels.  Deterministic in the case."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    n, d, K = c["n"], c["d"], c["K"]
    centers = rng.standard_normal((K, d)) * (2.0 / np.sqrt(d))
    y = np.arange(n) % K
    rng.shuffle(y)
    x = centers[y] + rng.standard_normal((n, d)) / np.sqrt(d) * 1.5
    if c["standardize"]:
        x = x * 10.0 ** np.linspace(-1.0, 1.0, d)[None, :] + np.linspace(-3.0, 3.0, d)[None, :]
    return np.ascontiguousarray(x, dtype=np.float32), y.astype(np.int32)


def checksum(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def column_stats(x):
    """StandardScaler statistics in float64: mean | population std (values below 10 eps replaced by 1)."""
    x = x.astype(np.float64)
    mu = x.mean(0)
    sd = np.sqrt(((x - mu) ** 2).mean(0))
    sd = np.where(sd < 10 * np.finfo(np.float64).eps, 1.0, sd)
    return np.concatenate([mu, sd])


def x_tilde(x, stats=None):
    """fp32 [n, d + 1]: the features as the kernels see them (standardised on load, rounded to fp32 once) and the 1 column."""
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    if stats is not None:
        x = ((x.astype(np.float64) - stats[:d]) * (1.0 / stats[d:])).astype(np.float32)
    return np.concatenate([x, np.ones((n, 1), np.float32)], axis=1)


def objective_grad(W, xt, y, C, want_grad=True, mean=False, penalise_intercept=False, label_shift=0, max_shift=True):
    """(f, g) in float64 at W [K, d + 1] on xt = x_tilde(...).  The keyword switches state WRONG variants (tests use them to show
    that the bounds discriminate): mean instead of sum, a penalised intercept, labels shifted by one, no max shift."""
    W = np.asarray(W, dtype=np.float64)
    K, D = W.shape
    d = D - 1
    xt = np.asarray(xt, dtype=np.float64)
    y = (np.asarray(y).astype(np.int64) + label_shift)
    if label_shift:
        y = y % K
    ok = (y >= 0) & (y < K)
    z = xt @ W.T
    with np.errstate(over="ignore", invalid="ignore"):
        zmax = z.max(1, keepdims=True) if max_shift else np.zeros((z.shape[0], 1))
        e = np.exp(z - zmax)
        se = e.sum(1, keepdims=True)
        lse = np.log(se) + zmax
        yy = np.where(ok, y, 0)
        loss = np.where(ok, lse[:, 0] - z[np.arange(len(y)), yy], 0.0)
        scale = 1.0 / max(int(ok.sum()), 1) if mean else 1.0
        pen = W if penalise_intercept else W[:, :d]
        f = scale * loss.sum() + 0.5 / C * (pen * pen).sum()
        if not want_grad:
            return f, None
        r = e / se
        r[np.arange(len(y)), yy] -= 1.0
        r[~ok] = 0.0
        g = scale * (r.T @ xt)
        g[:, :d] += W[:, :d] / C
        if penalise_intercept:
            g[:, d] += W[:, d] / C
    return f, g


def grad_allowance(W, xt, y, crit_max=2.0 ** -20):
    """E: what the fp32 GEMM criterion (tests/_gemm_ref.py: every entry within 2^-20 of the sum of its term magnitudes) allows the
    device gradient R^T X~ to deviate, as a bound on max|g|: max over entries of crit_max * sum_i |r_ic| |x~_ij|, plus one fp32
    rounding of the residuals themselves (2^-24 of the same sum)."""
    W = np.asarray(W, dtype=np.float64)
    xt = np.asarray(xt, dtype=np.float64)
    z = xt @ W.T
    e = np.exp(z - z.max(1, keepdims=True))
    r = e / e.sum(1, keepdims=True)
    y = np.asarray(y).astype(np.int64)
    ok = (y >= 0) & (y < W.shape[0])
    r[np.arange(len(y))[ok], y[ok]] -= 1.0
    r[~ok] = 0.0
    S = np.abs(r).T @ np.abs(xt)
    return float((crit_max + 2.0 ** -24) * S.max())


def objective_allowance(W, xt, y, f, crit_max=2.0 ** -20):
    """What the device objective may differ from the float64 one: 2^-40 |f| for its double sums, plus the logits' share: a logit
    off by dz_ic moves the loss of row i by at most sum_c (softmax_ic + [c = y_i]) |dz_ic|, and the fp32 GEMM criterion bounds
    |dz_ic| by crit_max * sum_j |x~_ij| |W_cj|."""
    W = np.asarray(W, dtype=np.float64)
    xt = np.asarray(xt, dtype=np.float64)
    z = xt @ W.T
    e = np.exp(z - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    y = np.asarray(y).astype(np.int64)
    ok = (y >= 0) & (y < W.shape[0])
    p[np.arange(len(y))[ok], y[ok]] += 1.0
    p[~ok] = 0.0
    return float(2.0 ** -40 * abs(f) + crit_max * (p * (np.abs(xt) @ np.abs(W).T)).sum())


def margins(W, xt):
    """(argmax, top-two margin) of the float64 logits."""
    z = np.asarray(xt, np.float64) @ np.asarray(W, np.float64).T
    top = np.argmax(z, axis=1)
    zs = np.sort(z, axis=1)
    return top, zs[:, -1] - zs[:, -2]


def pow2_ceil(v):
    return float(2.0 ** np.ceil(np.log2(v))) if v > 0 else 0.0


# ---------------------------------------------------------------------------------------------------------------------------- #
# the device algorithm in numpy, in the device's number formats
# ---------------------------------------------------------------------------------------------------------------------------- #
def _rows(zd, y, ok):
    """fp32 residuals and the double loss of double logits zd."""
    with np.errstate(over="ignore", invalid="ignore"):
        zmax = zd.max(1, keepdims=True)
        e = np.exp(zd - zmax)
        se = e.sum(1, keepdims=True)
        r = e / se
        yy = np.where(ok, y, 0)
        loss = np.where(ok, np.log(se[:, 0]) + zmax[:, 0] - zd[np.arange(len(y)), yy], 0.0).sum()
        r[np.arange(len(y)), yy] -= 1.0
        r[~ok] = 0.0
    return r.astype(np.float32), float(loss)


def _direction(cnt_order, g_idx, B, sumabs):
    """Two-loop recursion in coefficient space over the Gram matrix B: the coefficients of p in the basis."""
    nb = B.shape[0]
    q = np.zeros(nb)
    q[g_idx] = 1.0
    if not cnt_order:
        q[g_idx] = -1.0 / sumabs
        return q
    alphas = []
    for (si, yi) in reversed(cnt_order):                   # newest first
        rho = 1.0 / B[si, yi]
        a = rho * (B[si] @ q)
        q[yi] -= a
        alphas.append((a, rho))
    si, yi = cnt_order[-1]
    q *= B[si, yi] / B[yi, yi]
    for (si, yi), (a, rho) in zip(cnt_order, reversed(alphas)):      # oldest first
        b = rho * (B[yi] @ q)
        q[si] += a - b
    return -q


def fit_fp32(x, y, C=1.0, stats=None, max_iter=200, history=10, gtol=None, W0=None):
    """The launch train of umlh_softmax_probe_fit restated: returns dict(W fp32 [K, d+1], n_iter, converged, objective, max_grad,
    objectives, K).  y must be remapped to 0..K-1; K = max(y) + 1 unless W0 fixes it."""
    xt = x_tilde(x, stats)
    n, D = xt.shape
    d = D - 1
    y = np.asarray(y).astype(np.int64)
    K = int(y.max()) + 1 if W0 is None else W0.shape[0]
    ok = (y >= 0) & (y < K)
    gtol = 1e-4 * n if gtol is None else gtol
    inv_c = 1.0 / C
    W = np.zeros((K, D), np.float32) if W0 is None else np.array(W0, np.float32)
    h = history
    S = np.zeros((h, K, D), np.float32)
    Y = np.zeros((h, K, D), np.float32)
    nb = 2 * h + 1
    B = np.zeros((nb, nb))
    head, cnt = 0, 0
    gold = None
    objectives = np.full(max_iter + 1, np.nan)
    it, t, have_step, fresh, want_fresh = 0, 0.0, False, True, False
    zd = zp = None
    f = None
    rec = None
    shift = 0.0
    for k in range(max_iter + 1):
        if fresh:
            zparts = -(-D // 128)
            zc = (-(-D // zparts) + 3) // 4 * 4             # fp32 partial products over column chunks, added in double
            zd = sum((xt[:, k0:k0 + zc] @ W[:, k0:k0 + zc].T).astype(np.float64) for k0 in range(0, D, zc))
        elif have_step:
            zd = zd + t * zp.astype(np.float64)
        r, loss = _rows(zd, y, ok)
        gd = (r.T @ xt).astype(np.float64)
        gd[:, d] = r.astype(np.float64).sum(0)              # the intercepts' gradient: column sums of R in double,
        gd[:, d] -= gd[:, d].mean()                         # their mean over the classes (rounding of R) taken out
        gd[:, :d] += inv_c * W[:, :d].astype(np.float64)
        g = gd.astype(np.float32)
        mg = float(np.abs(gd).max()) if np.isfinite(gd).all() else float("nan")
        sumabs = float(np.abs(gd).sum())
        wpen = float((W[:, :d].astype(np.float64) ** 2).sum())
        if fresh:
            if k > 0:
                shift += loss + 0.5 * inv_c * wpen - f
            f = loss + 0.5 * inv_c * wpen
            if k == 0:
                objectives[0] = f
        if have_step:
            Y[head] = g - gold
        # Gram rows of the new vectors
        vecs = [S[i].ravel().astype(np.float64) for i in range(h)] + [Y[i].ravel().astype(np.float64) for i in range(h)] + [g.ravel().astype(np.float64)]
        rows = ([head, h + head] if have_step else []) + [2 * h]
        for ri in rows:
            for cj in range(nb):
                B[ri, cj] = B[cj, ri] = float(vecs[ri] @ vecs[cj])
        if mg != mg or f != f:
            rec = (0, f, mg)
            break
        if mg <= gtol:
            if fresh:
                rec = (1, f, mg)
                break
            want_fresh = True
        if k == max_iter:
            rec = (0, f, mg)
            break
        if have_step:
            sy, ss, yy_ = B[head, h + head], B[head, head], B[h + head, h + head]
            if sy > PAIR_TOL * np.sqrt(ss * yy_):
                head = (head + 1) % h
                cnt = min(cnt + 1, h)
            elif cnt == h:
                cnt = h - 1
        order = [((head - cnt + i) % h, h + (head - cnt + i) % h) for i in range(cnt)]
        c = _direction(order, 2 * h, B, sumabs)
        gtp = float(c @ B[2 * h])
        first = cnt == 0
        if not gtp < 0.0:
            cnt, first = 0, True
            c = np.zeros(nb)
            c[2 * h] = -1.0 / sumabs
            gtp = float(c @ B[2 * h])
        p = np.zeros(K * D)
        for j in range(nb):
            if c[j] != 0.0:
                p += c[j] * vecs[j]
        p = p.astype(np.float32).reshape(K, D)
        gold = g
        zp = xt @ p.T
        wp = float((W[:, :d].astype(np.float64) * p[:, :d]).sum())
        pp = float((p[:, :d].astype(np.float64) ** 2).sum())
        was_fresh = fresh
        t = 0.0
        for tj in LS_STEPS:
            if tj > 1.0 and not first:
                continue
            zt = zd + tj * zp.astype(np.float64)
            _, lt = _rows(zt, y, ok)
            ft = lt + 0.5 * inv_c * (wpen + 2.0 * tj * wp + tj * tj * pp)
            if ft <= f + ARMIJO * tj * gtp:
                t = tj
                break
        if t == 0.0:
            if was_fresh:
                rec = (2, f, mg)
                break
            have_step, fresh, want_fresh = False, True, False
            continue
        f = ft
        it += 1
        objectives[it] = f - shift
        Wn = (W.astype(np.float64) + t * p.astype(np.float64)).astype(np.float32)
        S[head] = Wn - W
        W = Wn
        have_step = True
        fresh = want_fresh or (k + 1 == max_iter)
        want_fresh = False
    return dict(W=W, n_iter=it, converged=rec[0], objective=rec[1], max_grad=rec[2], objectives=objectives, K=K)
