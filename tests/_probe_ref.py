"""float64 numpy restatement of the linear probes of the reference's MultiBench evaluate() (MultiBench/train.py:31-91,
93-240): masked mean pooling, StandardScaler statistics, the two binary logistic-regression objectives sklearn minimises
there (sum form, t = 2y - 1, x~ = [x, 1], C = 1), their optimum by a damped Newton iteration, decision values, and the
decidability margin the GPU tests use.  Nothing here runs on the GPU and nothing imports sklearn."""
import numpy as np

LBFGS, LIBLINEAR = 0, 1          # LogisticRegression(max_iter=200)  /  StandardScaler + LogisticRegression(solver='liblinear')


def masked_mean(z, lengths=None):
    """[B, T, Z] -> [B, Z]: sum_{t < min(len, T)} z / min(len, T) (train.py:120-125); None: the plain mean over T."""
    z = np.asarray(z, np.float64)
    B, T, _ = z.shape
    L = np.full(B, T) if lengths is None else np.clip(np.asarray(lengths).astype(np.int64), 0, T)
    mask = (np.arange(T)[None, :] < L[:, None]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (z * mask[:, :, None]).sum(1) / L[:, None].astype(np.float64)


def masked_mean_bound(z, lengths=None):
    """The fp32 chain bound of the GPU test: T * 2^-24 * sum_t |z| / len, element-wise."""
    return z.shape[1] * 2.0 ** -24 * masked_mean(np.abs(np.asarray(z, np.float64)), lengths)


def column_stats(x):
    """StandardScaler().fit(x): mean and population std (ddof = 0), std < 10 eps -> 1 (sklearn's _handle_zeros_in_scale)."""
    x = np.asarray(x, np.float64)
    mean = x.mean(0)
    sd = np.sqrt(((x - mean) ** 2).mean(0))
    sd[sd < 10 * np.finfo(np.float64).eps] = 1.0
    return mean, sd


def standardise(x, stats):
    x = np.asarray(x, np.float64)
    return x if stats is None else (x - stats[0]) / stats[1]


def _aug(x):
    return np.concatenate([x, np.ones((x.shape[0], 1))], axis=1)


def objective(w, xa, y, kind, C=1.0):
    """sum_i log(1 + exp(-t_i w.x~_i)) + R(w) / (2C); R = |w|^2 without the intercept (LBFGS) or with it (LIBLINEAR)."""
    m = -(2.0 * y - 1.0) * (xa @ w)
    reg = w @ w if kind == LIBLINEAR else w[:-1] @ w[:-1]
    return np.sum(np.maximum(m, 0.0) + np.log1p(np.exp(-np.abs(m)))) + 0.5 * reg / C


def gradient(w, xa, y, kind, C=1.0):
    p = 1.0 / (1.0 + np.exp(-(xa @ w)))
    r = np.full(w.shape, 1.0 / C)
    if kind != LIBLINEAR:
        r[-1] = 0.0
    return xa.T @ (p - y) + r * w, p, r


def fit(x, y, kind, C=1.0, stats=None, tol=1e-10, max_iter=200):
    """The optimum w* ([d + 1], intercept last) of the `kind` objective on (standardised) x by a damped Newton iteration,
    run until max|gradient| <= tol.  Returns (w*, iterations, max|gradient|)."""
    xa = _aug(standardise(x, stats))
    y = np.asarray(y, np.float64)
    w = np.zeros(xa.shape[1])
    f = objective(w, xa, y, kind, C)
    for it in range(max_iter):
        g, p, r = gradient(w, xa, y, kind, C)
        if np.abs(g).max() <= tol:
            return w, it, np.abs(g).max()
        H = (xa * (p * (1 - p))[:, None]).T @ xa + np.diag(r)
        step = np.linalg.solve(H + 1e-300 * np.eye(len(w)), -g)
        a = 1.0
        while a > 1e-6:
            fn = objective(w + a * step, xa, y, kind, C)
            if fn <= f + 1e-4 * a * (g @ step):
                break
            a *= 0.5
        if a <= 1e-6:            # no representable decrease: the float64 floor of the objective
            return w, it, np.abs(g).max()
        w, f = w + a * step, fn
    g = gradient(w, xa, y, kind, C)[0]
    return w, max_iter, np.abs(g).max()


def decision(w, x, stats=None):
    return _aug(standardise(x, stats)) @ np.asarray(w, np.float64)


def score(w, x, y, stats=None):
    return float(np.mean((decision(w, x, stats) > 0).astype(np.int64) == np.asarray(y)))


def decidable(w_star, x, stats=None, w_other=None):
    """Boolean [N]: |dec64_i| > |w_other - w*|_2 |x~_i|_2 + (d + 2) 2^-24 sum_j |w*_j x~_ij| -- the coefficient error (0 when
    w_other is None) plus the fp32 dot-product bound.  On these samples a prediction from w_other in fp32 arithmetic must
    equal the optimum's."""
    xa = _aug(standardise(x, stats))
    w_star = np.asarray(w_star, np.float64)
    d = xa.shape[1] - 1
    margin = (d + 2) * 2.0 ** -24 * (np.abs(xa) @ np.abs(w_star))
    if w_other is not None:
        margin = margin + np.linalg.norm(np.asarray(w_other, np.float64) - w_star) * np.linalg.norm(xa, axis=1)
    return np.abs(xa @ w_star) > margin


def mosi_label(y):
    y = np.asarray(y)
    return (y >= 0).astype(np.int64)


def sarcasm_label(y):
    y = np.asarray(y)
    r = y.copy()
    r[y == -1] = 0
    return r
