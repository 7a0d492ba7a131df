"""float64 restatement of the reference's SVCCA (MultiBench/metrics.py:129-160) in closed form, for the tests of
umlh.align.svcca / umlh.spectral.principal_subspace and for scripts/make_golden_svcca.py.

The reference standardises the columns, takes the top-q left singular vectors U_a, U_b of the two views (randomised SVD) and
fits scikit-learn's CCA on them.  U_a and U_b are centred and orthonormal and CCA is invariant to invertible maps of either
basis, so the canonical correlations are the singular values of U_a^T U_b and the reference's value is their mean."""
import numpy as np


def standardise64(x):
    """(x - mean) / (unbiased std + 1e-8) per column, in float64 (metrics.py:132-135)."""
    x = np.asarray(x, np.float64)
    c = x - x.mean(axis=0)
    return c / (c.std(axis=0, ddof=1) + 1e-8)


def rho64(a, b, q):
    """The q canonical correlations of the top-q left singular subspaces of the standardised views, descending, in [0, 1]."""
    ua = np.linalg.svd(standardise64(a), full_matrices=False)[0][:, :q]
    ub = np.linalg.svd(standardise64(b), full_matrices=False)[0][:, :q]
    return np.clip(np.linalg.svd(ua.T @ ub, compute_uv=False), 0.0, 1.0)


def svcca64(a, b, q=10):
    return float(rho64(a, b, q).mean())


def gram64(a, standardize):
    """The d x d Gram of the (standardised) columns in float64."""
    x = standardise64(a) if standardize else np.asarray(a, np.float64)
    return x.T @ x


def top_eigh(g, q):
    """(evals[q] descending, evecs[d, q]) of a symmetric matrix by numpy.linalg.eigh, each vector's largest-magnitude component
    positive (the first one on ties); and all eigenvalues, descending."""
    lam, vec = np.linalg.eigh(g)
    lam, vec = lam[::-1], vec[:, ::-1]
    v = vec[:, :q].copy()
    for k in range(q):
        if v[np.argmax(np.abs(v[:, k])), k] < 0:
            v[:, k] = -v[:, k]
    return lam[:q].copy(), v, lam


def eig_ratios(g, lam, v):
    """(max |G V - V L| / (d eps lam_1), max |V^T V - I| / (d eps)) with eps = 2^-53 and lam_1 the largest eigenvalue given."""
    d, eps = g.shape[0], 2.0 ** -53
    res = np.abs(g @ v - v * lam[None, :]).max() / (d * eps * lam[0])
    orth = np.abs(v.T @ v - np.eye(v.shape[1])).max() / (d * eps)
    return float(res), float(orth)


def matrix_512():
    """600 x 512: ten planted directions (strengths 30 -> 12 over unit noise), column scales over two decades."""
    g = np.random.default_rng(512)
    lat = np.linalg.qr(g.standard_normal((600, 10)))[0] * np.sqrt(600)
    rows = np.linalg.qr(g.standard_normal((512, 10)))[0]
    a = (lat * np.linspace(30.0, 12.0, 10)) @ rows.T + g.standard_normal((600, 512))
    return (a * np.logspace(-1, 1, 512)[g.permutation(512)]).astype(np.float32)


def quantised_pair():
    """A planted pair on a 2^-8 grid with |x| < 64, so that small affine maps of its columns are exact in fp32."""
    g = np.random.default_rng(77)
    lat = np.linalg.qr(g.standard_normal((300, 9)))[0] * np.sqrt(300)
    out = []
    for d, cols in ((24, slice(0, 6)), (30, slice(3, 9))):
        rows = np.linalg.qr(g.standard_normal((d, 6)))[0]
        x = (lat[:, cols] * np.linspace(9.0, 5.0, 6)) @ rows.T + 0.3 * g.standard_normal((300, d))
        x = np.round(np.clip(x, -63, 63) * 256) / 256
        out.append(x.astype(np.float32))
    return out


def invariance_maps(a, b):
    """For the pair of quantised_pair: a row permutation, and float64 copies of a and b under per-column affine maps with
    positive scales and offsets on the grid: every mapped value is a multiple of 2^-9 below 2^9, exact in fp32."""
    g = np.random.default_rng(3)
    perm = g.permutation(a.shape[0])
    sa, sb = g.choice([0.5, 1.0, 2.0, 3.0, 4.0], a.shape[1]), g.choice([0.5, 1.0, 2.0, 3.0, 4.0], b.shape[1])
    ta, tb = g.integers(-25600, 25600, a.shape[1]) / 256.0, g.integers(-25600, 25600, b.shape[1]) / 256.0
    return perm, a.astype(np.float64) * sa + ta, b.astype(np.float64) * sb + tb


# ---- planted cases: scripts/make_golden_svcca.py records them, tests/test_svcca_gpu.py generates one more ----
GAIN = 8.0


def planted(g, latent, d):
    """latent[n, q] (orthogonal columns of norm sqrt(n)) -> n x d: strengths GAIN * (3 -> 1.5) along q orthonormal row
    directions, plus noise of unit spectral scale (its largest singular value is about sqrt(n), like one latent direction of
    strength 1)."""
    n, q = latent.shape
    rows = np.linalg.qr(g.standard_normal((d, q)))[0]
    if q == 1:                         # one direction: random signs, so that no column is left to the noise alone (which the
        rows = np.sign(rows) / np.sqrt(d)   # standardisation would scale up until sigma_2 / sigma_1 passes 0.2)
    noise = g.standard_normal((n, d)) / (1.0 + np.sqrt(d / n))
    return (latent * (GAIN * np.linspace(3.0, 1.5, q))) @ rows.T + noise


def gen_case(name, n, d_a, d_b, q, shared):
    g = np.random.default_rng(sum(map(ord, name)))
    lat = np.linalg.qr(g.standard_normal((n, 2 * q - shared)))[0] * np.sqrt(n)
    la = lat[:, :q]
    lb = np.concatenate([lat[:, :shared], lat[:, q:]], axis=1)
    a = planted(g, la, d_a)
    if name == "same":                 # B = A W, W a column permutation times a positive diagonal: the same subspace, rho = 1
        a32 = a.astype(np.float32)
        return a32, (a32.astype(np.float64)[:, g.permutation(d_a)] * g.uniform(0.5, 2.0, d_a)).astype(np.float32)
    b = planted(g, lb, d_b)
    if name == "offset":               # means up to 50 sigma, scales over 10^3, one exactly constant column per view
        for x in (a, b):
            scale = np.logspace(-1.5, 1.5, x.shape[1])[g.permutation(x.shape[1])]
            x *= scale
            x += g.uniform(-50.0, 50.0, x.shape[1]) * x.std(axis=0)
        a[:, 17] = 3.25
        b[:, 40] = -0.4375
    return a.astype(np.float32), b.astype(np.float32)
