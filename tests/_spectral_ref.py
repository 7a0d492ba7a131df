"""float64 restatement of the reference's effective rank (MultiBench/utilis.py:27-36) and of the row predicate of
MultiBench/train.py:380-389, for the tests of umlh.spectral and for scripts/make_golden_spectral.py."""
import numpy as np


def svdvals64(a):
    """Singular values of a [n, d] or [batch, n, d] array in float64, descending: min(n, d) of them."""
    return np.linalg.svd(np.asarray(a, np.float64), compute_uv=False)


def erank_of(sv, eps=1e-6):
    """exp(-sum p log(p + eps)), p = sv / sum sv, over the last axis (empty: 1; all zero: NaN)."""
    sv = np.asarray(sv, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = sv / sv.sum(axis=-1, keepdims=True)
        return np.exp(-(p * np.log(p + eps)).sum(axis=-1))


def erank64(a, eps=1e-6):
    return erank_of(svdvals64(a), eps)


def valid_rows(z, lengths=None, drop_last=0):
    """The rows z[b, t] with t < clamp(lengths[b], 0, T) - drop_last of a [B, T, d] array, b-major: [rows, d]."""
    z = np.asarray(z)
    B, T, d = z.shape
    ln = np.full(B, T, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, T)
    keep = np.arange(T)[None, :] < (ln - drop_last)[:, None]
    return z[keep]


def erank_seq64(z, lengths=None, drop_last=0, eps=1e-6):
    """(effective rank, row count) of the compacted matrix; zero rows: (1.0, 0)."""
    rows = valid_rows(z, lengths, drop_last)
    if rows.shape[0] == 0:
        return 1.0, 0
    return float(erank64(rows, eps)), rows.shape[0]


def errors(sv, erank, sv64, erank64_):
    """(max |sv - sv64| / sigma_max, |erank - erank64| / erank64) of one matrix."""
    sv, sv64 = np.asarray(sv, np.float64), np.asarray(sv64, np.float64)
    smax = sv64.max() if sv64.size else 1.0
    return float(np.abs(sv - sv64).max() / smax), float(abs(float(erank) - float(erank64_)) / float(erank64_))
