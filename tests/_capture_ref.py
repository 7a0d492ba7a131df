"""Host references for the embedding capture (umlh.seq_compact, umlh.paired_cosine, multibench.capture): numpy, float64
where arithmetic is involved, written as the reference writes them (MultiBench/train.py:302-345,464-499)."""
import copy

import numpy as np


def rows_of(lengths, t_len, drop_last=0):
    """Rows each sequence contributes: max(clamp(len, 0, t_len) - drop_last, 0)."""
    if lengths is None:
        return None
    return np.maximum(np.clip(np.asarray(lengths, dtype=np.int64), 0, t_len) - drop_last, 0)


def compact(z, lengths=None, drop_last=0):
    """The reference's nested loops (train.py:335-339,464-472): per sequence j the slice z[j, :rows_j, :], concatenated.
    The dtype of ``z`` is kept, so the fp32 result can be compared bit for bit."""
    z = np.asarray(z)
    B, T, d = z.shape
    n = rows_of(lengths, T, drop_last)
    parts = []
    for j in range(B):
        k = max(T - drop_last, 0) if n is None else int(n[j])
        parts.append(z[j, :k, :])
    return np.concatenate(parts, axis=0) if parts else np.zeros((0, d), z.dtype)


def cosine_rows(a, b, eps=1e-8):
    """F.cosine_similarity(a, b, dim=1, eps) in float64: each row divided by its own clamped norm, then the dot product."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na = np.maximum(np.sqrt((a * a).sum(axis=1, keepdims=True)), eps)
    nb = np.maximum(np.sqrt((b * b).sum(axis=1, keepdims=True)), eps)
    return ((a / na) * (b / nb)).sum(axis=1)


def cosine_mean(a, b, eps=1e-8):
    return float(cosine_rows(a, b, eps).mean())


def take_fixed_samples(loader_1, loader_2, modalities, n_samples=1000, batch_size=None):
    """The selection rule of train.py:302-331 for ds_name != 'mimic', restated: pair i of the zipped loader copies gives its
    first ``batch_size`` rows while (i + 1) * batch_size <= n_samples, else its first n_samples - i * batch_size rows, and
    the walk ends after the first pair with (i + 1) * batch_size >= n_samples.  -> ({'x1', 'x2', 'lx1', 'lx2': lists},
    {'x1_label', 'x2_label': lists of element 3})."""
    if batch_size is None:
        batch_size = loader_1.batch_size if hasattr(loader_1, "batch_size") else loader_1[0][0][modalities[0]].shape[0]
    kept = {k: [] for k in ("x1", "x2", "lx1", "lx2")}
    labels = {"x1_label": [], "x2_label": []}
    for i, pair in enumerate(zip(copy.deepcopy(loader_1), copy.deepcopy(loader_2))):
        head = slice(None, batch_size if (i + 1) * batch_size <= n_samples else n_samples - i * batch_size)
        for side, (batch, m) in enumerate(zip(pair, modalities), start=1):
            kept[f"x{side}"].append(batch[0][m].float()[head])
            kept[f"lx{side}"].append(batch[1][m][head])
            labels[f"x{side}_label"].append(batch[3][head])
        if (i + 1) * batch_size >= n_samples:
            break
    return kept, labels
