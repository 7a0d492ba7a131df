"""Reference statements for the class index and class statistics of the feature capture  --  TEST INFRASTRUCTURE ONLY.

``class_index`` and ``class_stats`` state the two contracts of include/umlh.h (umlh_class_index, umlh_class_stats) in numpy
float64; ``reference_fp32`` restates vision_language/finetune.py:222-231 with the reference's own torch fp32 ops (the per-class
loop with ``nonzero``, ``mean``, ``norm`` and ``.item()``, then ``np.mean``).

FP32_FORM_BOUND is the relative bound on train/inclass_distance between any correct evaluation and the reference's logged
fp32 value: the fp32 form's own measured error against float64 on run A of tests/golden/feature_capture.npz (the largest
relative difference over the six steps between ``reference_fp32`` -- which reproduces the logged values bit for bit -- and
``class_stats`` in float64 on the saved features: 2.11e-8), times 8 (1.69e-7), rounded up to a power of two: 2^-22 = 2.38e-7.

``WRONG`` holds three deliberately wrong variants of ``class_stats`` (distance to the mean of ALL rows; mean of SQUARED
distances; empty classes skipped instead of NaN): tests/test_featcap_cpu.py shows that each breaks a bound of the GPU tests by
at least 8x on those tests' own cases.
"""
import numpy as np

FP32_FORM_BOUND = 2.0 ** -22


def class_index(labels, n_class):
    """(order, offsets): numpy's stable argsort restricted to the labels inside [0, n_class)."""
    labels = np.asarray(labels, dtype=np.int64)
    keep = np.flatnonzero((labels >= 0) & (labels < n_class))
    order = keep[np.argsort(labels[keep], kind="stable")]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(labels[keep], minlength=n_class))]).astype(np.int64)
    return order.astype(np.int32), offsets


def class_rows(order, offsets, n_class, n):
    """Per class the rows the kernel reads: offsets through its running maximum clamped to [0, n], entries outside [0, n)
    dropped."""
    mono = np.maximum.accumulate(np.clip(np.asarray(offsets, dtype=np.int64), 0, n))
    order = np.asarray(order, dtype=np.int64)
    out = []
    for c in range(n_class):
        r = order[mono[c]:mono[c + 1]]
        out.append(r[(r >= 0) & (r < n)])
    return out


def class_means(feats, rows):
    """float64 [n_class, d] class means; NaN rows for empty classes."""
    x = np.asarray(feats, dtype=np.float64)
    m = np.full((len(rows), x.shape[1]), np.nan)
    with np.errstate(all="ignore"):
        for c, r in enumerate(rows):
            if r.size:
                m[c] = x[r].sum(axis=0) / r.size
    return m


def class_dists(feats, rows, means):
    """float64 [n_class]: mean over a class's rows of |x_i - means[c]|_2 with explicit differences; NaN for empty classes."""
    x = np.asarray(feats, dtype=np.float64)
    means = np.asarray(means, dtype=np.float64)
    d = np.full(len(rows), np.nan)
    with np.errstate(all="ignore"):
        for c, r in enumerate(rows):
            if r.size:
                d[c] = np.sqrt(((x[r] - means[c]) ** 2).sum(axis=1)).sum() / r.size
    return d


def out2(dist, rows):
    with np.errstate(all="ignore"):
        return np.asarray([np.sum(dist) / len(dist), float(sum(r.size == 0 for r in rows))])


def class_stats(feats, order, offsets, n_class, means32=None):
    """(means float64, dist float64 against ``means32`` -- default: the float64 means rounded to fp32 --, out2, rows)."""
    rows = class_rows(order, offsets, n_class, np.asarray(feats).shape[0])
    m64 = class_means(feats, rows)
    m32 = m64.astype(np.float32) if means32 is None else np.asarray(means32)
    dist = class_dists(feats, rows, m32)
    return m64, dist, out2(dist, rows), rows


def reference_fp32(img_features, image_samples_labels, n_class):
    """finetune.py:222-231 as written: (np.mean of the per-class ``.item()`` values, those values, the class means)."""
    import torch
    img_features = torch.as_tensor(img_features, dtype=torch.float32)
    image_samples_labels = torch.as_tensor(image_samples_labels)
    img_features_class_mean, inclass_distances = [], []
    for label in range(n_class):
        indices = (image_samples_labels == label).nonzero(as_tuple=True)[0]
        img_features_mean = img_features[indices].mean(dim=0)
        inclass_distances.append(torch.norm(img_features[indices] - img_features_mean.unsqueeze(0), dim=1).mean().item())
        img_features_class_mean.append(img_features_mean.unsqueeze(0))
    return np.mean(inclass_distances), np.asarray(inclass_distances), torch.cat(img_features_class_mean, dim=0).numpy()


# ---- deliberately wrong variants: (dist, out2) from the same arguments ----
def _wrong_global_mean(feats, rows):
    x = np.asarray(feats, dtype=np.float64)
    every = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    g = x[every].mean(axis=0) if every.size else np.full(x.shape[1], np.nan)
    dist = class_dists(feats, rows, np.tile(g, (len(rows), 1)))
    return dist, out2(dist, rows)


def _wrong_mean_of_squares(feats, rows):
    x = np.asarray(feats, dtype=np.float64)
    m = class_means(feats, rows).astype(np.float32).astype(np.float64)
    dist = np.asarray([((x[r] - m[c]) ** 2).sum(axis=1).mean() if r.size else np.nan for c, r in enumerate(rows)])
    return dist, out2(dist, rows)


def _wrong_skip_empty(feats, rows):
    dist = class_dists(feats, rows, class_means(feats, rows).astype(np.float32))
    kept = dist[[r.size > 0 for r in rows]]
    return dist, np.asarray([kept.mean() if kept.size else np.nan, float(sum(r.size == 0 for r in rows))])


WRONG = {"distance to the mean of all rows": _wrong_global_mean, "mean of squared distances": _wrong_mean_of_squares,
         "empty classes skipped": _wrong_skip_empty}


# ---- the bounds of the GPU tests ----
def means_bound(m64, feats, rows):
    """|means - m64| <= 2^-24 |m64| + 2^-40 mean_i |x_ij|: one fp32 rounding of an fp64 sum of at most 2^13 terms."""
    x = np.abs(np.asarray(feats, dtype=np.float64))
    mean_abs = np.stack([x[r].mean(axis=0) if r.size else np.zeros(x.shape[1]) for r in rows])
    return 2.0 ** -24 * np.abs(m64) + 2.0 ** -40 * mean_abs


def dist_rel_bound(d, rows):
    """(d + |R_c| + 4) 2^-53 per class: sums of non-negative terms, so the bound follows from the term count."""
    return np.asarray([(d + r.size + 4) * 2.0 ** -53 for r in rows])


def broken(got, want, bound_rel, factor=8.0):
    """True where ``got`` misses ``want`` by at least ``factor`` x the relative bound (a NaN on one side only counts)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    one_nan = np.isnan(got) != np.isnan(want)
    with np.errstate(all="ignore"):
        off = np.abs(got - want) >= factor * bound_rel * np.abs(want)
    return one_nan | (off & ~np.isnan(got) & ~np.isnan(want) & (np.abs(got - want) > 0))


# ---- cases shared by the CPU and GPU tests: name -> (feats fp32 [n, d], labels int64 [n], n_class) ----
def stats_cases():
    rng = np.random.default_rng(20261019)
    cases = {}
    for d in (1, 63, 64, 65, 257):
        n, c = 97, 7
        cases[f"d{d}"] = (rng.standard_normal((n, d)).astype(np.float32) + 0.5, rng.integers(0, c, n), c)
    y = rng.integers(0, 5, 40)
    y[y == 3] = 0
    y[7] = 3                                                    # class 3: one row
    cases["one_row_class"] = (rng.standard_normal((40, 33)).astype(np.float32), y, 5)
    y = rng.integers(0, 6, 50)
    y[y == 2] = 4                                               # class 2: empty
    cases["empty_class"] = (rng.standard_normal((50, 20)).astype(np.float32), y, 6)
    cases["one_class_5000_rows"] = (rng.standard_normal((5000, 24)).astype(np.float32) + 1.0, np.zeros(5000, dtype=np.int64), 1)
    cases["1000x16_d32"] = (rng.standard_normal((16000, 32)).astype(np.float32), rng.permutation(np.repeat(np.arange(1000), 16)), 1000)
    return {k: (x, np.asarray(y, dtype=np.int64), c) for k, (x, y, c) in cases.items()}
