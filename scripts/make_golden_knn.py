#!/usr/bin/env python
"""Fixtures for the k-nearest-neighbour probe (umlh.KNeighborsProbe), recorded from scikit-learn.  Run on the build machine only
(needs scikit-learn; neither the tests nor the package import it).  Writes tests/golden/knn_probe.npz and
knn_probe.part<i>.npz (data only, allow_pickle=False, every file under 1 MiB).

Per case `<tag>::` the fp32 train / query matrices, int32 labels, and what KNeighborsClassifier(n_neighbors=k) -- constructed as
the reference constructs it (MultiBench/train.py:99-100), with k passed where a case is not the default 5 -- returned:
kneighbors (distances, indices), predict and score.  Data are Gaussian class blobs with OVERLAPPING classes: the separation of
the class means is searched per case so that sklearn's accuracy lies in 0.5 .. 0.8 and at least a quarter of the queries win
their vote by one vote or less (with separated blobs every variant of the code scores 1.0 and the vote is untested).  A seed
is kept only if the float64 (distance, index) order of tests/_knn_ref.py reproduces sklearn's lists and predictions on every
row and at most 2 % of its queries are non-sharp (tests/_knn_ref.py: sharp); otherwise the next seed is taken.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _knn_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

# tag, n_train, d, n_query, classes, k
CASES = [("a600x40_k5", 600, 40, 200, 2, 5),
         ("b1000x35_k5", 1000, 35, 256, 2, 5),
         ("c900x64_c10_k5", 900, 64, 200, 10, 5),
         ("d700x33_k1", 700, 33, 130, 3, 1),
         ("d700x33_k24", 700, 33, 130, 3, 24),
         ("e513x7_k8", 513, 7, 97, 2, 8)]
PARTS = [("knn_probe", ["a600x40_k5", "b1000x35_k5", "e513x7_k8"]),
         ("knn_probe.part1", ["c900x64_c10_k5", "d700x33_k1", "d700x33_k24"])]


def blobs(rng, n, d, classes, sep):
    means = sep * rng.standard_normal((classes, d))
    y = rng.integers(0, classes, n)
    return (means[y] + rng.standard_normal((n, d))).astype(np.float32), y.astype(np.int32)


def margin_one_or_less(neigh_labels):
    out = np.zeros(len(neigh_labels), bool)
    for i, row in enumerate(neigh_labels):
        c = np.sort(np.unique(row, return_counts=True)[1])[::-1]
        out[i] = (c[0] - (c[1] if len(c) > 1 else 0)) <= 1
    return out


def one(tag, nt, d, nq, classes, k, seed):
    from sklearn.neighbors import KNeighborsClassifier
    for sep in (0.4, 0.33, 0.27, 0.22, 0.18, 0.15, 0.12):
        rng = np.random.default_rng(seed)
        x, y = blobs(rng, nt + nq, d, classes, sep)
        xt, yt, xq, yq = x[:nt], y[:nt], x[nt:], y[nt:]
        clf = KNeighborsClassifier() if k == 5 else KNeighborsClassifier(n_neighbors=k)
        clf.fit(xt, yt)
        dist, idx = clf.kneighbors(xq)
        pred, score = clf.predict(xq), clf.score(xq, yq)
        close = margin_one_or_less(yt[idx]).mean()
        if not (0.5 <= score <= 0.8 and close >= 0.25):
            continue
        d2, ridx = R.kneighbors(xq, xt, k)
        if not (np.array_equal(ridx, idx) and np.array_equal(R.vote(yt[ridx])[0], pred)):
            print(f"  {tag} seed {seed} sep {sep}: the float64 order differs from sklearn's, next")
            continue
        blunt = int((~R.sharp(xq, xt, k)).sum())
        if blunt > R.CAP * nq:
            print(f"  {tag} seed {seed} sep {sep}: {blunt} non-sharp queries, next")
            continue
        print(f"  {tag}: seed {seed} sep {sep} score {score:.3f} one-vote wins {close:.2f} non-sharp {blunt} "
              f"stage-1 error 2^{np.log2(R.stage1_error(xq, xt)):.1f}")
        return {"train": xt, "train_labels": yt, "query": xq, "query_labels": yq, "k": np.int32(k), "dist": dist.astype(np.float64),
                "idx": idx.astype(np.int64), "pred": pred.astype(np.int64), "score": np.float64(score), "sep": np.float64(sep),
                "seed": np.int64(seed)}
    return None


def main():
    recs = {}
    for tag, nt, d, nq, classes, k in CASES:
        seed, rec = 1, None
        while rec is None:
            assert seed < 200, tag
            rec = one(tag, nt, d, nq, classes, k, seed)
            seed += 1
        recs[tag] = rec
    for name, tags in PARTS:
        arrays = {f"{t}::{k}": v for t in tags for k, v in recs[t].items()}
        if name == "knn_probe":
            arrays["cases"] = np.array([c[0] for c in CASES])
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(f"{path}: {size} bytes")
        assert size < (1 << 20), (path, size)


if __name__ == "__main__":
    main()
