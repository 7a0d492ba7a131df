"""Device time of the k-nearest-neighbour probe (umlh.KNeighborsProbe: search + vote), next to the torch-op form on the same GPU
(cdist + topk + label mode, chunked over the queries where the full distance matrix would not fit) and to scikit-learn on the
CPU when it imports on this machine.

    python scripts/bench_knn.py [--reps R] [--out DIR] [--no-sklearn] [--no-torch] [--skip-table]

Writes DIR/knn_bench.txt (one JSON line per size: median, min and max over the repeats) and DIR/knn_accuracy.txt (per recorded
case of tests/golden/knn_probe*.npz the worst relative dist error against float64 and the non-sharp count, tests/_knn_ref.py).
Sizes: the MOSEI probes (train 16 265 rows, queries 1 869 and 4 643, d 40 / 80 / 600), the raw-feature size d 335, a feature
table (16 000 x 1024 train rows, 50 000 queries, 1000 classes), all k = 5; and one whole multibench.train.evaluate at the MOSEI
row counts with the default classifier and with ('knn',).  Times are CUDA-event times around the enqueue of search + vote."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import umlh  # noqa: E402
import _knn_ref as R  # noqa: E402

DEV = "cuda:0"
TORCH_CHUNK_BYTES = 1 << 30          # distance-matrix bytes per chunk of the torch-op form


def timed(fn, reps, warm=1):
    """(median, min, max) microseconds of CUDA-event time over ``reps`` calls."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def blobs(nt, nq, d, classes, seed):
    rng = np.random.default_rng(seed)
    means = 0.3 * rng.standard_normal((classes, d)).astype(np.float32)
    y = rng.integers(0, classes, nt + nq)
    x = means[y] + rng.standard_normal((nt + nq, d), dtype=np.float32)
    return x[:nt], y[:nt].astype(np.int32), x[nt:], y[nt:].astype(np.int32)


def torch_ops(xt, yt, xq, yq, k):
    """The same prediction from torch ops: the n_query x n_train distance matrix in chunks, topk, the mode of the labels."""
    rows = max(1, min(len(xq), TORCH_CHUNK_BYTES // (4 * len(xt))))
    correct = torch.zeros((), dtype=torch.int64, device=xq.device)
    for s in range(0, len(xq), rows):
        idx = torch.cdist(xq[s:s + rows], xt).topk(k, dim=1, largest=False).indices
        pred = torch.mode(yt[idx].sort(dim=1).values, dim=1).values
        correct += (pred == yq[s:s + rows]).sum()
    return correct


def bench_size(name, nt, nq, d, classes, k, reps, use_torch, use_sklearn):
    xt, yt, xq, yq = blobs(nt, nq, d, classes, seed=nt + nq + d)
    xtd, ytd, xqd, yqd = (torch.from_numpy(a).to(DEV) for a in (xt, yt, xq, yq))
    pr = umlh.KNeighborsProbe(k).fit(xtd, ytd)
    med, lo, hi = timed(lambda: pr.correct(xqd, yqd), reps)
    out = {"size": name, "n_train": nt, "n_query": nq, "d": d, "classes": classes, "k": k, "hip_us": med, "hip_us_min": lo,
           "hip_us_max": hi, "hip_score": int(pr.correct(xqd, yqd)) / nq}
    if use_torch:
        try:
            med, lo, hi = timed(lambda: torch_ops(xtd, ytd.long(), xqd, yqd.long(), k), reps)
            out.update({"torch_ops_us": med, "torch_ops_us_min": lo, "torch_ops_us_max": hi,
                        "torch_ops_score": int(torch_ops(xtd, ytd.long(), xqd, yqd.long(), k)) / nq})
        except Exception as e:                                                    # the baseline is optional
            out["torch_ops_error"] = repr(e)[:200]
    if use_sklearn:
        try:
            from sklearn.neighbors import KNeighborsClassifier
            clf = KNeighborsClassifier(n_neighbors=k).fit(xt, yt)
            t0 = time.perf_counter()
            out["sklearn_cpu_score"] = float(clf.score(xq, yq))
            out["sklearn_cpu_s_this_machine"] = time.perf_counter() - t0
        except ImportError:
            pass
    return out


def bench_evaluate(reps):
    from multibench.models import Linear, Transformer, UML
    from multibench.train import evaluate
    z, dx, dy, T, bs = 40, 35, 300, 50, 32
    torch.manual_seed(0)
    m = UML(Linear(dx, z), Linear(dy, z), Transformer(z, z, nhead=5, num_layers=5, conv1d=True, out_last=False, pos_embd=True,
                                                       pos_learnable=False, max_len=128),
            [Linear(z, dx), Linear(z, dy)], modality="xy").to(DEV)
    rng = np.random.default_rng(1)
    cfg = {"freq": 100}
    for t, n in (("train", 16265), ("val", 1869), ("test", 4643)):
        x = torch.from_numpy(rng.standard_normal((n, T, dx)).astype(np.float32))
        y = torch.from_numpy(rng.standard_normal((n, T, dy)).astype(np.float32))
        lx = torch.from_numpy(rng.integers(5, T + 1, n))
        lab = torch.from_numpy((x[:, :5].mean((1, 2)) + 0.05 * rng.standard_normal(n)).numpy().astype(np.float32))
        cfg[t] = [([x[s:s + bs], None, y[s:s + bs]], [lx[s:s + bs], None, lx[s:s + bs]], None, lab[s:s + bs].reshape(-1, 1))
                  for s in range(0, n, bs)]

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}
    return {"shape": "MOSEI rows: 16265/1869/4643 sequences, T 50, batch 32, z 40, dx 35, dy 300",
            "evaluate_default_ms_wall": wall(lambda: evaluate(m, cfg, "mosei", device=DEV)),
            "evaluate_knn_ms_wall": wall(lambda: evaluate(m, cfg, "mosei", device=DEV, classifier_types=("knn",)))}


def accuracy(path):
    from conftest import load_golden
    g = load_golden("knn_probe")
    with open(path, "w") as f:
        f.write("# per recorded case: worst |dist_gpu - sqrt(d2_float64)| / sqrt(d2_float64), queries whose list differs from sklearn's, "
                f"non-sharp queries at tau = 2^{int(np.log2(R.TAU))} (tests/_knn_ref.py)\n")
        for tag in (str(t) for t in g["cases"]):
            c = {k.split("::", 1)[1]: v for k, v in g.items() if k.startswith(tag + "::")}
            k, t, q = int(c["k"]), c["train"], c["query"]
            pr = umlh.KNeighborsProbe(k).fit(torch.from_numpy(t).to(DEV), torch.from_numpy(c["train_labels"]).to(DEV))
            dist, idx = (a.cpu().numpy() for a in pr.kneighbors(torch.from_numpy(q).to(DEV)))
            d = np.sqrt(np.take_along_axis(R.sqdist(q, t), idx, 1))
            line = json.dumps({"case": tag, "n_train": len(t), "n_query": len(q), "d": int(t.shape[1]), "k": k,
                               "worst_dist_rel_error": float((np.abs(dist - d) / d).max()),
                               "lists_differing_from_sklearn": int((idx != c["idx"]).any(1).sum()),
                               "non_sharp": int((~R.sharp(q, t, k)).sum()),
                               "score": pr.score(torch.from_numpy(q).to(DEV), torch.from_numpy(c["query_labels"]).to(DEV)),
                               "sklearn_score": float(c["score"])})
            print(line)
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--skip-table", action="store_true", help="leave the 16 000 x 1024 / 50 000-query size out")
    ap.add_argument("--skip-evaluate", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn.py needs a GPU: a CPU run says nothing about device time")
    os.makedirs(a.out, exist_ok=True)
    lines = [{"device": torch.cuda.get_device_name(0), "reps": a.reps, "times": "CUDA-event microseconds: median, min, max"}]
    sizes = [(f"mosei q{nq} d{d}", 16265, nq, d, 2) for nq in (1869, 4643) for d in (40, 80, 600)]
    sizes += [("mosei raw q4643 d335", 16265, 4643, 335, 2), ("mosei raw q1869 d335", 16265, 1869, 335, 2)]
    if not a.skip_table:
        sizes.append(("feature table 16000x1024 q50000", 16000, 50000, 1024, 1000))
    for name, nt, nq, d, classes in sizes:
        table = nq >= 50000
        lines.append(bench_size(name, nt, nq, d, classes, 5, max(3, a.reps // 2) if table else a.reps, not a.no_torch,
                                not a.no_sklearn and not table))
        print(json.dumps(lines[-1]), flush=True)
    if not a.skip_evaluate:
        lines.append(bench_evaluate(max(3, a.reps // 2)))
        print(json.dumps(lines[-1]), flush=True)
    with open(os.path.join(a.out, "knn_bench.txt"), "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    accuracy(os.path.join(a.out, "knn_accuracy.txt"))


if __name__ == "__main__":
    main()
