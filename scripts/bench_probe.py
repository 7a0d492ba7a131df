"""Device time of the linear probes (umlh.probe) and of one whole multibench.train.evaluate, next to sklearn's CPU time on
the same arrays when sklearn imports on this machine.

    python scripts/bench_probe.py [--reps R] [--out DIR] [--no-sklearn]

Writes DIR/probe_bench.txt (one JSON line per size) and DIR/probe_accuracy.txt (max|w_gpu - w*| per recorded case, w* the
float64 optimum of tests/_probe_ref.py).  Sizes: the MOSI probes (N 1 284, z 40: d 40 and 80, StandardScaler + the liblinear
objective), the MOSEI probes (N 16 265, z 40 and z 300: d 40, 80, 300, 600), d 600 at N 4 000, and evaluate() at the MOSI
shape (1 284 / 229 / 686 sequences, T 50, batch 32, z 40).  A fit's time is CUDA-event time from the enqueue of its first
launch to the end of its last one, so it includes the launches that return at once after the fit has converged."""
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
import _probe_ref as R  # noqa: E402

DEV = "cuda:0"
# sklearn on the 16-core build machine, synthetic embeddings, the reference's estimator settings (not this machine)
BUILD_MACHINE_SKLEARN_S = {"N 1284-4000, d 40-80": "0.28-0.5", "N 16000, d 300": "1.2", "N 4000, d 600": "3.2"}


def timed(fn, reps, warm=1):
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
    return ts[len(ts) // 2]


def data(n, d, seed, shift=0.2):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * rng.uniform(0.3, 2.0, d) + shift * rng.standard_normal(d)).astype(np.float32)
    wt = rng.standard_normal(d) / np.sqrt(d)
    y = ((x - x.mean(0)) @ wt + 0.5 * rng.standard_normal(n) > 0).astype(np.int64)
    return x, y


def sklearn_fit_seconds(x, y, kind):
    try:
        from sklearn.linear_model import LogisticRegression
        from sklearn.pipeline import make_pipeline
        from sklearn.preprocessing import StandardScaler
    except Exception:
        return None
    clf = (make_pipeline(StandardScaler(), LogisticRegression(max_iter=1000, solver="liblinear")) if kind == "liblinear"
           else LogisticRegression(max_iter=200))
    t0 = time.perf_counter()
    clf.fit(x, y)
    return time.perf_counter() - t0


def bench_fit(n, d, kind, reps, use_sklearn):
    x, y = data(n, d, seed=n + d)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV).to(torch.int32)
    holder = {}

    def run():
        holder["p"] = umlh.LogisticProbe(kind).fit(xd, yd, check_classes=False)
    us = timed(run, reps)
    pr = holder["p"]
    t0 = time.perf_counter()
    run()
    enqueue_us = (time.perf_counter() - t0) * 1e6
    torch.cuda.synchronize()
    rec = pr.record()
    out = {"N": n, "d": d, "kind": kind, "hip_fit_us": us, "hip_enqueue_us": enqueue_us, "iterations": rec["n_iter"],
           "converged": rec["converged"], "max_grad": rec["max_grad"]}
    if use_sklearn:
        s = sklearn_fit_seconds(x, y, kind)
        if s is not None:
            out["sklearn_cpu_fit_s_this_machine"] = s
    return out


def bench_evaluate(reps):
    from multibench.models import Linear, Transformer, UML
    from multibench.train import evaluate, evaluate_raw_data
    z, dx, dy, T, bs = 40, 35, 300, 50, 32
    torch.manual_seed(0)
    m = UML(Linear(dx, z), Linear(dy, z), Transformer(z, z, nhead=5, num_layers=5, conv1d=True, out_last=False, pos_embd=True,
                                                       pos_learnable=False, max_len=128),
            [Linear(z, dx), Linear(z, dy)], modality="xy").to(DEV)
    rng = np.random.default_rng(1)
    cfg = {"freq": 100}
    for t, n in (("train", 1284), ("val", 229), ("test", 686)):
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
            ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2] * 1e3
    return {"shape": "MOSI: 1284/229/686 sequences, T 50, batch 32, z 40, dx 35, dy 300",
            "evaluate_ms_wall": wall(lambda: evaluate(m, cfg, "mosi", device=DEV)),
            "evaluate_raw_data_ms_wall": wall(lambda: evaluate_raw_data(cfg, "mosi", device=DEV)),
            "evaluate_lbfgs_kind_ms_wall": wall(lambda: evaluate(m, cfg, "mosei", device=DEV))}


def accuracy(path):
    from conftest import load_golden
    with open(path, "w") as f:
        f.write("# max|w_gpu - w*| per recorded case (w*: float64 optimum, tests/_probe_ref.py); sklearn's own distance beside it\n")
        for tag in ("mosi_a", "mosi_b", "mosei_a", "mosei_b", "humor_c"):
            g = load_golden("probe_" + tag)
            kind = "liblinear" if int(g["kind"]) == R.LIBLINEAR else "lbfgs"
            pr = umlh.LogisticProbe(kind).fit(torch.from_numpy(g["x_train"]).to(DEV), torch.from_numpy(g["y_train"]).to(DEV))
            w = torch.cat([pr.coef_.reshape(-1), pr.intercept_]).cpu().numpy()
            line = json.dumps({"case": tag, "kind": kind, "N": int(g["x_train"].shape[0]), "d": int(g["x_train"].shape[1]),
                               "delta_gpu": float(np.abs(w - g["w_star"]).max()), "delta_sklearn": float(g["delta_ref"]),
                               "iterations": pr.n_iter_, "converged": pr.converged_, "max_grad": pr.max_grad_})
            print(line)
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_probe.py needs a GPU: a CPU run says nothing about device time")
    os.makedirs(a.out, exist_ok=True)
    lines = [{"device": torch.cuda.get_device_name(0), "sklearn_cpu_fit_s_build_machine": BUILD_MACHINE_SKLEARN_S}]
    for n, d, kind in ((1284, 40, "liblinear"), (1284, 80, "liblinear"), (16265, 40, "lbfgs"), (16265, 80, "lbfgs"),
                       (16265, 300, "lbfgs"), (16265, 600, "lbfgs"), (4000, 600, "lbfgs")):
        lines.append(bench_fit(n, d, kind, a.reps, not a.no_sklearn))
        print(json.dumps(lines[-1]), flush=True)
    lines.append(bench_evaluate(max(3, a.reps // 2)))
    print(json.dumps(lines[-1]), flush=True)
    with open(os.path.join(a.out, "probe_bench.txt"), "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    accuracy(os.path.join(a.out, "probe_accuracy.txt"))


if __name__ == "__main__":
    main()
