"""Device time (events) of the alignment metrics on the HIP kernels against the reference's formulation in torch on the
same GPU (vision_language/metrics.py: A @ A.T, fill_diagonal_, argsort, two N x N masks; K @ H @ L @ H), where that fits.

    python scripts/bench_align.py [--reps R]

Sizes: the Gaussian eval (N 2000, d 128, both views), a MultiBench-raw size (N 50000, dA 35, dB 300) and kNN alone at
N 32768, d 256 with its achieved TFLOP/s (2 N^2 d per call)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd")):
    sys.path.insert(0, p)
from umlh import align  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps, warm=2):
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


def ref_knn(x, k):
    return (x @ x.T).fill_diagonal_(-1e8).argsort(dim=1, descending=True)[:, :k]


def ref_mknn(a, b, k):
    ka, kb = ref_knn(a, k), ref_knn(b, k)
    n = ka.shape[0]
    r = torch.arange(n, device=a.device).unsqueeze(1)
    ma = torch.zeros(n, n, device=a.device)
    mb = torch.zeros(n, n, device=a.device)
    ma[r, ka] = 1.0
    mb[r, kb] = 1.0
    return ((ma * mb).sum(dim=1) / k).mean()


def ref_cka(a, b):
    K, L = a @ a.T, b @ b.T
    n = K.shape[0]
    H = torch.eye(n, device=a.device) - 1 / n
    h = lambda X, Y: torch.trace(X @ H @ Y @ H)
    return h(K, L) / (torch.sqrt(h(K, K) * h(L, L)) + 1e-6)


def fits(n, arrays):
    free, _ = torch.cuda.mem_get_info()
    return arrays * n * n * 4 < 0.8 * free


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0)}
    for name, n, da, db in (("gaussian_eval", 2000, 128, 128), ("multibench_raw", 50000, 35, 300)):
        a = torch.randn(n, da, device=DEV, generator=g)
        b = torch.randn(n, db, device=DEV, generator=g) + 5.0
        r = {"N": n, "dA": da, "dB": db}
        r["hip_cka_us"] = timed(lambda: align.cka(a, b), args.reps)
        r["hip_mknn_us"] = timed(lambda: align.mutual_knn(a, b, 10), args.reps)
        r["hip_both_us"] = timed(lambda: (align.cka(a, b), align.mutual_knn(a, b, 10)), args.reps)
        if fits(n, 6):
            r["ref_cka_us"] = timed(lambda: ref_cka(a, b), max(3, args.reps // 4), warm=1)
            r["ref_mknn_us"] = timed(lambda: ref_mknn(a, b, 10), max(3, args.reps // 4), warm=1)
        else:
            r["ref"] = f"does not fit: the reference form needs several N x N fp32 arrays ({n * n * 4 / 2**30:.1f} GiB each)"
        out[name] = r
        print(json.dumps({name: r}), flush=True)
        del a, b
        torch.cuda.empty_cache()
    n, d = 32768, 256
    x = torch.randn(n, d, device=DEV, generator=g)
    us = timed(lambda: align.knn(x, 10), max(5, args.reps // 2))
    r = {"N": n, "d": d, "topk": 10, "hip_knn_us": us, "hip_tflops": 2.0 * n * n * d / (us * 1e-6) / 1e12}
    if fits(n, 3):
        r["ref_knn_us"] = timed(lambda: ref_knn(x, 10), 3, warm=1)
    out["knn_32768x256"] = r
    print(json.dumps({"knn_32768x256": r}), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
