"""Device time (events, medians) of unbiased / RBF CKA, CKNNA and the k-NN list statistics on the HIP kernels against the
reference's formulation in torch on the same GPU (vision_language/metrics.py: dense N x N kernels, hsic_unbiased with a
torch.mm of the two, K @ H @ L @ H, two scattered N x N masks for CKNNA), where that fits.

    python scripts/bench_align_ext.py [--reps R] [--out profiles/align_ext_bench.txt]

Sizes: N 2000, d 128 + 128 (the Gaussian eval; launch-bound, recorded without a bar); N 8192, d 256 + 256 (the bar: the HIP
path is at least as fast as the reference form for RBF CKA and unbiased linear CKA); N 50000, d 35 + 300 (HIP only: the
reference form needs tens of GB).  lcs_knn / edit_distance_knn have no torch form to time: the reference runs a Python
double loop per row on the CPU."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)
from umlh import align  # noqa: E402
from bench_align import DEV, fits, timed  # noqa: E402


def ref_hsic_unbiased(K, L):
    m = K.shape[0]
    Kt, Lt = K.clone().fill_diagonal_(0), L.clone().fill_diagonal_(0)
    v = torch.sum(Kt * Lt.T) + torch.sum(Kt) * torch.sum(Lt) / ((m - 1) * (m - 2)) - 2 * torch.sum(torch.mm(Kt, Lt)) / (m - 2)
    return v / (m * (m - 3))


def ref_hsic_biased(K, L):
    n = K.shape[0]
    H = torch.eye(n, dtype=K.dtype, device=K.device) - 1 / n
    return torch.trace(K @ H @ L @ H)


def ref_cka(a, b, rbf_sigma=None, unbiased=False):
    if rbf_sigma is None:
        K, L = a @ a.T, b @ b.T
    else:
        K = torch.exp(-torch.cdist(a, a) ** 2 / (2 * rbf_sigma ** 2))
        L = torch.exp(-torch.cdist(b, b) ** 2 / (2 * rbf_sigma ** 2))
    h = ref_hsic_unbiased if unbiased else ref_hsic_biased
    return h(K, L) / (torch.sqrt(h(K, K) * h(L, L)) + 1e-6)


def ref_cknna(a, b, topk):
    n = a.shape[0]
    K, L = a @ a.T, b @ b.T

    def sim(X, Y):
        ix = torch.topk(X.clone().fill_diagonal_(float("-inf")), topk, dim=1).indices
        iy = torch.topk(Y.clone().fill_diagonal_(float("-inf")), topk, dim=1).indices
        mask = torch.zeros(n, n, device=a.device).scatter_(1, ix, 1) * torch.zeros(n, n, device=a.device).scatter_(1, iy, 1)
        return ref_hsic_unbiased(mask * X, mask * Y)

    return sim(K, L) / (torch.sqrt(sim(K, K) * sim(L, L)) + 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_ext_bench.txt"))
    ap.add_argument("--sizes", default="2000,8192,50000")
    args = ap.parse_args()
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps})]
    shapes = {2000: (128, 128), 8192: (256, 256), 50000: (35, 300)}
    for n in (int(s) for s in args.sizes.split(",")):
        da, db = shapes[n]
        a = torch.randn(n, da, device=DEV, generator=g)
        b = torch.randn(n, db, device=DEV, generator=g) + 5.0
        sigma = float((da + db) ** 0.5)
        r = {"N": n, "dA": da, "dB": db, "sigma": sigma}
        reps = args.reps if n < 50000 else max(3, args.reps // 3)
        hip = {"unbiased_cka": lambda: align.unbiased_cka(a, b), "rbf_cka": lambda: align.rbf_cka(a, b, sigma),
               "rbf_cka_unbiased": lambda: align.rbf_cka(a, b, sigma, True), "cknna_k10": lambda: align.cknna(a, b, 10),
               "cycle_lcs_edit_k10": lambda: align.list_stats(align.knn(a, 10), align.knn(b, 10))}
        ref = {"unbiased_cka": lambda: ref_cka(a, b, None, True), "rbf_cka": lambda: ref_cka(a, b, sigma, False),
               "rbf_cka_unbiased": lambda: ref_cka(a, b, sigma, True), "cknna_k10": lambda: ref_cknna(a, b, 10)}
        for name, fn in hip.items():
            r[f"hip_{name}_us"] = timed(fn, reps)
        if n <= 8192 and fits(n, 12):
            for name, fn in ref.items():
                r[f"ref_{name}_us"] = timed(fn, max(3, reps // 3), warm=1)
                r[f"speedup_{name}"] = r[f"ref_{name}_us"] / r[f"hip_{name}_us"]
                r[f"value_{name}"] = [float(hip[name]()), float(fn())]
        else:
            r["ref"] = f"not run: the reference form needs about ten N x N fp32 arrays ({n * n * 4 / 2**30:.1f} GiB each)"
        r["rbf_tflops"] = 2.0 * n * n * (da + db) / (r["hip_rbf_cka_us"] * 1e-6) / 1e12
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
        del a, b
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
