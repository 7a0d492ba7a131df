"""Device time (events, medians) and accuracy of umlh.align.svcca against the reference's form on the same GPU:
torch.svd_lowrank of the standardised views on the device, then scikit-learn's CCA on the host as in
MultiBench/metrics.py:129-160, or, where scikit-learn is absent, a float64 SVD of U_a^T U_b standing in for it.

    python scripts/bench_svcca.py [--reps R] [--only-kernels]

Writes profiles/svcca_bench.txt (times; no speed bar is set) and profiles/svcca_accuracy.txt: for every case of
tests/golden/svcca.npz the errors of the HIP value and canonical correlations against the float64 closed form next to the
reference's own (five seeds, stored in the golden), the eigenpair ratios of umlh.principal_subspace next to those of
numpy.linalg.eigh on the same float64 Gram (every view, and the generated 600 x 512 matrix of the tests), and the invariance
figures of the tests (row permutation, exact affine maps, swapped views, an added constant column).  ``--only-kernels`` runs the HIP op once per size and writes nothing."""
import argparse
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import umlh  # noqa: E402
import _svcca_ref as R  # noqa: E402  (the float64 yardstick and the generated inputs of the tests)
from bench_align import DEV, timed  # noqa: E402

try:
    from sklearn.cross_decomposition import CCA
except ImportError:
    CCA = None

SIZES = ((1000, 35, 300), (8192, 512, 512), (50000, 300, 300))      # 1000 x 35 / 300: the capture of MultiBench/train.py:308
Q = 10
EPS = 2.0 ** -53


def planted(n, d, g):
    lat = torch.randn(n, Q, device=DEV, generator=g)
    rows = torch.linalg.qr(torch.randn(d, Q, device=DEV, generator=g))[0]
    return (lat * torch.linspace(24.0, 12.0, Q, device=DEV)) @ rows.T + torch.randn(n, d, device=DEV, generator=g)


def ref_svcca(a, b, q=Q):
    def pre(x):
        x = x - torch.mean(x, axis=0)
        return x / (torch.std(x, axis=0) + 1e-8)
    u1, u2 = torch.svd_lowrank(pre(a), q=q)[0], torch.svd_lowrank(pre(b), q=q)[0]
    if CCA is None:
        return float(torch.linalg.svdvals(u1.double().T @ u2.double()).mean())
    u1, u2 = u1.cpu().numpy(), u2.cpu().numpy()
    c1, c2 = CCA(n_components=q).fit(u1, u2).transform(u1, u2)
    return float(np.mean([np.corrcoef(c1[:, i], c2[:, i])[0, 1] for i in range(q)]))


def load_golden():
    """tests/golden/svcca.npz and its parts, if any, as one dict."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "svcca*.npz"))):
        with np.load(path, allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
    return out


def eigenpair_rows(name, x, q):
    for std in (0, 1):
        G = R.gram64(x, bool(std))
        lam, v = (t.cpu().numpy() for t in umlh.principal_subspace(torch.from_numpy(x).to(DEV), q, standardize=bool(std)))
        lam64, v64, all64 = R.top_eigh(G, q)
        hip, ref = R.eig_ratios(G, lam, v), R.eig_ratios(G, lam64, v64)
        yield {"case": name, "d": x.shape[1], "q": q, "standardize": std, "hip_residual_ratio": hip[0],
               "hip_orthogonality_ratio": hip[1], "eigh_residual_ratio": ref[0], "eigh_orthogonality_ratio": ref[1],
               "projector_distance": float(np.linalg.norm(v @ v.T - v64 @ v64.T, 2)),
               "relative_gap": float((all64[q - 1] - all64[q]) / all64[0]) if q < x.shape[1] else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only-kernels", action="store_true")
    args = ap.parse_args()
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    if args.only_kernels:
        for n, da, db in SIZES:
            umlh.svcca(planted(n, da, g), planted(n, db, g), Q)
        torch.cuda.synchronize()
        return
    tail = "scikit-learn CCA on the host" if CCA is not None else "float64 SVD of U_a^T U_b (scikit-learn absent)"
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "q": Q, "unit": "us, median of device-event times",
                         "reference_form": "torch.svd_lowrank on the device + " + tail})]
    for n, da, db in SIZES:
        a, b = planted(n, da, g), planted(n, db, g)
        r = {"n": n, "d_a": da, "d_b": db}
        r["hip_svcca_us"] = timed(lambda: umlh.svcca(a, b, Q), args.reps)
        r["hip_principal_subspace_b_us"] = timed(lambda: umlh.principal_subspace(b, Q, standardize=True), args.reps)
        r["hip_svdvals_b_us"] = timed(lambda: umlh.svdvals(b), args.reps)
        r["reference_form_us"] = timed(lambda: ref_svcca(a, b), max(3, args.reps // 2), warm=1)
        r["reference_over_hip"] = r["reference_form_us"] / r["hip_svcca_us"]
        r["values"] = [float(umlh.svcca(a, b, Q)), ref_svcca(a, b)]
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "svcca_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")

    gold = load_golden()
    hip = lambda x, y, q: float(umlh.svcca(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(y)).to(DEV), q))
    acc = [json.dumps({"device": torch.cuda.get_device_name(0), "errors": "|svcca - closed64| and max_k |rho_k - rho64_k| against the "
                       "float64 closed form; reference = MultiBench AlignmentMetrics.svcca on the CPU, seeds 0-4 (from the golden); "
                       "eigenpair ratios: max|GV - VL| / (d eps lam_1) and max|V^T V - I| / (d eps), eps = 2^-53, G in float64"})]
    for case in gold["cases"]:
        a, b, q = gold[f"{case}/a"], gold[f"{case}/b"], int(gold[f"{case}/q"])
        closed = float(gold[f"{case}/closed64"])
        val, rho, _ = umlh.svcca_terms(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), q)
        acc.append(json.dumps({"case": str(case), "shape": [a.shape[0], a.shape[1], b.shape[1], q], "hip_value_err": abs(float(val) - closed),
                               "hip_rho_err": float(np.abs(rho.cpu().numpy() - gold[f"{case}/rho64"]).max()),
                               "reference_fp32_err": float(np.abs(gold[f"{case}/ref32"] - closed).max()),
                               "reference_fp64_err": float(np.abs(gold[f"{case}/ref64"] - closed).max())}))
        print(acc[-1], flush=True)
        for view, x in (("a", a), ("b", b)):
            for r in eigenpair_rows(f"{case}-{view}", x, q):
                acc.append(json.dumps(r))
                print(acc[-1], flush=True)
    for r in eigenpair_rows("gen512 (600 x 512, generated)", R.matrix_512(), 10):
        acc.append(json.dumps(r))
        print(acc[-1], flush=True)
    # invariances on the quantised pair of the tests (the affine maps are exact in fp32)
    a, b = R.quantised_pair()
    perm, a2, b2 = R.invariance_maps(a, b)
    base = hip(a, b, 6)
    acc.append(json.dumps({"case": "invariances, quantised 300 x 24 / 30, q 6", "svcca": base,
                           "row_permutation": abs(hip(a[perm], b[perm], 6) - base),
                           "affine_map_of_a": abs(hip(a2.astype(np.float32), b, 6) - base),
                           "affine_map_of_b": abs(hip(a, b2.astype(np.float32), 6) - base),
                           "swapped_views": abs(hip(b, a, 6) - base)}))
    print(acc[-1], flush=True)
    mid_a, mid_b = gold["mid/a"], gold["mid/b"]
    with_const = np.concatenate([mid_a[:, :9], np.full((mid_a.shape[0], 1), 7.5, np.float32), mid_a[:, 9:]], axis=1)
    acc.append(json.dumps({"case": "constant column added to mid-a", "difference": abs(hip(with_const, mid_b, 10) - hip(mid_a, mid_b, 10))}))
    print(acc[-1], flush=True)
    with open(os.path.join(ROOT, "profiles", "svcca_accuracy.txt"), "w") as f:
        f.write("\n".join(acc) + "\n")


if __name__ == "__main__":
    main()
