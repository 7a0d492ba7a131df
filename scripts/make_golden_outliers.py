"""Golden values of the outlier clamp: runs the reference's own remove_outliers and compute_knn_accuracy
(vision_language/metrics.py:327-341, :258-269) on CPU torch and writes tests/golden/outliers.npz (well under 1 MiB).  Needs the
reference checkout (REFERENCE_ROOT, default ../reference next to the repo) at generation time only; no test reads it.

Per case `<name>/`: x (fp32 input), q (float64), exact (0/1), out (the reference's result), q_val (the bound it clamped at,
recomputed with the reference's own expression) and, for exact = 0, rowq (torch.quantile(x.abs().flatten(1), q, dim=1), the
per-row values the bound is the mean of).  `cases` lists the names.  Lists: knn2 [n, k] and knn3 [n, k, k] with acc2 / acc3."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from make_golden_alignment import REF, _load_ref  # noqa: E402


def inputs():
    rng = np.random.default_rng(20)
    g = lambda *s: rng.standard_normal(s).astype(np.float32)
    heavy = lambda *s: rng.standard_t(1.5, s).astype(np.float32)
    c = {}
    c["gauss_64x33_q95"] = (g(64, 33), 0.95)
    c["gauss_17x257_q50"] = (g(17, 257), 0.5)                 # odd d, q = 0.5: pos integral
    c["gauss_8x1100_q95"] = (g(8, 1100) * 3.0, 0.95)
    c["gauss_300x20_q999"] = (g(300, 20), 0.999)
    c["heavy_40x100_q999"] = (heavy(40, 100), 0.999)
    c["heavy_33x64_q95"] = (heavy(33, 64), 0.95)
    c["heavy_5x2_q50"] = (heavy(5, 2), 0.5)
    c["cube_6x5x7_q95"] = (g(6, 5, 7), 0.95)
    c["cube_4x3x50_q50"] = (heavy(4, 3, 50), 0.5)
    x = g(5, 16); x[2, 7] = np.nan
    c["nan_5x16_q50"] = (x, 0.5)
    x = g(5, 16); x[1, 3] = np.inf; x[4, 0] = -np.inf
    c["inf_5x16_q95"] = (x, 0.95)
    x = g(6, 9); x[0, :4] = -0.0; x[1, :] = 0.0; x[2, 5] = -0.0
    c["negzero_6x9_q50"] = (x, 0.5)
    x = np.zeros((3, 8), np.float32); x[:, ::2] = -0.0
    c["allzero_3x8_q50"] = (x, 0.5)                           # bound 0: which zero the clamp returns
    return c


def main():
    vl = _load_ref("ref_vl_metrics", os.path.join(REF, "vision_language", "metrics.py"))
    out = {}
    names = []
    for base, (x, q) in inputs().items():
        for exact in (0, 1):
            name = f"{base}_{'exact' if exact else 'rows'}"
            t = torch.from_numpy(x)
            res = vl.remove_outliers(t, q, exact=bool(exact))
            if exact:
                q_val = t.view(-1).abs().sort().values[int(q * t.numel())]
            else:
                rowq = torch.quantile(t.abs().flatten(start_dim=1), q, dim=1)
                q_val = rowq.mean()
                out[f"{name}/rowq"] = rowq.numpy()
            assert torch.equal(torch.nan_to_num(res, nan=7.0), torch.nan_to_num(t.clamp(-q_val, q_val), nan=7.0))
            out[f"{name}/x"], out[f"{name}/q"], out[f"{name}/exact"] = x, np.float64(q), np.int64(exact)
            out[f"{name}/out"], out[f"{name}/q_val"] = res.numpy(), q_val.numpy()
            names.append(name)
    assert vl.remove_outliers(torch.ones(2, 2), 1) is not None
    rng = np.random.default_rng(21)
    knn2 = rng.integers(0, 50, (50, 5)).astype(np.int64)
    knn3 = rng.integers(0, 30, (30, 4, 4)).astype(np.int64)
    out["knn2"], out["acc2"] = knn2, vl.compute_knn_accuracy(torch.from_numpy(knn2)).numpy()
    out["knn3"], out["acc3"] = knn3, vl.compute_knn_accuracy(torch.from_numpy(knn3)).numpy()
    out["cases"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "outliers.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(names)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
