"""Golden values of the remaining alignment metrics: runs the reference's own metrics module (vision_language/metrics.py)
on CPU torch and writes tests/golden/alignment_ext.npz (under 1 MiB).  Needs the reference checkout (REFERENCE_ROOT,
default ../reference next to the repo) at generation time only; no test reads it.

The file holds NO input arrays: the inputs are the a / b of the committed `alignment` fixture (six cases).  Per case it
records the reference's value in torch float64 (`*_ref64`, the yardstick) and in float32 (`*_ref32`, what the reference
returns on fp32 features) for

  unbiased_cka and its three hsic_unbiased terms                                  ucka_*, uhsic_*
  cka(kernel_metric='rbf'), biased and unbiased, in two settings                  rbf_{norm,raw}_{b,u}_*
    norm: rows L2-normalised in fp32, sigma = 1 (the reference's demo, metrics.py:355-360)
    raw:  the rows as they are, sigma = the mean of the two views' median pairwise distance (`rbf_raw_sigma`)
  cknna at k = 10 and 32                                                          cknna_k{10,32}_*
  cycle_knn and lcs_knn at k = 10                                                 cycle_k10_*, lcs_k10_*

edit_distance_knn has NO reference value here: the reference computes it with torchaudio.functional.edit_distance and
torchaudio is stubbed (it is not installed); the Levenshtein DP of tests/_align_ext_ref.py is that metric's yardstick."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import _align_ext_ref as X  # noqa: E402
from conftest import load_golden  # noqa: E402
from make_golden_alignment import REF, _load_ref  # noqa: E402

CASES = ("gauss", "offset", "wide", "ragged", "tiny", "toy")


def both(fn, a, b):
    """fn on float64 and on float32 copies of the features"""
    out = []
    for dt in (torch.float64, torch.float32):
        out.append(np.float64(fn(torch.from_numpy(a).to(dt), torch.from_numpy(b).to(dt))))
    return out


def record(name, a, b, vl):
    M = vl.AlignmentMetrics
    out = {}

    def put(key, fn, xa=a, xb=b):
        out[f"{name}/{key}_ref64"], out[f"{name}/{key}_ref32"] = both(fn, xa, xb)

    put("ucka", lambda p, q: M.unbiased_cka(p, q))
    hs64, hs32 = [], []
    for pick in ((0, 1), (0, 0), (1, 1)):
        def term(p, q, pick=pick):
            k = (p @ p.T, q @ q.T)
            return float(vl.hsic_unbiased(k[pick[0]], k[pick[1]]))
        v64, v32 = both(term, a, b)
        hs64.append(v64)
        hs32.append(v32)
    out[f"{name}/uhsic_ref64"], out[f"{name}/uhsic_ref32"] = np.array(hs64), np.array(hs32)
    na, nb = X.normalize_rows(a), X.normalize_rows(b)
    sigma = X.median_sigma(a, b)
    out[f"{name}/rbf_raw_sigma"] = np.float64(sigma)
    for tag, unb in (("b", False), ("u", True)):
        put(f"rbf_norm_{tag}", lambda p, q, unb=unb: M.cka(p, q, kernel_metric="rbf", rbf_sigma=1.0, unbiased=unb), na, nb)
        put(f"rbf_raw_{tag}", lambda p, q, unb=unb: M.cka(p, q, kernel_metric="rbf", rbf_sigma=sigma, unbiased=unb))
    for k in (10, 32):
        put(f"cknna_k{k}", lambda p, q, k=k: M.cknna(p, q, topk=k))
    put("cycle_k10", lambda p, q: M.cycle_knn(p, q, topk=10))
    put("lcs_k10", lambda p, q: float(M.lcs_knn(p, q, topk=10)))
    print(name, {k.split("/")[1]: (float(v) if np.ndim(v) == 0 else v.tolist()) for k, v in out.items()})
    return out


def main():
    vl = _load_ref("ref_vl_metrics_ext", os.path.join(REF, "vision_language", "metrics.py"))
    vl.pymp_available = False
    gold = load_golden("alignment")
    assert tuple(gold["cases"]) == CASES
    out = {"cases": np.array(CASES)}
    for name in CASES:
        out.update(record(name, gold[f"{name}/a"], gold[f"{name}/b"], vl))
    path = os.path.join(ROOT, "tests", "golden", "alignment_ext.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, path
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
