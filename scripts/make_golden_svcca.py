"""Golden vectors of SVCCA: runs the reference's own AlignmentMetrics.svcca (MultiBench/metrics.py:129-160: torch.svd_lowrank
+ scikit-learn's CCA) and writes tests/golden/svcca.npz (+ svcca.partK.npz, every file under 1 MiB).  Needs the reference
checkout (REFERENCE_ROOT, default ../reference next to the repo) and scikit-learn; no test reads either.

Per case: the fp32 inputs a, b and q; the closed-form float64 value and canonical correlations (tests/_svcca_ref.py); the
reference's value for torch / numpy seeds 0-4 on the fp32 inputs (ref32[5]) and on float64 copies (ref64[5]); and `bound`, the
distance from the closed form within which all ten must lie (a condition on the inputs: a case that breaks it needs a wider
planted gap, not a wider bound).

All cases are planted spectra (tests/_svcca_ref.py: gen_case): q latent directions of strengths 3 -> 1.5 times GAIN over unit
noise, `shared` of them common to both views, so that sigma_(q+1) / sigma_q of each standardised view stays near 0.15 and the
top-q subspace is well defined."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _svcca_ref as R  # noqa: E402
from make_golden_alignment import REF, _load_ref  # noqa: E402

BOUND = 1e-4
SEEDS = range(5)
#        name     n    d_a  d_b  q   shared
CASES = (("mosei", 257, 35, 300, 10, 6),
         ("mid", 400, 32, 48, 10, 5),
         ("offset", 500, 64, 64, 8, 4),
         ("wide", 40, 64, 48, 5, 3),
         ("q1", 300, 20, 24, 1, 1),
         ("full", 300, 6, 6, 6, 3),
         ("same", 300, 40, 40, 10, 10))


def reference_values(mb, a, b, q, dtype):
    out = []
    for seed in SEEDS:
        torch.manual_seed(seed)
        np.random.seed(seed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out.append(float(mb.AlignmentMetrics.svcca(torch.from_numpy(a).to(dtype), torch.from_numpy(b).to(dtype), cca_dim=q)))
    return np.array(out)


def main():
    mb = _load_ref("ref_mb_metrics", os.path.join(REF, "MultiBench", "metrics.py"))
    parts = []
    for name, n, d_a, d_b, q, shared in CASES:
        a, b = R.gen_case(name, n, d_a, d_b, q, shared)
        rho = R.rho64(a, b, q)
        closed = float(rho.mean())
        ref32, ref64 = reference_values(mb, a, b, q, torch.float32), reference_values(mb, a, b, q, torch.float64)
        gaps = [np.linalg.svd(R.standardise64(x), compute_uv=False) for x in (a, b)]
        ratio = max(s[q] / s[q - 1] if q < len(s) else 0.0 for s in gaps)
        e32, e64 = np.abs(ref32 - closed).max(), np.abs(ref64 - closed).max()
        print(f"{name:7s} {a.shape} {b.shape} q={q}: closed {closed:.15f}  sigma_(q+1)/sigma_q {ratio:.3f}  "
              f"reference max error fp32 {e32:.3e} fp64 {e64:.3e}")
        assert max(e32, e64) <= BOUND, name
        parts.append({f"{name}/a": a, f"{name}/b": b, f"{name}/q": np.int64(q), f"{name}/closed64": np.float64(closed),
                      f"{name}/rho64": rho, f"{name}/ref32": ref32, f"{name}/ref64": ref64, f"{name}/bound": np.float64(BOUND)})
    # the first file holds the case list and as many cases as fit under the size limit, the rest go to parts
    files, cur = [], {"cases": np.array([c[0] for c in CASES])}
    for part in parts:
        size = sum(v.nbytes for v in list(cur.values()) + list(part.values()))
        if size > 900 * 1024 and len(cur) > 1:
            files.append(cur)
            cur = {}
        cur.update(part)
    files.append(cur)
    for k, content in enumerate(files):
        path = os.path.join(ROOT, "tests", "golden", "svcca.npz" if k == 0 else f"svcca.part{k}.npz")
        np.savez_compressed(path, **content)
        assert os.path.getsize(path) < 1 << 20, path
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
