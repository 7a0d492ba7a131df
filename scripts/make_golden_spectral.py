"""Golden vectors of the effective rank: runs the reference's own compute_effective_rank (MultiBench/utilis.py:27-36) and
torch.linalg.svdvals in float32 on the CPU and writes tests/golden/effective_rank.npz: small stored inputs, the
reference's fp32 outputs, the float64 singular values and effective ranks of the same inputs (tests/_spectral_ref.py) and
the reference's own errors against float64.  Needs the reference checkout (REFERENCE_ROOT, default ../reference next to
the repo); no test reads it."""
import importlib.util
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REFERENCE_ROOT", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _spectral_ref as R  # noqa: E402


def _load_ref(name, path):
    for m in ("torchaudio", "torchaudio.functional"):      # imported by metrics.py, unused here
        stub = types.ModuleType(m)
        stub.__spec__ = mock.MagicMock()
        sys.modules.setdefault(m, stub)
    sys.modules["torchaudio"].functional = sys.modules["torchaudio.functional"]
    sys.path.insert(0, os.path.dirname(path))               # utilis.py imports its sibling metrics.py
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.dirname(path))
        sys.modules.pop("metrics", None)
    return mod


def gen_case(kind):
    g = np.random.default_rng({"ragged": 1, "wide": 2, "batch3": 3, "rank5": 4}[kind])
    if kind == "ragged":           # 257 x 35, columns offset from zero with unequal scales
        a = 3.0 + g.uniform(-1, 1, 35) + g.standard_normal((257, 35)) * g.uniform(0.2, 2.0, 35)
    elif kind == "wide":           # n < d: 40 singular values, 24 exact zeros in the Gram spectrum
        a = g.standard_normal((40, 64))
    elif kind == "batch3":         # the (B, N, D) form of compute_effective_rank
        a = g.standard_normal((3, 120, 24)) * np.array([1.0, 0.05, 20.0])[:, None, None]
        a[1] = a[1] @ np.diag(np.logspace(0, -3, 24))
    elif kind == "rank5":          # exactly rank 5 before rounding to fp32: 43 singular values at fp32 rounding level
        a = g.standard_normal((200, 5)) @ g.standard_normal((5, 48))
    else:
        raise ValueError(kind)
    return a.astype(np.float32)


def record(name, a, U):
    t = torch.from_numpy(a)
    t3 = t if t.ndim == 3 else t.unsqueeze(0)
    ref_sv = torch.linalg.svdvals(t3).numpy()
    ref_er = U.compute_effective_rank(t3).numpy()
    sv64, er64 = R.svdvals64(a.reshape(t3.shape)), R.erank64(a.reshape(t3.shape))
    errs = np.array([R.errors(ref_sv[b], ref_er[b], sv64[b], er64[b]) for b in range(t3.shape[0])])
    out = {f"{name}/a": a, f"{name}/ref_sv": ref_sv, f"{name}/ref_erank": ref_er, f"{name}/sv64": sv64, f"{name}/erank64": er64,
           f"{name}/ref_sv_err": errs[:, 0], f"{name}/ref_erank_err": errs[:, 1]}
    for b in range(t3.shape[0]):
        print(f"{name:7s}[{b}] {tuple(t3.shape[1:])}: erank ref {ref_er[b]:.7f} float64 {er64[b]:.9f}; reference errors "
              f"sv {errs[b, 0]:.3e} sigma_max, erank {errs[b, 1]:.3e}")
    return out


def main():
    U = _load_ref("ref_mb_utilis", os.path.join(REF, "MultiBench", "utilis.py"))
    torch.manual_seed(0)
    names = ["ragged", "wide", "batch3", "rank5"]
    out = {"cases": np.array(names)}
    for kind in names:
        out.update(record(kind, gen_case(kind), U))
    path = os.path.join(ROOT, "tests", "golden", "effective_rank.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, path
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
