"""Golden vectors of the alignment metrics: runs the reference's own metrics module (vision_language/metrics.py, and the
MultiBench copy's cka) on CPU torch float32 and writes tests/golden/alignment.npz + alignment.partK.npz (one case per
part, every file under 1 MiB).  Needs the reference checkout (REFERENCE_ROOT, default ../reference next to the repo);
no test reads it.

Per case: inputs a, b (float32); the reference's cka (both copies), compute_nearest_neighbors lists for k = 10 and
mutual_knn for k in {1, 10, 32}; the float64 values of the same formulas (tests/_align_ref.py) and per row the float64
gaps around the k-th neighbour with the decidability margin tau_i."""
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
import _align_ref as R  # noqa: E402
from conftest import load_golden  # noqa: E402

KS = (1, 10, 32)
KLIST = 10


def _load_ref(name, path):
    for m in ("torchaudio", "torchaudio.functional"):      # imported by metrics.py, unused by cka / mutual_knn
        stub = types.ModuleType(m)
        stub.__spec__ = mock.MagicMock()
        sys.modules.setdefault(m, stub)
    sys.modules["torchaudio"].functional = sys.modules["torchaudio.functional"]
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def undecidable(a, b):
    """rows that are not set-decidable in both views for every k of KS"""
    bad = np.zeros(a.shape[0], bool)
    for x in (a, b):
        _, s = R.knn64(x, max(KS))
        t = R.tau(x)
        for k in KS:
            bad |= ~R.set_decidable(s, t, k)
    return int(bad.sum())


def gen_case(kind, seed):
    g = np.random.default_rng(seed)
    if kind == "gauss":            # Gaussian-experiment-like: two noisy views of one latent
        z = g.standard_normal((512, 10))
        a = z @ g.standard_normal((10, 100)) + 0.5 * g.standard_normal((512, 100))
        b = z @ g.standard_normal((10, 100)) + 0.5 * g.standard_normal((512, 100))
    elif kind == "offset":         # column means ~50, spread ~1: catastrophic cancellation for X^T Y - N mu mu^T
        z = g.standard_normal((384, 8))
        a = 50 + g.uniform(-1, 1, 64) + z @ g.standard_normal((8, 64)) * 0.3 + g.standard_normal((384, 64)) * 0.8
        b = 50 + g.uniform(-1, 1, 48) + z @ g.standard_normal((8, 48)) * 0.3 + g.standard_normal((384, 48)) * 0.8
    elif kind == "wide":           # N < d
        z = g.standard_normal((96, 12))
        a = z @ g.standard_normal((12, 300)) + g.standard_normal((96, 300))
        b = z @ g.standard_normal((12, 200)) + g.standard_normal((96, 200))
    elif kind == "ragged":
        z = g.standard_normal((257, 6))
        a = z @ g.standard_normal((6, 35)) + g.standard_normal((257, 35))
        b = z @ g.standard_normal((6, 74)) + g.standard_normal((257, 74))
    elif kind == "tiny":           # std 1e-3: the +1e-6 of the CKA denominator moves the value
        z = g.standard_normal((200, 4))
        a = 1e-3 * (z @ g.standard_normal((4, 16)) + g.standard_normal((200, 16)))
        b = 1e-3 * (z @ g.standard_normal((4, 16)) + g.standard_normal((200, 16)))
    else:
        raise ValueError(kind)
    return a.astype(np.float32), b.astype(np.float32)


def record(name, a, b, vl, mb, seed):
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    out = {f"{name}/a": a, f"{name}/b": b, f"{name}/seed": np.int64(seed)}
    out[f"{name}/ref_cka"] = np.float64(vl.AlignmentMetrics.cka(ta, tb, kernel_metric="ip"))
    out[f"{name}/ref_cka_multibench"] = np.float64(mb.AlignmentMetrics.cka(ta, tb, kernel_metric="ip"))
    K = ta @ ta.T
    L = tb @ tb.T
    # the two reference copies (O(N^3) trace form and MultiBench's O(N^2) form) agree to fp32 rounding of their own
    out[f"{name}/ref_copies_absdiff"] = np.float64(abs(out[f"{name}/ref_cka"] - out[f"{name}/ref_cka_multibench"]))
    out[f"{name}/ref_hsic"] = np.array([float(vl.hsic_biased(K, L)), float(vl.hsic_biased(K, K)), float(vl.hsic_biased(L, L))])
    c64 = R.cka64(a, b)
    out[f"{name}/cka64"] = np.array(c64)
    for k in KS:
        out[f"{name}/ref_mknn_k{k}"] = np.float64(vl.AlignmentMetrics.mutual_knn(ta, tb, topk=k))
    for v, x, t in (("a", a, ta), ("b", b, tb)):
        out[f"{name}/ref_knn_{v}"] = vl.compute_nearest_neighbors(t, KLIST).numpy().astype(np.int32)
        i64, s64 = R.knn64(x, max(KS))
        tau = R.tau(x)
        out[f"{name}/tau_{v}"] = tau
        out[f"{name}/knn64_{v}"] = i64[:, :KLIST].astype(np.int32)
        out[f"{name}/list_gap_{v}"] = (s64[:, :KLIST] - s64[:, 1:KLIST + 1]).min(1)
        for k in KS:
            out[f"{name}/set_gap_{v}_k{k}"] = s64[:, k - 1] - s64[:, k]
    for k in KS:
        ka, _ = R.knn64(a, k)
        kb, _ = R.knn64(b, k)
        out[f"{name}/mknn64_k{k}"] = np.float64(R.mutual64(ka, kb))
    out[f"{name}/undecidable"] = np.int64(undecidable(a, b))
    print(f"{name:7s} N={a.shape[0]:4d} dA={a.shape[1]:3d} dB={b.shape[1]:3d} seed={seed}: cka ref {out[f'{name}/ref_cka']:.9f} "
          f"multibench {out[f'{name}/ref_cka_multibench']:.9f} float64 {c64[0]:.9f}; mknn@10 ref {out[f'{name}/ref_mknn_k10']:.6f} "
          f"float64 {out[f'{name}/mknn64_k10']:.6f}; undecidable rows {int(out[f'{name}/undecidable'])}")
    return out


def main():
    vl = _load_ref("ref_vl_metrics", os.path.join(REF, "vision_language", "metrics.py"))
    mb = _load_ref("ref_mb_metrics", os.path.join(REF, "MultiBench", "metrics.py"))
    torch.manual_seed(0)
    parts = []
    for kind in ("gauss", "offset", "wide", "ragged", "tiny"):
        best = None
        for seed in range(40):                 # the first seed whose rows are all set-decidable (else the best seen)
            a, b = gen_case(kind, seed)
            u = undecidable(a, b)
            if best is None or u < best[0]:
                best = (u, seed, a, b)
            if u == 0:
                break
        parts.append(record(kind, best[2], best[3], vl, mb, best[1]))
    gt = load_golden("gaussian_toy")
    parts.append(record("toy", gt["emb_x"].astype(np.float32), gt["emb_y"].astype(np.float32), vl, mb, -1))
    out_dir = os.path.join(ROOT, "tests", "golden")
    names = [next(iter(p_)).split("/")[0] for p_ in parts]
    np.savez_compressed(os.path.join(out_dir, "alignment.npz"), cases=np.array(names))
    for i, p_ in enumerate(parts, 1):
        path = os.path.join(out_dir, f"alignment.part{i}.npz")
        np.savez_compressed(path, **p_)
        assert os.path.getsize(path) < 1 << 20, path
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
