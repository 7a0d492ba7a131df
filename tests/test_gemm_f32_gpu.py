"""umlh_gemm_f32 called directly on every kernel path behind it (gemm_enc, gemm_f32 64x64, gemm_f32 128x128 with fp32-MFMA or x3
products, dw_f32, dw_f32x3, the split-K reduce), and the engine calls on the same dispatcher (umlh_logits, umlh_project) on both
sides of the 768-workgroup switch, against float64 (tests/_gemm_ref.py: the criterion and the dispatch rules).

The case table (_gemm_ref.CASES) runs in fresh child processes, one per setting of the switches UMLH_F32_X3 / UMLH_F32_TM /
UMLH_F32_DW (they are read once per process), one after another.  Every output buffer is (M+1) x ldo floats filled with a
sentinel and every slab buffer is one slab longer than the launch needs and filled with NaN: a write outside the [M, N] window
lands on a sentinel inside the allocation, and the parent checks that every element outside the window is bit-unchanged.

The SHA-256 digest of every (case, setting) window is also compared with the one that scripts/make_step_digests.py recorded in
tests/golden/f32_path_digests.json from an earlier build (the table's "recorded_from"): the kernel paths keep their bits across
commits, not only their accuracy."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _gemm_ref import (CASES, ENVS, SENTINEL_BITS, X3_KERNELS, case_ref, gemm_err, meets_criterion, predict_kernel,
                       slab_count)
from _switches import child_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unpaired-multimodal-learning_amd")

_CHILD = r"""
import ctypes as C, os, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import torch
import umlh
from _gemm_ref import CASES, SENTINEL_BITS, build_case, slab_count
outdir = sys.argv[3]
lib = umlh.load_library()
dev = "cuda:0"
p = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off) if t is not None else None
for c in CASES:
    A, B, a_rows, k_rows = build_case(c)
    M, N, ldo = c["M"], c["N"], c["ldo"]
    ns = slab_count(c["K"], c["splits"])[0]
    dA, dB = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    dr = torch.from_numpy(a_rows).to(dev) if a_rows is not None else None
    dk = torch.from_numpy(k_rows).to(dev) if k_rows is not None else None
    out = torch.full(((M + 1) * ldo,), SENTINEL_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    slabs = torch.full(((ns + 1) * max(M, 1) * ldo,), float("nan"), device=dev) if c["splits"] > 1 else None
    torch.cuda.synchronize()
    rc = lib.umlh_gemm_f32(p(dA, c["a_off"]), p(dB, c["b_off"]), p(out), M, N, c["K"], c["lda"], c["ldb"], ldo, c["ta"], c["tb"],
                           p(dr), p(dk), C.c_float(c["alpha"]), c["splits"], p(slabs), None)
    torch.cuda.synchronize()
    if rc != 0:
        print("umlh_gemm_f32 failed on", c["id"], rc, lib.umlh_last_error(), file=sys.stderr)
        sys.exit(2)
    np.save(os.path.join(outdir, c["id"] + "_out.npy"), out.cpu().numpy())
    if slabs is not None:
        np.save(os.path.join(outdir, c["id"] + "_slabs.npy"), slabs.cpu().numpy())
print("CHILD_OK", len(CASES))
"""


def _run_children(tmp_path):
    script = tmp_path / "gemm_f32_cases.py"
    script.write_text(_CHILD)
    dirs = {}
    for name, env_over in ENVS.items():             # one after another; the first failure ends the test
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([sys.executable, str(script), os.path.dirname(os.path.abspath(__file__)), PKG, str(d)],
                           env=child_env(env_over), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
        dirs[name] = d
    return dirs


def _window(c, buf):
    """The [M, N] window of an (M+1) x ldo output buffer, and the bits of everything outside it."""
    M, N, ldo = c["M"], c["N"], c["ldo"]
    full = buf.reshape(M + 1, ldo)
    mask = np.ones(full.shape, dtype=bool)
    mask[:M, :N] = False
    return full[:M, :N], full.view(np.uint32)[mask]


def window_digests(dirs):
    """{case id: {environment: SHA-256 of the [M, N] window}} of the children's outputs (cases that launch something)."""
    return {c["id"]: {name: hashlib.sha256(np.ascontiguousarray(_window(c, np.load(dirs[name] / (c["id"] + "_out.npy")))[0]).tobytes()).hexdigest()
                      for name in ENVS} for c in CASES if c["M"] and c["N"]}


def _recorded_digests():
    """The same digests of the build that tests/golden/f32_path_digests.json was recorded from (scripts/make_step_digests.py)."""
    with open(os.path.join(ROOT, "tests", "golden", "f32_path_digests.json")) as f:
        return json.load(f)["gemm"]


def _check_nonfinite(kernel, got, ref, S):
    """Exact IEEE pattern on the fp32-MFMA and gemm_enc paths; on the x3 paths an infinite operand may give NaN instead of +-inf
    (its mid piece is inf - inf), so there: non-finite where float64 is, NaN where float64 is, the rest within the criterion."""
    fin = np.isfinite(ref)
    assert fin.any() and (~fin).any()
    if kernel in X3_KERNELS:
        assert not np.isfinite(got[~fin]).any(), "a non-finite operand gave a finite output"
        assert np.isnan(got[np.isnan(ref)]).all(), "NaN did not stay NaN"
    else:
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
        np.testing.assert_array_equal(np.isposinf(got), np.isposinf(ref))
        np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
    return gemm_err(got, ref, S)


@pytest.mark.gpu
def test_gemm_f32_every_kernel_path_against_float64(tmp_path):
    dirs = _run_children(tmp_path)
    digests, kernels, levels, failures = {}, {}, {}, []
    by_case, recorded = window_digests(dirs), _recorded_digests()
    assert sorted(by_case) == sorted(recorded)
    for c in CASES:
        ref, S = case_ref(c) if c["M"] and c["N"] else (None, None)
        for name, env in ENVS.items():
            kernel = predict_kernel(c, env)
            kernels[c["id"], name] = kernel
            got, outside = _window(c, np.load(dirs[name] / (c["id"] + "_out.npy")))
            bad = int((outside != np.uint32(SENTINEL_BITS)).sum())
            if bad:
                failures.append(f"{c['id']} [{name}, {kernel}]: {bad} elements of out outside the [M, N] window were written")
            if c["splits"] > 1 and c["M"]:
                # the GEMM writes only the [M, N] window of each of its slabs: columns [N, ldo) and the spare slab stay NaN
                ns = slab_count(c["K"], c["splits"])[0]
                per = np.load(dirs[name] / (c["id"] + "_slabs.npy")).reshape(ns + 1, c["M"], c["ldo"])
                if not np.isnan(per[:, :, c["N"]:]).all() or not np.isnan(per[ns]).all():
                    failures.append(f"{c['id']} [{name}, {kernel}]: a split-K slab was written outside its [M, N] window")
            if ref is None:
                continue
            digests[c["id"], name] = by_case[c["id"]][name]
            if digests[c["id"], name] != recorded[c["id"]][name]:
                failures.append(f"{c['id']} [{name}, {kernel}]: the bits differ from the recorded build's")
            try:
                err = _check_nonfinite(kernel, got, ref, S) if c["nonfinite"] else gemm_err(got, ref, S)
            except AssertionError as e:
                failures.append(f"{c['id']} [{name}, {kernel}]: non-finite pattern: {str(e)[:300]}")
                continue
            levels.setdefault(kernel, []).append(err)
            if not meets_criterion(err):
                failures.append(f"{c['id']} [{name}, {kernel}]: error max 2^{np.log2(err[0]):.1f} rms 2^{np.log2(err[1]):.1f}")
    # routing without a profiler: x3 products round differently from the fp32 MFMA's, so a case predicted on an x3 kernel
    # differs from its UMLH_F32_X3=0 run somewhere, and a case predicted on the same kernel under two settings is bit-identical
    for c in CASES:
        if not (c["M"] and c["N"]) or c["nonfinite"]:
            continue
        d, k = digests[c["id"], "default"], kernels[c["id"], "default"]
        for name in ENVS:
            if kernels[c["id"], name] == k and digests[c["id"], name] != d:
                failures.append(f"{c['id']}: {name} is predicted on {k} as the default is, but the bits differ")
        if k in X3_KERNELS and digests[c["id"], "x3_off"] == d:
            failures.append(f"{c['id']}: predicted {k}, but the result equals the UMLH_F32_X3=0 run bit for bit")
    lg = lambda v: f"2^{np.log2(v):.1f}" if v > 0 else "0"
    print("GEMM_F32_LEVELS", json.dumps({k: [lg(max(e[0] for e in v)), lg(max(e[1] for e in v))] for k, v in sorted(levels.items())}))
    assert not failures, "\n".join(failures)


# ---- engine calls on the same dispatcher ----
def _engine(d_img, d, C, proj):
    import torch
    import umlh
    e = umlh.HeadEngine(d_img, d, C, has_proj=proj, learnable_temp=True, optimizer="adamw", max_rows_img=12800,
                        max_rows_txt=12800, precision="fp32", device="cuda:0")
    rng = np.random.default_rng(11)
    w = rng.standard_normal((C, d)).astype(np.float32)
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    e.w_head.copy_(torch.from_numpy(w))
    e.scales.copy_(torch.tensor([100.0, 37.0], dtype=torch.float32))     # image scale 100, learnable text scale 37
    wp = None
    if proj:
        wp = (rng.standard_normal((d, d_img)) / np.sqrt(d_img)).astype(np.float32)
        e.w_proj.copy_(torch.from_numpy(wp))
    return e, w, wp


def _unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.mark.gpu
def test_logits_on_both_sides_of_the_x3_switch():
    """umlh_logits (fp32 engine, d = 512, C = 1000): 12160 rows are 760 workgroups of the 128x128 grid (64x64 tile, fp32 MFMA),
    12290 rows are 776 (128x128, x3 products, ragged last tile).  Unit-norm rows through a permuted RowBatch index; image scale
    100, learnable text scale 37 (the device-resident alpha_ptr).  Both sizes meet 1e-4 against the oracle's float64 logits and
    the GEMM criterion.  A row's logits can differ in the last bits with the batch size (the two sizes use different product
    forms): the rows both batches share agree to 1e-4, not bit for bit."""
    import torch
    import umlh
    from oracle import uml_oracle as O
    d, C = 512, 1000
    e, w, _ = _engine(d, d, C, False)
    table = _unit_rows(13000, d, 12)
    X = torch.from_numpy(table).cuda()
    Y = torch.zeros(13000, dtype=torch.int64, device="cuda")
    perm = np.random.default_rng(13).permutation(13000)
    w64 = w.astype(np.float64)
    got = {}
    for rows, kernel in ((12160, "tm1"), (12290, "tm2_x3")):
        assert predict_kernel(dict(ta=0, tb=0, M=rows, N=C, K=d, lda=d, ldb=d, ldo=C, a_rows=True)) == kernel
        idx = perm[:rows]
        xs = table[idx].astype(np.float64)
        for mod, scale in ((0, 100.0), (1, 37.0)):
            z = e.logits(umlh.RowBatch(X, Y, torch.from_numpy(idx).cuda()), mod).cpu().numpy()
            ref = O.head_logits(xs, w64, scale)
            assert np.abs(z - ref).max() < 1e-4, (rows, mod, float(np.abs(z - ref).max()))
            err = gemm_err(z, ref, scale * (np.abs(xs) @ np.abs(w64).T))
            assert meets_criterion(err), (rows, mod, kernel, np.log2(err))
            got[rows, mod] = z
    for mod in (0, 1):
        assert np.abs(got[12160, mod][:100] - got[12290, mod][:100]).max() < 1e-4


@pytest.mark.gpu
def test_projected_head_project_and_logits_on_x3_tiles():
    """has_proj (d_img = 768, d_shared = 1024, C = 1000) at 12290 rows: umlh_project (12290 x 1024 x 768: 8 x 97 = 776 workgroups)
    and the image logits behind it (12290 x 1000 x 1024: 776) both run on the 128x128 x3 tile; against float64."""
    import torch
    import umlh
    d_img, d, C, rows = 768, 1024, 1000, 12290
    e, w, wp = _engine(d_img, d, C, True)
    assert predict_kernel(dict(ta=0, tb=0, M=rows, N=d, K=d_img, lda=d_img, ldb=d_img, ldo=d, a_rows=True)) == "tm2_x3"
    assert predict_kernel(dict(ta=0, tb=0, M=rows, N=C, K=d, lda=d, ldb=d, ldo=C, a_rows=False)) == "tm2_x3"
    table = _unit_rows(12800, d_img, 14)
    idx = np.random.default_rng(15).permutation(12800)[:rows]
    batch = umlh.RowBatch(torch.from_numpy(table).cuda(), torch.zeros(12800, dtype=torch.int64, device="cuda"),
                          torch.from_numpy(idx).cuda())
    h = e.project(batch).cpu().numpy()
    z = e.logits(batch, 0).cpu().numpy()
    xs, wp64, w64 = table[idx].astype(np.float64), wp.astype(np.float64), w.astype(np.float64)
    h_ref = xs @ wp64.T
    err = gemm_err(h, h_ref, np.abs(xs) @ np.abs(wp64).T)
    assert meets_criterion(err), ("project", np.log2(err))
    # the logits GEMM multiplies the fp32 projection the first GEMM wrote: the criterion is applied to that GEMM alone, and the
    # end-to-end logits are within 1e-4 of float64 through both GEMMs
    h32 = h.astype(np.float64)
    err = gemm_err(z, 100.0 * h32 @ w64.T, 100.0 * np.abs(h32) @ np.abs(w64).T)
    assert meets_criterion(err), ("logits", np.log2(err))
    assert np.abs(z - 100.0 * h_ref @ w64.T).max() < 1e-4
