"""GPU: the MultiBench critics of include/umlh.h (umlh_seq_mse_forward / _backward, umlh_infonce_forward / _backward) called on
their own through ctypes against the float64 contract of tests/_critic_ref.py: single sums under the GEMM criterion, ties to the
kernels' own outputs bit for bit, composites under the CPU-calibrated bounds of that module.  No tolerance is chosen here.

Every output buffer is filled with a NaN sentinel and is one row longer than the call needs: all of the output must be written and
nothing behind it.  The scratch of the decoder backward is sized by the size query plus a NaN tail that must survive.  Run with -s
to see the CRITIC_LEVELS line (profiles/critic_accuracy.txt)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _critic_ref as R
from _gemm_ref import CRIT_MAX, CRIT_RMS, SENTINEL_BITS, gemm_err, meets_criterion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
LEVELS = {}


@pytest.fixture(scope="module")
def lib():
    import umlh
    return umlh.load_library()


def _ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.umlh_last_error())


_ALIVE = []


@pytest.fixture(autouse=True)
def _inputs_stay_alive():
    """A device input made by dev() lives until its test ends (see tests/test_encoder_kernels_gpu.py)."""
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def dev(a):
    _ALIVE.append(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    return _ALIVE[-1]


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def sentinel(n, row=64):
    """n + row floats of the NaN sentinel."""
    return torch.full((n + row,), SENTINEL_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def written(buf, n, what=""):
    """The first n floats of a sentinel buffer as numpy: all of them written, the tail behind them untouched."""
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    bits = a.view(np.uint32)
    assert (bits[n:] == np.uint32(SENTINEL_BITS)).all(), f"{what}: written past the end of the output"
    assert (bits[:n] != np.uint32(SENTINEL_BITS)).all(), f"{what}: {int((bits[:n] == np.uint32(SENTINEL_BITS)).sum())} outputs not written"
    return a[:n].copy()


def bit_equal(got, ref, what=""):
    got, ref = np.asarray(got, F32).ravel(), np.asarray(ref, F32).ravel()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), what


def note(fam, key, err):
    LEVELS.setdefault(fam, {})[key] = max(LEVELS.get(fam, {}).get(key, 0.0), float(err))


def within(fam, got, ref, what):
    """Every output of `ref` under the family's bound; returns the failures."""
    bad = []
    for k in ref:
        e = R.comp_err(got[k], ref[k])
        note(fam, k, e)
        if not e <= R.BOUNDS[fam][k]:
            bad.append(f"{what} {k}: 2^{np.log2(e):.1f} > 2^{np.log2(R.BOUNDS[fam][k]):.0f}")
    return bad


def sum_crit(fam, key, got, ref, S, what):
    e = gemm_err(np.asarray(got).ravel(), np.asarray(ref).ravel(), np.asarray(S).ravel())
    note(fam, key + "_max", e[0])
    note(fam, key + "_rms", e[1])
    return [] if meets_criterion(e) else [f"{what} {key}: max 2^{np.log2(e[0]):.1f} rms 2^{np.log2(e[1]):.1f}"]


def nonneg_crit(fam, key, got, ref, what):
    """A sum of non-negative terms relative to its float64 value at CRIT_MAX; a zero must be reproduced exactly."""
    got, ref = np.asarray(got, F64).ravel(), np.asarray(ref, F64).ravel()
    if not np.isfinite(got).all() or (got[ref == 0] != 0).any():
        return [f"{what} {key}: not finite, or not 0 where the reference is 0"]
    pos = ref > 0
    e = float((np.abs(got - ref)[pos] / ref[pos]).max(initial=0.0))
    note(fam, key, e)
    return [] if e <= CRIT_MAX else [f"{what} {key}: 2^{np.log2(e):.1f} > 2^-20"]


# ---------------------------------------------------------------------------------------------------------------------------- #
# decoder Linear + masked next-step MSE
# ---------------------------------------------------------------------------------------------------------------------------- #
def _forward(lib, c, dz, dw, db, dx, dl, with_recon):
    B, T, Z, D = c["B"], c["T"], c["Z"], c["D"]
    n = B * T * D
    recon = sentinel(n, D) if with_recon else None
    dres, rp, lc = sentinel(n, D), sentinel(B * T), sentinel(2)
    _ok(lib, lib.umlh_seq_mse_forward(vp(dz), vp(dw), vp(db), vp(dx), vp(dl), B, T, Z, D, vp(recon), vp(dres), vp(rp), vp(lc), None),
        "seq_mse_forward")
    return dict(recon=written(recon, n, "recon").reshape(B, T, D) if with_recon else None,
                dres=written(dres, n, "dres").reshape(B, T, D), row_partial=written(rp, B * T, "row_partial").reshape(B, T),
                loss_cnt=written(lc, 2, "loss_cnt"))


def _backward(lib, c, dz, dw, dres, loss_cnt, grad_out, with_scratch):
    """dz [B,T,Z], dw [D,Z], db [D] of umlh_seq_mse_backward on the given leaves (numpy fp32 dres / loss_cnt)."""
    B, T, Z, D = c["B"], c["T"], c["Z"], c["D"]
    n_scr = int(lib.umlh_seq_mse_backward_scratch_floats(B, T, Z, D))
    assert n_scr == R.scratch_floats(B, T, Z, D)
    scratch = torch.full((n_scr + 256,), float("nan"), device=DEV) if with_scratch else None
    gz, gw, gb = sentinel(B * T * Z, Z), sentinel(D * Z, Z), sentinel(D)
    _ok(lib, lib.umlh_seq_mse_backward(vp(dz), vp(dw), vp(dev(dres)), vp(dev(np.asarray(loss_cnt, F32))), vp(dev(np.array([grad_out], F32))),
                                       B, T, Z, D, vp(gz), vp(gw), vp(gb), vp(scratch), None), "seq_mse_backward")
    what = f"{c['id']} scratch={with_scratch}"
    out = dict(dz=written(gz, B * T * Z, what + " dz").reshape(B, T, Z), dw=written(gw, D * Z, what + " dw").reshape(D, Z),
               db=written(gb, D, what + " db"))
    if with_scratch:
        assert torch.isnan(scratch[n_scr:]).all(), what + ": written past the queried scratch"
    return out


def _backward_both(lib, c, dz, dw, z, w, dres, loss_cnt, grad_out, what):
    """The backward with the queried scratch and (sp > 1) with scratch == NULL: each against float64 given the leaves, dz bit-equal
    between the two.  Returns (the outputs of the scratch run, failures)."""
    ref = R.seq_mse_backward_ref(z, w, dres, loss_cnt[1], grad_out)
    runs = [(True, _backward(lib, c, dz, dw, dres, loss_cnt, grad_out, True))]
    if c["plan"][0] > 1:
        runs.append((False, _backward(lib, c, dz, dw, dres, loss_cnt, grad_out, False)))
        bit_equal(runs[0][1]["dz"], runs[1][1]["dz"], what + ": dz differs between the two paths")
    bad = []
    for with_scratch, got in runs:
        fam = "decoder_bwd" if with_scratch else "decoder_bwd_noscratch"
        for k in ("dz", "dw", "db"):
            bad += sum_crit(fam, k, got[k], ref[k][0], ref[k][1], f"{what} scratch={with_scratch}")
    return runs[0][1], bad


@pytest.mark.parametrize("c", R.DECODER_CASES, ids=lambda c: c["id"])
def test_seq_mse_forward_then_backward(lib, c):
    B, T, Z, D = c["B"], c["T"], c["Z"], c["D"]
    z, w, b, x = R.build_decoder(c)
    dz, dw, db, dx = dev(z), dev(w), dev(b), dev(x)
    bad = []
    for pat in R.decoder_runs(c):
        what = f"{c['id']} {pat}"
        ln = R.build_lengths(c, pat)
        dl = None if ln is None else dev(ln)
        ref = R.seq_mse_ref(z, w, b, x, ln, R.GRAD_OUT)
        f = _forward(lib, c, dz, dw, db, dx, dl, True)
        f0 = _forward(lib, c, dz, dw, db, dx, dl, False)       # recon == NULL
        for k in ("dres", "row_partial", "loss_cnt"):
            bit_equal(f[k], f0[k], f"{what}: {k} differs with recon == NULL")
        # recon: a single sum of products
        bad += sum_crit("decoder_fwd", "recon", f["recon"], ref["recon"], ref["S_recon"], what)
        # dres: tied to the kernel's own recon, +0 on dead positions
        live = ref["live"]
        xt = np.concatenate([x[:, 1:], x[:, -1:]], 1) if T > 1 else x
        tie = np.where(live[..., None], f["recon"] - xt, F32(0)).astype(F32)
        bit_equal(f["dres"], tie, what + ": dres is not float32(recon) - float32(x_target) / +0")
        assert not f["dres"][~live].view(np.uint32).any(), what + ": a dead position's dres is not +0"
        # the denominator: D * #live exactly (the + 1e-8 is absorbed), 1e-8 with no live position
        cnt = F32(D * int(live.sum()))
        masked = ln is not None and T > 1
        want = F32(cnt + F32(1e-8)) if masked else cnt
        assert want == (cnt if cnt >= 1 else F32(1e-8))
        bit_equal(f["loss_cnt"][1], want, what + ": denominator")
        assert float(want) == float(F32(ref["denominator"]))
        # the sums of non-negative terms, each from the kernel's own terms
        bad += nonneg_crit("decoder_fwd", "row_partial", f["row_partial"], (f["dres"].astype(F64) ** 2).sum(-1), what)
        bad += nonneg_crit("decoder_fwd", "loss", f["loss_cnt"][0], f["row_partial"].astype(F64).sum() / float(f["loss_cnt"][1]), what)
        # the backward on the forward's leaves: given its arguments, then end to end
        g, bad_b = _backward_both(lib, c, dz, dw, z, w, f["dres"], f["loss_cnt"], R.GRAD_OUT, what)
        bad += bad_b
        got = dict(loss=f["loss_cnt"][0], dz=g["dz"], dw=g["dw"], db=g["db"])
        bad += within("decoder", got, {k: ref[k] for k in got}, what)
        if pat == "dead":
            assert float(f["loss_cnt"][0]) == 0 and not g["dz"].any() and not g["dw"].any() and not g["db"].any(), what
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("c", R.DECODER_CASES, ids=lambda c: c["id"])
def test_seq_mse_backward_in_isolation(lib, c):
    """Hand-made leaves: a dres no forward produced (row magnitudes over 10^+-3) and an arbitrary denominator."""
    z, w, _, _ = R.build_decoder(c)
    dz, dw = dev(z), dev(w)
    dres, den = R.build_isolated(c)
    bad = []
    for g in R.ISOLATED_GRADS:
        got, bad_b = _backward_both(lib, c, dz, dw, z, w, dres, np.array([0.25, den], F32), g, f"{c['id']} isolated g={g}")
        bad += bad_b
        if g == 0:
            assert not got["dz"].any() and not got["dw"].any() and not got["db"].any()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------- #
# InfoNCE
# ---------------------------------------------------------------------------------------------------------------------------- #
def _infonce_forward(lib, pred, target, n, D, temp):
    ph, th, pn = sentinel(n * D, D), sentinel(n * D, D), sentinel(n)
    probs, rl, loss = sentinel(n * n, n), sentinel(n), sentinel(1)
    _ok(lib, lib.umlh_infonce_forward(vp(dev(pred)), vp(dev(target)), n, D, C.c_float(temp), vp(ph), vp(th), vp(pn), vp(probs), vp(rl),
                                      vp(loss), None), "infonce_forward")
    return dict(pred_hat=written(ph, n * D, "pred_hat").reshape(n, D), target_hat=written(th, n * D, "target_hat").reshape(n, D),
                pred_norm=written(pn, n, "pred_norm"), probs=written(probs, n * n, "probs").reshape(n, n),
                row_loss=written(rl, n, "row_loss"), loss=written(loss, 1, "loss")[0])


def _infonce_backward(lib, ph, th, pn, probs, grad_out, n, D, temp):
    dhat, dpred = sentinel(n * D, D), sentinel(n * D, D)
    _ok(lib, lib.umlh_infonce_backward(vp(dev(ph)), vp(dev(th)), vp(dev(pn)), vp(dev(probs)), vp(dev(np.array([grad_out], F32))), n, D,
                                       C.c_float(temp), vp(dhat), vp(dpred), None), "infonce_backward")
    return dict(dhat=written(dhat, n * D, "dhat").reshape(n, D), dpred=written(dpred, n * D, "dpred").reshape(n, D))


@pytest.mark.parametrize("c", R.INFONCE_CASES, ids=R.infonce_id)
def test_infonce_forward_then_backward(lib, c):
    n, D, temp, kind = c
    fam, what = R.infonce_family(c), R.infonce_id(c)
    pred, target = R.build_infonce(c)
    ref = R.infonce_ref(pred, target, temp, R.GRAD_OUT)
    f = _infonce_forward(lib, pred, target, n, D, temp)
    swapped = _infonce_forward(lib, target, pred, n, D, temp)    # the target norms are no output: the same kernel on target
    bit_equal(swapped["pred_hat"], f["target_hat"], what + ": target_hat differs from pred_hat of the swapped call")
    tn = swapped["pred_norm"]
    bad = nonneg_crit(fam, "pred_norm", f["pred_norm"], ref["pred_norm"], what)
    bad += nonneg_crit(fam, "target_norm", tn, ref["target_norm"], what)
    # unit rows: one IEEE fp32 division by the kernel's own norm
    bit_equal(f["pred_hat"], pred / f["pred_norm"][:, None], what + ": pred_hat is not x / norm")
    bit_equal(f["target_hat"], target / tn[:, None], what + ": target_hat is not x / norm")
    # backward on the forward's leaves, end to end.  dhat on these leaves is recorded, not held to the GEMM criterion: a row of
    # softmax - I is one term near -1 followed by hundreds of small positive ones, and a k-ordered fp32 chain -- the form the
    # criterion is calibrated on -- reaches 2^-19.0 rms on them at n = 257 (tests/test_critic_ref_cpu.py emulates it).  The
    # criterion is asserted on arbitrary leaves below.
    b = _infonce_backward(lib, f["pred_hat"], f["target_hat"], f["pred_norm"], f["probs"], R.GRAD_OUT, n, D, temp)
    lref = R.infonce_backward_ref(f["pred_hat"], f["target_hat"], f["pred_norm"], f["probs"], R.GRAD_OUT, temp)
    sum_crit(fam, "dhat_forward_leaves", b["dhat"], lref["dhat"], lref["S_dhat"], what)
    got = dict(probs=f["probs"], row_loss=f["row_loss"], loss=f["loss"], dpred=b["dpred"])
    bad += within(fam, got, {k: ref[k] for k in got}, what)
    row = R.special_row(c)
    if kind == "tiny_row":
        # the documented form c * (dy - y (y . dy)) / norm on the row of norm 1e-15 (it dominates the tensor's scale; torch's form
        # differs from it by |y|^2 = 1e-6 of the row, below what fp32 resolves here: the CPU test states that difference)
        e = R.comp_err(b["dpred"][row], ref["dpred"][row])
        note(fam, "dpred_tiny_row", e)
        assert e <= R.BOUNDS[fam]["dpred"], what
        assert float(f["pred_norm"][row]) == float(F32(1e-12))
    if kind == "zero_row":
        assert not f["pred_hat"][row].any() and float(f["pred_norm"][row]) == float(F32(1e-12))
    if n == 1:
        assert float(f["loss"]) == 0 and not f["probs"].any() and not b["dpred"].any(), what
    zero = _infonce_backward(lib, f["pred_hat"], f["target_hat"], f["pred_norm"], f["probs"], 0.0, n, D, temp)
    assert not zero["dpred"].any(), what + ": grad_out == 0"
    # backward on arbitrary leaves
    ph, th, pn, pr = R.build_leaves(c)
    a = _infonce_backward(lib, ph, th, pn, pr, R.GRAD_OUT, n, D, temp)
    aref = R.infonce_backward_ref(ph, th, pn, pr, R.GRAD_OUT, temp)
    bad += sum_crit("leaves", "dhat", a["dhat"], aref["dhat"], aref["S_dhat"], what + " leaves")
    bad += within("leaves", a, dict(dpred=aref["dpred"]), what + " leaves")
    assert not bad, "\n".join(bad)


def test_zz_print_levels():
    """The measured GPU levels (log2) per family and output, one line."""
    lg = lambda v: round(float(np.log2(v)), 1) if v > 0 else None
    print("\nCRITIC_LEVELS", json.dumps({f: {k: lg(v) for k, v in sorted(d.items())} for f, d in sorted(LEVELS.items())}))
    assert CRIT_MAX == 2.0 ** -20 and CRIT_RMS == 2.0 ** -23
