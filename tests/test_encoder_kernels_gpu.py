"""GPU: every encoder entry point of include/umlh.h called on its own through ctypes, in eval and in train mode, against the
float64 contract of tests/_encoder_ref.py: the elementwise ops bit for bit, the column sums under the GEMM criterion, LayerNorm,
attention, one layer, the stack and the plan under the CPU-calibrated bounds of that module.  No tolerance is chosen here.

Every output buffer is filled with a NaN sentinel and is one row longer than the call needs: all of the output must be written
and nothing behind it.  Dropout masks are what umlh_dropout leaves of a tensor of ones, and are checked against the hash restated
in _encoder_ref.keep_mask each time one is drawn.  Run with -s to see the ENC_LEVELS line (profiles/encoder_accuracy.txt)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _encoder_ref as R
from _gemm_ref import CRIT_MAX, CRIT_RMS, SENTINEL_BITS, gemm_err, meets_criterion, spread_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
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
    """A device input made by dev() lives until its test ends: a temporary passed as `vp(dev(x))` would go back to torch's
    caching allocator before the launch and the next upload could land on it."""
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def dev(a):
    _ALIVE.append(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))
    return _ALIVE[-1]


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


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
    """Bit for bit; a NaN of the reference must be a NaN (any payload)."""
    got, ref = np.asarray(got, F32).ravel(), np.asarray(ref, F32).ravel()
    nan = np.isnan(ref)
    assert np.isnan(got[nan]).all(), what
    assert np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32)), what


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
    e = gemm_err(got, ref, S)
    note(fam, key + "_max", e[0])
    note(fam, key + "_rms", e[1])
    return [] if meets_criterion(e) else [f"{what} {key}: max 2^{np.log2(e[0]):.1f} rms 2^{np.log2(e[1]):.1f}"]


def make_mask_fn(lib):
    def gpu_mask(seed, n, p):
        x = torch.ones(n, device=DEV)
        _ok(lib, lib.umlh_dropout(vp(x), n, C.c_float(p), seed, None), "dropout")
        torch.cuda.synchronize()
        m = x.cpu().numpy() != 0
        assert np.array_equal(m, R.keep_mask(seed, n, p)), "umlh_dropout on ones differs from _encoder_ref.keep_mask"
        return m
    return gpu_mask


def special_values(rng, n):
    """Standard normal fp32 with 0, -0.0 and NaN planted."""
    x = rng.standard_normal(n).astype(F32)
    for i, v in zip(rng.choice(n, min(n, 6), replace=False), (0.0, -0.0, np.nan, -0.0, np.nan, 0.0)):
        x[i] = v
    return x


# ---------------------------------------------------------------------------------------------------------------------------- #
# elementwise ops: bit-equal to numpy float32
# ---------------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("n", R.ELEMENT_COUNTS)
def test_bias_act(lib, n):
    rng = np.random.default_rng(n)
    for N in (1, 7, 64):
        M = -(-n // N)
        for with_bias in (False, True):
            for relu in (0, 1):
                y = special_values(rng, M * N).reshape(M, N)
                b = rng.standard_normal(N).astype(F32) if with_bias else None
                buf = sentinel(M * N)
                buf[:M * N] = dev(y.ravel())
                db = dev(b) if with_bias else None
                _ok(lib, lib.umlh_bias_act(vp(buf), vp(db), M, N, relu, None), "bias_act")
                torch.cuda.synchronize()
                a = buf.cpu().numpy()
                assert (a.view(np.uint32)[M * N:] == np.uint32(SENTINEL_BITS)).all()
                bit_equal(a[:M * N], R.bias_act_ref(y, b, relu), (n, N, with_bias, relu))


@pytest.mark.parametrize("n", R.ELEMENT_COUNTS)
def test_relu_backward_and_add_inplace(lib, n):
    rng = np.random.default_rng(n + 1)
    y, dy = special_values(rng, n), rng.standard_normal(n).astype(F32)
    buf = sentinel(n)
    buf[:n] = dev(dy)
    _ok(lib, lib.umlh_relu_backward(vp(dev(y)), vp(buf), n, None), "relu_backward")
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a.view(np.uint32)[n:] == np.uint32(SENTINEL_BITS)).all()
    bit_equal(a[:n], R.relu_backward_ref(y, dy), "relu_backward")
    assert not a[:n][~(y > 0)].any()                           # zeroed wherever !(y > 0): 0, -0.0, NaN, negatives
    x = rng.standard_normal(n).astype(F32)
    buf = sentinel(n)
    buf[:n] = dev(dy)
    _ok(lib, lib.umlh_add_inplace(vp(buf), vp(dev(x)), n, None), "add_inplace")
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a.view(np.uint32)[n:] == np.uint32(SENTINEL_BITS)).all()
    bit_equal(a[:n], dy + x, "add_inplace")


@pytest.mark.parametrize("T,B,Z", R.POS_SHAPES)
def test_add_positions(lib, T, B, Z):
    rng = np.random.default_rng(T * 100 + Z)
    x, pos = rng.standard_normal(T * B * Z).astype(F32), rng.standard_normal(T * Z).astype(F32)
    buf = sentinel(T * B * Z, Z)
    buf[:T * B * Z] = dev(x)
    _ok(lib, lib.umlh_add_positions(vp(buf), vp(dev(pos)), T, B, Z, None), "add_positions")
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a.view(np.uint32)[T * B * Z:] == np.uint32(SENTINEL_BITS)).all()
    bit_equal(a[:T * B * Z], R.add_positions_ref(x, pos, T, B, Z), "add_positions")


@pytest.mark.parametrize("n,Z,rows", [(37, 7, 50), (300, 65, 333), (1, 1, 1)])
def test_gather_rows(lib, n, Z, rows):
    assert (n * Z) % 256 != 0
    rng = np.random.default_rng(n)
    x = rng.standard_normal((rows, Z)).astype(F32)
    idx = rng.integers(0, rows, n).astype(np.int64)             # with repeats
    if n > 2:
        idx[1] = idx[0]
    out = sentinel(n * Z, Z)
    _ok(lib, lib.umlh_gather_rows(vp(dev(x)), vp(dev(idx)), n, Z, vp(out), 0, None), "gather")
    bit_equal(written(out, n * Z, "gather"), R.gather_rows_ref(x, idx, n, False), "gather")
    # scatter: a permutation of the first n of `rows` output rows into a zeroed buffer
    perm = rng.permutation(rows)[:n].astype(np.int64)
    src = rng.standard_normal((n, Z)).astype(F32)
    out = sentinel(rows * Z, Z)
    out[:rows * Z] = 0
    _ok(lib, lib.umlh_gather_rows(vp(dev(src)), vp(dev(perm)), n, Z, vp(out), 1, None), "scatter")
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert (a.view(np.uint32)[rows * Z:] == np.uint32(SENTINEL_BITS)).all()
    bit_equal(a[:rows * Z], R.gather_rows_ref(src, perm, rows, True), "scatter")


# ---------------------------------------------------------------------------------------------------------------------------- #
# umlh_dropout
# ---------------------------------------------------------------------------------------------------------------------------- #
def _dropout(lib, x, p, seed):
    n = x.size
    buf = sentinel(n)
    buf[:n] = dev(x)
    _ok(lib, lib.umlh_dropout(vp(buf), n, C.c_float(p), seed, None), "dropout")
    torch.cuda.synchronize()
    a = buf.cpu().numpy()
    assert (a.view(np.uint32)[n:] == np.uint32(SENTINEL_BITS)).all()
    return a[:n].copy()


def test_dropout_values_prefix_and_noop(lib):
    rng = np.random.default_rng(3)
    x = rng.standard_normal(5000).astype(F32)
    for p in (0.1, 0.5, 0.3):
        got = _dropout(lib, x, p, 4242)
        keep = got != 0
        scaled = (x * R.inv_keep(p, F32)).astype(F32)
        bit_equal(got, np.where(keep, scaled, F32(0)), p)        # x * float32(1 / (1 - p)) or 0
        assert np.array_equal(keep, R.keep_mask(4242, 5000, p))
        assert np.array_equal(_dropout(lib, x[:1000], p, 4242) != 0, keep[:1000])      # the mask of a prefix is the prefix
    bit_equal(_dropout(lib, x, 0.0, 4242), x, "p = 0 leaves the buffer untouched")


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_rate_and_independent_streams(lib, p):
    n, seed = 1 << 20, 991
    ones = np.ones(n, F32)
    q = 1.0 - float(F32(p))
    masks = {k: _dropout(lib, ones, p, seed + k) != 0 for k in (0, 1, 2, 3, R.STACK_SEED_STRIDE)}
    for k, m in masks.items():
        assert abs(m.mean() - q) <= 5 * np.sqrt(q * (1 - q) / n), (k, m.mean())
    a = q * q + (1 - q) ** 2                                    # two independent masks agree with this probability
    ks = list(masks)
    for i in range(len(ks)):
        for j in range(i + 1, len(ks)):
            agree = (masks[ks[i]] == masks[ks[j]]).mean()
            assert agree < 1.0 and abs(agree - a) <= 5 * np.sqrt(a * (1 - a) / n), (ks[i], ks[j], agree)


# ---------------------------------------------------------------------------------------------------------------------------- #
# column sums against float64 (the GEMM criterion)
# ---------------------------------------------------------------------------------------------------------------------------- #
def test_colsum(lib):
    bad = []
    for M in R.COLSUM_M:
        for N in R.COLSUM_N:
            x = spread_rows(np.random.default_rng(M * 1000 + N), M, N)
            out = sentinel(N, N)
            _ok(lib, lib.umlh_colsum(vp(dev(x)), M, N, vp(out), None), "colsum")
            ref, S = R.colsum_ref(x)
            bad += sum_crit("colsum", "out", written(out, N, "colsum"), ref, S, f"colsum {M}x{N}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("T,B,Z", R.POS_GRAD_SHAPES)
def test_positions_backward(lib, T, B, Z):
    dx = spread_rows(np.random.default_rng(T + B + Z), T * B, Z)
    out = sentinel(T * Z, Z)
    _ok(lib, lib.umlh_positions_backward(vp(dev(dx)), T, B, Z, vp(out), None), "positions_backward")
    ref, S = R.positions_backward_ref(dx, T, B, Z)
    bad = sum_crit("positions_backward", "dpos", written(out, T * Z, "dpos").reshape(T, Z), ref, S, f"{T},{B},{Z}")
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------- #
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("with_r", [False, True])
def test_layernorm_forward_backward(lib, with_r):
    bad = []
    for M, N, scale in R.LN_CASES:
        what = f"layernorm {M}x{N} scale {scale} r={with_r}"
        x, r, gamma, beta, dy = R.build_layernorm(M, N, scale)
        s, y, mean, rstd = sentinel(M * N, N), sentinel(M * N, N), sentinel(M), sentinel(M)
        dg, dbt = dev(gamma), dev(beta)
        _ok(lib, lib.umlh_add_layernorm_forward(vp(dev(x)), vp(dev(r)) if with_r else None, vp(dg), vp(dbt), M, N, C.c_float(R.EPS),
                                                vp(s), vp(y), vp(mean), vp(rstd), None), what)
        got = dict(y=written(y, M * N, what).reshape(M, N), mean=written(mean, M, what), rstd=written(rstd, M, what))
        bit_equal(written(s, M * N, what), (x + r) if with_r else x, what + ": s is x + r")
        ref, sums = R.layernorm_eval(M, N, scale, with_r, 0)
        if N == 1:
            bit_equal(got["y"], np.broadcast_to(beta, (M, N)), what + ": zero variance, y is beta")
        bad += within("layernorm", got, {k: ref[k] for k in got}, what)
        # backward on the float64 forward's s / mean / rstd rounded to fp32 (layernorm_eval's inputs)
        s64, _, mean64, rstd64 = R.layernorm_ref(x, r if with_r else None, gamma, beta)
        s32, mean32, rstd32 = s64.astype(F32), mean64.astype(F32), rstd64.astype(F32)
        ds, dgam, dbet = sentinel(M * N, N), sentinel(N, N), sentinel(N, N)
        _ok(lib, lib.umlh_layernorm_backward(vp(dev(dy)), vp(dev(s32)), vp(dg), vp(dev(mean32)), vp(dev(rstd32)), M, N, vp(ds), vp(dgam),
                                             vp(dbet), None), what)
        bad += within("layernorm", dict(ds=written(ds, M * N, what).reshape(M, N)), dict(ds=ref["ds"]), what)
        bad += sum_crit("layernorm", "dgamma", written(dgam, N, what), sums["dgamma"][0], sums["dgamma"][1], what)
        bad += sum_crit("layernorm", "dbeta", written(dbet, N, what), sums["dbeta"][0], sums["dbeta"][1], what)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("with_r", [False, True])
def test_layernorm_forward_signed_zeros(lib, with_r):
    """s = x + r keeps IEEE signed zeros: -0 + -0 is -0, every other pairing of zeros is +0, and without r it is x + (+0), so a
    -0 of x comes out as +0.  (A sum that starts from +0, as the slab form's does, would lose the first.)  5 rows: a second block
    of 4; 65 columns: lane 0 takes a second column."""
    M, N = 5, 65
    rng = np.random.default_rng(565)
    x, r = rng.standard_normal((M, N)).astype(F32), rng.standard_normal((M, N)).astype(F32)
    gamma, beta = rng.standard_normal(N).astype(F32), rng.standard_normal(N).astype(F32)
    nz, pz = F32(-0.0), F32(0.0)
    planted = {(0, 0): (nz, nz), (0, 1): (nz, pz), (1, 63): (pz, nz), (1, 64): (pz, pz), (4, 64): (nz, nz), (4, 0): (pz, nz),
               (2, 5): (nz, None), (3, 7): (None, nz), (4, 33): (nz, pz)}       # (x, r) at (m, n); None: the random value stays
    for (m, n), (vx, vr) in planted.items():
        if vx is not None:
            x[m, n] = vx
        if vr is not None:
            r[m, n] = vr
    ref = (x + r) if with_r else (x + F32(0))
    assert ref.dtype == F32
    for (m, n), (vx, vr) in planted.items():                                    # numpy's own bits for the planted pairs
        if vx is not None and (vr is not None or not with_r):
            both_neg = with_r and np.signbit(vx) and np.signbit(vr)
            assert ref[m, n] == 0 and bool(np.signbit(ref[m, n])) == bool(both_neg), (m, n)
    s, y, mean, rstd = sentinel(M * N, N), sentinel(M * N, N), sentinel(M), sentinel(M)
    _ok(lib, lib.umlh_add_layernorm_forward(vp(dev(x)), vp(dev(r)) if with_r else None, vp(dev(gamma)), vp(dev(beta)), M, N,
                                            C.c_float(R.EPS), vp(s), vp(y), vp(mean), vp(rstd), None), "add_layernorm_forward")
    got = written(s, M * N, "s")
    assert np.array_equal(got.view(np.uint32), ref.ravel().view(np.uint32)), "s differs from numpy's fp32 sum in some bit"
    written(y, M * N, "y"), written(mean, M, "mean"), written(rstd, M, "rstd")


# ---------------------------------------------------------------------------------------------------------------------------- #
# attention
# ---------------------------------------------------------------------------------------------------------------------------- #
def _attention(lib, qkv, dctx, lengths, T, B, Z, H, p, seed):
    """ctx [T,B,Z], lse [B,H,T], dqkv [T,B,3Z] of the two entry points."""
    dq, dl = dev(qkv), None if lengths is None else dev(np.asarray(lengths, np.int64))
    ctx, lse, dqkv = sentinel(T * B * Z, Z), sentinel(B * H * T, T), sentinel(T * B * 3 * Z, 3 * Z)
    _ok(lib, lib.umlh_attention_forward(vp(dq), vp(dl), T, B, Z, H, C.c_float(p), seed, vp(ctx), vp(lse), None), "attention_forward")
    got_lse = written(lse, B * H * T, "lse")
    dlse = dev(got_lse)
    _ok(lib, lib.umlh_attention_backward(vp(dq), vp(dl), vp(dlse), vp(dev(dctx)), T, B, Z, H, C.c_float(p), seed, vp(dqkv), None),
        "attention_backward")
    return dict(ctx=written(ctx, T * B * Z, "ctx").reshape(T, B, Z), lse=got_lse.reshape(B, H, T),
                dqkv=written(dqkv, T * B * 3 * Z, "dqkv").reshape(T, B, 3 * Z))


@pytest.mark.parametrize("c", R.ATT_CASES, ids=lambda c: c["id"])
def test_attention(lib, c):
    T, B, Z, H = c["T"], c["B"], c["Z"], c["H"]
    qkv, dctx = R.build_attention(c)
    bad = []
    for p in R.runs_of(c):
        got = _attention(lib, qkv, dctx, c["lengths"], T, B, Z, H, p, c["seed"])
        ref = R.attention_eval(c, p, 0, mask_fn=make_mask_fn(lib))
        bad += within(R.att_family(c), got, ref, f"{c['id']} p={p}")
        g, r = got["dqkv"].reshape(T, B, 3, Z), ref["dqkv"].reshape(T, B, 3, Z)
        for i, third in enumerate(("dq", "dk", "dv")):          # the thirds on the tensor's scale, for the record
            note(R.att_family(c), third, np.abs(g[:, :, i] - r[:, :, i]).max() / np.abs(r).max())
        for b, ln in enumerate(c["lengths"] or []):
            assert not g[ln:, b, 1:].any(), f"{c['id']} p={p}: dk / dv of a padded key is not exactly 0"
    assert not bad, "\n".join(bad)


def test_attention_mask_probe(lib):
    """V[j, :] = e_j makes ctx[t, b, h*dh + j] the dropped probability of (t, j): the mask convention read off the kernel."""
    c = R.MASK_PROBE
    T, B, Z, H, p = c["T"], c["B"], c["Z"], c["H"], c["p"]
    dh = Z // H
    assert dh >= T
    qkv, dctx = R.build_attention(c)
    v = np.zeros((T, B, H, dh), F32)
    v[np.arange(T), :, :, np.arange(T)] = 1.0
    qkv[..., 2 * Z:] = v.reshape(T, B, Z)
    got = _attention(lib, qkv, dctx, c["lengths"], T, B, Z, H, p, c["seed"])
    keep = make_mask_fn(lib)(c["seed"], B * H * T * T, p).reshape(B, H, T, T)        # element ((b*H + h)*T + t)*T + j
    live = keep & R.visible(c["lengths"], T, B)[:, None]
    probs = got["ctx"].reshape(T, B, H, dh)[..., :T].transpose(1, 2, 0, 3)           # [B,H,t,j]
    assert np.array_equal(probs != 0, live), "dropped / invisible probabilities are not exactly the zeros of ctx"
    assert not got["ctx"].reshape(T, B, H, dh)[..., T:].any()
    ref = R.attention_ref(qkv, c["lengths"], T, B, Z, H, keep, R.inv_keep(p), dctx)
    bad = within("attention", got, dict(ctx=ref[0], lse=ref[1], dqkv=ref[2]), "mask probe")
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------- #
# one layer, the stack, the plan
# ---------------------------------------------------------------------------------------------------------------------------- #
def _enc_cfg(c, p, seed):
    from umlh._lib import EncLayer
    return EncLayer(c["T"], c["B"], c["Z"], c["H"], c["d_ff"], float(p), float(c["eps"]), seed, None)


def _nan_tail(lib_fn, cfg, tail=256):
    n = int(lib_fn(C.byref(cfg)))
    assert n > 0
    return torch.full((n + tail,), float("nan"), device=DEV), n


def _grad_bufs(Z, F, n_layers=1):
    sizes = [int(np.prod(s)) for s in R.param_shapes(Z, F)] * n_layers
    return [sentinel(n) for n in sizes], sizes


def _named(h_out, dh_in, grads, n_layers=1):
    out = dict(h_out=h_out, dh_in=dh_in)
    for i, n in enumerate(R.PARAM_NAMES):
        out["d_" + n] = np.concatenate([grads[12 * li + i].ravel() for li in range(n_layers)])
    return out


def _shaped(ref):
    return {k: np.asarray(v).ravel() for k, v in ref.items()}


@pytest.mark.parametrize("c", R.LAYER_CASES, ids=lambda c: c["id"])
def test_encoder_layer(lib, c):
    T, B, Z, F = c["T"], c["B"], c["Z"], c["d_ff"]
    M = T * B
    params, h_in, dh_out = R.build_layer(c, c["seeds"][0])
    P = [dev(t) for t in params]
    dl = None if c["lengths"] is None else dev(np.asarray(c["lengths"], np.int64))
    dh_in_d, ddh = dev(h_in), dev(dh_out)
    bad = []
    for p in R.runs_of(c):
        cfg = _enc_cfg(c, p, c["seed"])
        saved, n_saved = _nan_tail(lib.umlh_encoder_layer_saved_floats, cfg)
        scratch, n_scr = _nan_tail(lib.umlh_encoder_layer_scratch_floats, cfg)
        h_out, dh_in = sentinel(M * Z, Z), sentinel(M * Z, Z)
        G, sizes = _grad_bufs(Z, F)
        _ok(lib, lib.umlh_encoder_layer_forward(C.byref(cfg), ptrs(P), vp(dh_in_d), vp(dl), vp(saved), vp(scratch), vp(h_out), None),
            "layer_forward")
        _ok(lib, lib.umlh_encoder_layer_backward(C.byref(cfg), ptrs(P), vp(dh_in_d), vp(dl), vp(saved), vp(ddh), vp(scratch), ptrs(G),
                                                 vp(dh_in), None), "layer_backward")
        what = f"{c['id']} p={p}"
        got = _named(written(h_out, M * Z, what), written(dh_in, M * Z, what), [written(g, n, what) for g, n in zip(G, sizes)])
        assert torch.isnan(saved[n_saved:]).all() and torch.isnan(scratch[n_scr:]).all(), what + ": written past saved / scratch"
        ref, fws, _ = R.layer_eval(c, p, c["seeds"][0], mask_fn=make_mask_fn(lib))
        assert R.kink_margin(fws[0], params) > R.KINK
        bad += within("layer", got, _shaped(ref), what)
    assert not bad, "\n".join(bad)


def test_encoder_stack_and_plan(lib):
    c = R.STACK_CASE
    T, B, Z, F, n, p, seed = c["T"], c["B"], c["Z"], c["d_ff"], c["n_layers"], c["p"], c["seed"]
    M = T * B
    params, h0, dh_out = R.build_layer(c, c["seeds"][0], n)
    P = [dev(t) for t in params]
    lengths = np.asarray(c["lengths"], np.int64)
    dl, dh0_in, ddh = dev(lengths), dev(h0), dev(dh_out)
    cfg = _enc_cfg(c, p, seed)
    n_saved = int(lib.umlh_encoder_layer_saved_floats(C.byref(cfg)))
    saved = torch.full((n * n_saved + 256,), float("nan"), device=DEV)
    scratch, n_scr = _nan_tail(lib.umlh_encoder_layer_scratch_floats, cfg)
    h, dh, dh0 = sentinel(n * M * Z, Z), sentinel(2 * M * Z, Z), sentinel(M * Z, Z)
    G, sizes = _grad_bufs(Z, F, n)
    _ok(lib, lib.umlh_encoder_stack_forward(C.byref(cfg), n, ptrs(P), vp(dh0_in), vp(dl), vp(saved), vp(scratch), vp(h), None), "stack_forward")
    _ok(lib, lib.umlh_encoder_stack_backward(C.byref(cfg), n, ptrs(P), vp(dh0_in), vp(dl), vp(saved), vp(h), vp(ddh), vp(scratch), ptrs(G),
                                             vp(dh), vp(dh0), None), "stack_backward")
    hs = written(h, n * M * Z, "stack h")
    got = _named(hs[(n - 1) * M * Z:], written(dh0, M * Z, "dh0"), [written(g, k, "stack grads") for g, k in zip(G, sizes)], n)
    torch.cuda.synchronize()
    assert (dh.cpu().numpy().view(np.uint32)[2 * M * Z:] == np.uint32(SENTINEL_BITS)).all()
    assert torch.isnan(saved[n * n_saved:]).all() and torch.isnan(scratch[n_scr:]).all()
    ref, fws, _ = R.layer_eval(c, p, c["seeds"][0], mask_fn=make_mask_fn(lib))       # layer 1's masks: streams seed + 7919 ..
    for li, fw in enumerate(fws):
        assert R.kink_margin(fw, params[12 * li:12 * li + 12]) > R.KINK
    bad = within("stack", got, _shaped(ref), "stack")
    assert not bad, "\n".join(bad)

    # the plan on the same parameters: eager, capture, replay -- each bit-equal to the stack call
    ws = torch.full((int(lib.umlh_encoder_plan_floats(C.byref(cfg), n)) + 256,), float("nan"), device=DEV)
    n_ws = ws.numel() - 256
    plan = C.c_void_p()
    _ok(lib, lib.umlh_encoder_plan_create(C.byref(cfg), n, ptrs(P), 1, vp(ws), C.byref(plan)), "plan_create")
    try:
        off = (C.c_uint64 * 6)()
        _ok(lib, lib.umlh_encoder_plan_offsets(plan, off), "plan_offsets")
        o_h0, o_len, o_last, o_dhout, o_dh0, o_grads = (int(v) for v in off)
        n_grads = sum(sizes)
        stack_grads = np.concatenate([written(g, k) for g, k in zip(G, sizes)])
        for call in ("eager", "capture", "replay"):
            ws[o_h0:o_h0 + M * Z] = dh0_in.ravel()
            ws[o_len:o_len + 2 * B].view(torch.int64).copy_(dl)
            ws[o_dhout:o_dhout + M * Z] = ddh.ravel()
            ws[o_last:o_last + M * Z] = float("nan")
            ws[o_dh0:o_dh0 + M * Z] = float("nan")
            ws[o_grads:o_grads + n_grads] = float("nan")
            _ok(lib, lib.umlh_encoder_plan_forward(plan, seed, None), "plan_forward " + call)
            _ok(lib, lib.umlh_encoder_plan_backward(plan, None), "plan_backward " + call)
            torch.cuda.synchronize()
            a = ws.cpu().numpy()
            bit_equal(a[o_last:o_last + M * Z], got["h_out"], call + ": h_last")
            bit_equal(a[o_dh0:o_dh0 + M * Z], got["dh_in"], call + ": dh0")
            bit_equal(a[o_grads:o_grads + n_grads], stack_grads, call + ": grads")
            assert np.isnan(a[n_ws:]).all(), call + ": written past the plan workspace"
    finally:
        torch.cuda.synchronize()
        lib.umlh_encoder_plan_destroy(plan)


def test_zz_print_levels():
    """The measured GPU levels (log2) per family and output, one line."""
    lg = lambda v: round(float(np.log2(v)), 1) if v > 0 else None
    print("\nENC_LEVELS", json.dumps({f: {k: lg(v) for k, v in sorted(d.items())} for f, d in sorted(LEVELS.items())}))
    assert CRIT_MAX == 2.0 ** -20 and CRIT_RMS == 2.0 ** -23
