"""GPU: the standalone optimizer entry points (umlh_optimizer_step, umlh_optimizer_step_multi) and umlh_to_bf16 called through
ctypes against the float64 contract of tests/_optstep_ref.py: p, m and v in fp32 ulps under the CPU-calibrated bounds of that
module, v untouched under SGD, nothing written behind element n, no block of the multi-tensor kernel on the wrong tensor.  No
tolerance is chosen here.  Run with -s to see the OPTSTEP_LEVELS line (profiles/critic_accuracy.txt)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _optstep_ref as O
from _gemm_ref import SENTINEL_BITS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
LEVELS = {}
SENT = np.uint32(SENTINEL_BITS)
GAP = 8                                                       # sentinel floats between two tensors of a carved allocation


@pytest.fixture(scope="module")
def lib():
    import umlh
    return umlh.load_library()


def _ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.umlh_last_error())


def sentinel(n):
    return torch.full((n,), SENTINEL_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def note(fam, key, err):
    LEVELS.setdefault(fam, {})[key] = max(LEVELS.get(fam, {}).get(key, 0.0), float(err))


def _hyper(step, wd):
    return (C.c_double(O.LR), step, C.c_double(O.BETAS[0]), C.c_double(O.BETAS[1]), C.c_double(O.EPS), C.c_double(O.MOMENTUM),
            C.c_double(wd))


def _check(fam, kind, got, data, wd, step, what):
    """p, m (and v) under the kind's bounds against float64; returns the failures."""
    bad = []
    for o, e in O.errors_against_ref(kind, got, data, wd, step).items():
        note(fam, f"{kind}_{o}", e)
        if not e <= O.BOUNDS[kind][o]:
            bad.append(f"{what} {o}: {e:.1f} ulps > {O.BOUNDS[kind][o]:.0f}")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------- #
# umlh_optimizer_step
# ---------------------------------------------------------------------------------------------------------------------------- #
def _single(lib, kind, data, wd, step, v_mode, offset=0):
    """One call on buffers whose element 0 sits `offset` floats past a 16-byte boundary, with 64 sentinel floats behind element n.
    v_mode: 'buffer', 'null'.  Returns (p, m, v) as numpy (v: the buffer's first n floats, whatever the kernel did with them)."""
    p, g, m, v = data
    n = p.size
    bufs = []
    for a in (p, g, m, v):
        b = sentinel(offset + n + 64)
        assert b.data_ptr() % 16 == 0
        b[offset:offset + n] = torch.from_numpy(a).to(DEV)
        bufs.append(b)
    if kind == "sgd":
        bufs[3] = sentinel(offset + n + 64)                   # a sentinel v: SGD must leave it alone
    ptr = lambda b: C.c_void_p(b.data_ptr() + 4 * offset)
    vptr = None if v_mode == "null" else ptr(bufs[3])
    _ok(lib, lib.umlh_optimizer_step(O.OPT_ID[kind], ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), vptr, n, *_hyper(step, wd), None),
        f"optimizer_step {kind} n={n}")
    torch.cuda.synchronize()
    out = [b.cpu().numpy() for b in bufs]
    for name, a in zip("pgmv", out):
        bits = a.view(np.uint32)
        assert (bits[:offset] == SENT).all() and (bits[offset + n:] == SENT).all(), f"{kind} n={n}: {name} written outside [0, n)"
    assert np.array_equal(out[1][offset:offset + n].view(np.uint32), g.view(np.uint32)), "the gradient was modified"
    if kind == "sgd":
        assert (out[3].view(np.uint32) == SENT).all(), "SGD touched v"
    return out[0][offset:offset + n], out[2][offset:offset + n], out[3][offset:offset + n]


@pytest.mark.parametrize("kind", O.KINDS)
def test_optimizer_step_lengths_steps_and_decay(lib, kind):
    bad = []
    for i, n in enumerate(O.SINGLE_N):
        data = O.build_data(n, 0)
        # every length under one (wd, step) in turn; the longest under all of them
        for wd, step in (O.settings() if n == O.SINGLE_N[-1] else [O.settings()[i % len(O.settings())]]):
            got = _single(lib, kind, data, wd, step, "buffer")
            bad += _check("single", kind, got, data, wd, step, f"{kind} n={n} wd={wd} step={step}")
            if kind == "sgd":                                 # v == NULL: the same bits
                nul = _single(lib, kind, data, wd, step, "null")
                assert np.array_equal(nul[0].view(np.uint32), got[0].view(np.uint32)) and np.array_equal(nul[1].view(np.uint32), got[1].view(np.uint32))
    # step < 1 is step 1, bit for bit
    data = O.build_data(1025, 1)
    a, b = _single(lib, kind, data, 0.1, 0, "buffer"), _single(lib, kind, data, 0.1, 1, "buffer")
    c = _single(lib, kind, data, 0.1, -5, "buffer")
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and np.array_equal(x.view(np.uint32), z.view(np.uint32))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", O.KINDS)
def test_optimizer_step_base_off_a_16_byte_boundary(lib, kind):
    """param, grad, m and v four bytes past a 16-byte boundary: the entry point's host code sends the call to the element-wise
    kernel (include/umlh.h), so the float4 path never sees the base.  Same contract, same bounds."""
    bad = []
    for n in (1, 5, 1024, 1025, 4099):
        data = O.build_data(n, 2)
        got = _single(lib, kind, data, 0.1, 2, "buffer", offset=1)
        bad += _check("single_unaligned", kind, got, data, 0.1, 2, f"{kind} n={n} offset 1")
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------- #
# umlh_optimizer_step_multi
# ---------------------------------------------------------------------------------------------------------------------------- #
def _carve(counts):
    """Offsets of the tensors in one allocation: each starts on a 16-byte boundary, GAP sentinel floats before, between, behind."""
    offs, o = [], GAP
    for n in counts:
        offs.append(o)
        o = -(-(o + n + GAP) // 4) * 4
    return offs, o + GAP


def _multi_data(counts, seed):
    """Per tensor (p, g, m, v): p encodes (tensor, element); g, m, v as build_data's."""
    out = []
    for t, n in enumerate(counts):
        _, g, m, v = O.build_data(n, seed + 1000 * t, "multi")
        out.append((O.encode_p(t, n), g, m, v))
    return out


def _multi(lib, kind, counts, data, wd, step, v_null=False):
    offs, total = _carve(counts)
    host = [np.full(total, SENT, np.uint32).view(F32) for _ in range(4)]
    for (o, n, d) in zip(offs, counts, data):
        for h, a in zip(host, d):
            h[o:o + n] = a
    if kind == "sgd":
        host[3][:] = np.full(total, SENT, np.uint32).view(F32)
    bufs = [torch.from_numpy(h.copy()).to(DEV) for h in host]
    k = len(counts)
    arr = lambda b: (C.c_void_p * k)(*[b.data_ptr() + 4 * o for o in offs])
    cnt = (C.c_int64 * k)(*counts)
    _ok(lib, lib.umlh_optimizer_step_multi(O.OPT_ID[kind], k, arr(bufs[0]), arr(bufs[1]), arr(bufs[2]), None if v_null else arr(bufs[3]),
                                           cnt, *_hyper(step, wd), None), f"optimizer_step_multi {kind} {k} tensors")
    torch.cuda.synchronize()
    out = [b.cpu().numpy() for b in bufs]
    inside = np.zeros(total, bool)
    for o, n in zip(offs, counts):
        inside[o:o + n] = True
    for name, a in zip("pgmv", out):
        assert (a.view(np.uint32)[~inside] == SENT).all(), f"{kind} {k} tensors: {name} written in a gap between tensors"
    assert np.array_equal(out[1].view(np.uint32), host[1].view(np.uint32)), "a gradient was modified"
    if kind == "sgd":
        assert (out[3].view(np.uint32) == SENT).all(), "SGD touched v"
    return [(out[0][o:o + n], out[2][o:o + n], out[3][o:o + n]) for o, n in zip(offs, counts)]


@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("name", list(O.multi_lists()))
def test_optimizer_step_multi(lib, kind, name):
    counts = O.multi_lists()[name]
    wd, step = O.settings()[(len(counts) + O.KINDS.index(kind)) % len(O.settings())]
    data = _multi_data(counts, 7)
    got = _multi(lib, kind, counts, data, wd, step)
    bad, agree = [], True
    for t, (n, d, g) in enumerate(zip(counts, data, got)):
        bad += _check("multi", kind, g, d, wd, step, f"{kind} {name} tensor {t} (n={n}) wd={wd} step={step}")
        if n and name.startswith("tensors_") and t % 16 == 5:
            # the single-tensor entry point on the same data: recorded, not asserted
            one = _single(lib, kind, d, wd, step, "buffer")
            agree &= all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(one[:2 if kind == "sgd" else 3], g))
    if name.startswith("tensors_"):
        LEVELS.setdefault("entry_points_bit_equal", {}).setdefault(kind, True)
        LEVELS["entry_points_bit_equal"][kind] &= agree
    if kind == "sgd" and name in ("empty_between", "tensors_49"):
        nul = _multi(lib, kind, counts, data, wd, step, v_null=True)
        for a, b in zip(nul, got):
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert not bad, "\n".join(bad[:20])


# ---------------------------------------------------------------------------------------------------------------------------- #
# umlh_to_bf16
# ---------------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("n", O.BF16_N)
def test_to_bf16_is_torch_round_to_nearest_even(lib, n):
    x = O.build_bf16_input(n)
    src = torch.from_numpy(x.copy()).to(DEV) if n else torch.zeros(8, device=DEV)
    dst = torch.full((n + 16,), 0x5A5A, dtype=torch.int16, device=DEV)
    _ok(lib, lib.umlh_to_bf16(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), n, None), "to_bf16")
    torch.cuda.synchronize()
    got = dst.cpu().numpy().view(np.uint16)
    assert (got[n:] == 0x5A5A).all(), "written behind element n"
    ref = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    is_nan16 = ((got[:n] & 0x7F80) == 0x7F80) & ((got[:n] & 0x007F) != 0)
    assert is_nan16[nan].all() and not is_nan16[~nan].any(), "a NaN must stay a NaN, and only a NaN"
    assert np.array_equal(got[:n][~nan], ref[~nan])


def test_zz_print_levels():
    """The measured GPU levels in ulps per entry point, kind and output, one line."""
    out = {f: ({k: round(v, 2) for k, v in sorted(d.items())} if f != "entry_points_bit_equal" else d) for f, d in sorted(LEVELS.items())}
    print("\nOPTSTEP_LEVELS", json.dumps(out))
