"""GPU: umlh_ae_forward and umlh_ae_train_steps called through ctypes against the float64 contract of tests/_gauss_ref.py, under
the CPU-calibrated bounds of that module.  Every output and every P / M / V tensor sits between guard floats of a NaN pattern and
the scratch is one region longer than queried: everything asked for is written, nothing else is.  The gradient is read exactly
(sgd with momentum 0 leaves it in M), a real adam / adamw step is compared in ulps with opt_ref on that gradient, mode 'x' leaves
the y heads bit-unchanged, and n steps in one call equal n calls bit for bit.  No tolerance is chosen here.  Run with -s to see the
GAUSS_LEVELS line (profiles/gaussian_accuracy.txt)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import _gauss_ref as R
import _optstep_ref as O
from _gemm_ref import SENTINEL_BITS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
SENT = np.uint32(SENTINEL_BITS)
GUARD = 24                       # sentinel floats in front of, between and behind the tensors of an arena
LEVELS = {}
LR = 1e-2


@pytest.fixture(scope="module")
def lib():
    import umlh
    yield umlh.load_library()
    # per case: log2 of the worst relative error of every output; then the update's worst errors in ulps
    for cid in sorted({k[0] for k in LEVELS if isinstance(k, tuple)}):
        print("\nGAUSS_LEVELS " + cid + " " + json.dumps({k[1]: round(float(np.log2(v)), 2) if v > 0 else None
                                                          for k, v in sorted(LEVELS.items(), key=str) if isinstance(k, tuple) and k[0] == cid}))
    print("\nGAUSS_ULPS " + json.dumps({k: round(float(v), 2) for k, v in sorted(LEVELS.items(), key=str) if not isinstance(k, tuple)}))


_CASES = {}


def case_of(case, seed=0):
    """The case's data and its float64 references, computed once and shared."""
    key = (case, seed)
    if key not in _CASES:
        c = R.build_case(case, seed)
        c["ref"] = {}
        _CASES[key] = c
    return _CASES[key]


def ref_of(c, mode, indexed=True):
    key = (mode, indexed)
    if key not in c["ref"]:
        c["ref"][key] = R.step_grads(c["P"], *R.gathered(c, indexed), mode, R.ALPHA)
    return c["ref"][key]


def note(key, err):
    LEVELS[key] = max(LEVELS.get(key, 0.0), float(err))


class Arena:
    """Tensors carved out of one sentinel-filled device buffer, GUARD sentinel floats around each."""

    def __init__(self, arrays):
        self.shapes = [None if a is None else tuple(np.shape(a)) for a in arrays]
        self.offs, off = [], GUARD
        for a in arrays:
            self.offs.append(off)
            if a is not None:
                off += int(np.size(a)) + GUARD
        self.buf = torch.full((off,), SENTINEL_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
        host = np.full(off, SENT, np.uint32).view(F32)
        for a, o in zip(arrays, self.offs):
            if a is not None and not isinstance(a, _Blank):
                host[o:o + np.size(a)] = np.asarray(a, F32).ravel()
        self.buf.copy_(torch.from_numpy(host))

    def ptr(self, i):
        return None if self.shapes[i] is None else C.c_void_p(self.buf.data_ptr() + 4 * self.offs[i])

    def ptrs(self):
        return (C.c_void_p * len(self.offs))(*[self.buf.data_ptr() + 4 * o for o in self.offs])

    def read(self, what):
        """The tensors as numpy; asserts that every guard float survived."""
        host = self.buf.cpu().numpy()
        bits = host.view(np.uint32)
        keep = np.ones(host.size, bool)
        out = []
        for s, o in zip(self.shapes, self.offs):
            if s is None:
                out.append(None)
                continue
            n = int(np.prod(s))
            keep[o:o + n] = False
            out.append(host[o:o + n].reshape(s).copy())
        assert (bits[keep] == SENT).all(), f"{what}: written outside a tensor"
        return out


class _Blank:
    """An output of this shape: left as sentinels."""

    def __init__(self, shape):
        self.shape = tuple(shape)
        self.size = int(np.prod(shape))


def all_written(a):
    return not (np.asarray(a).view(np.uint32) == SENT).any()


def _ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.umlh_last_error())


def _cfg(c):
    from umlh._lib import AeCfg
    return AeCfg(c["D"], c["C"], c["L"])


def _scratch(lib, c, rows, train):
    n = lib.umlh_ae_scratch(C.byref(_cfg(c)), rows[0], rows[1], train)
    assert n > 0
    extra = 4096
    buf = torch.full(((n + extra) // 4,), SENTINEL_BITS, dtype=torch.int32, device=DEV)
    return buf, n, extra


def _scratch_tail_ok(buf, n):
    return bool((buf[n // 4:] == SENTINEL_BITS).all().item())


def _tables(c):
    return [torch.from_numpy(t).to(DEV) for t in c["tables"]]


def run_forward(lib, c, indexed=True, idx=None, stream=None, want=(True, True, True)):
    """(losses [2], rec_x, rec_y, emb_x, emb_y) of one umlh_ae_forward; idx: (idx_x, idx_y) int32 arrays overriding the case's."""
    D, L = c["D"], c["L"]
    ids = list(idx) if idx is not None else (list(c["idx"]) if indexed else [None, None])
    rows = [c["rows"][v] if ids[v] is None else len(ids[v]) for v in range(2)]
    tabs = _tables(c)
    dids = [None if i is None or len(i) == 0 else torch.from_numpy(np.asarray(i, np.int32)).to(DEV) for i in ids]
    outs = Arena([_Blank((2,)) if want[0] else None] +
                 [_Blank((rows[v], D)) if want[1] and rows[v] else None for v in range(2)] +
                 [_Blank((rows[v], L)) if want[2] and rows[v] else None for v in range(2)])
    P = Arena(c["P"])
    scratch, n, _ = _scratch(lib, c, rows, 0)
    dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = None if stream is None else C.c_void_p(stream.cuda_stream)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    _ok(lib, lib.umlh_ae_forward(C.byref(_cfg(c)), P.ptrs(), dp(tabs[0]), c["ld"], dp(dids[0]), rows[0], dp(tabs[1]), c["ld"], dp(dids[1]),
                                 rows[1], outs.ptr(0), outs.ptr(1), outs.ptr(2), outs.ptr(3), outs.ptr(4), C.c_void_p(scratch.data_ptr()),
                                 n, st), "umlh_ae_forward")
    torch.cuda.synchronize()
    got = outs.read("ae_forward outputs")
    assert all(all_written(g) for g in got if g is not None), "an output that was asked for was not written"
    for a, b in zip(P.read("ae_forward parameters"), c["P"]):
        assert np.array_equal(a.view(np.uint32), np.asarray(b, F32).view(np.uint32)), "the forward changed a parameter"
    assert _scratch_tail_ok(scratch, n), "written behind the scratch"
    return got


def run_steps(lib, c, kind, mode, P, M, V, *, step=1, wd=0.0, momentum=0.0, n_steps=1, idx=None, indexed=True, alpha=R.ALPHA, v_null=False):
    """P, M, V (lists of 16 arrays) after n_steps fused steps, and the [n_steps, 3] losses."""
    rows = list(c["rows"])
    ids = list(idx) if idx is not None else (list(c["idx"]) if indexed else [None, None])
    tabs = _tables(c)
    dids = [None if i is None or len(i) == 0 else torch.from_numpy(np.asarray(i, np.int32)).to(DEV) for i in ids]
    aP, aM, aV = Arena(P), Arena(M), Arena(V)
    losses = Arena([_Blank((n_steps, 3))])
    scratch, n, _ = _scratch(lib, c, rows, 1)
    dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    _ok(lib, lib.umlh_ae_train_steps(C.byref(_cfg(c)), aP.ptrs(), aM.ptrs(), None if v_null else aV.ptrs(), dp(tabs[0]), c["ld"], dp(dids[0]),
                                     rows[0], dp(tabs[1]), c["ld"], dp(dids[1]), rows[1], n_steps, 1 if mode == "xy" else 0, alpha[0], alpha[1],
                                     O.OPT_ID[kind], LR, step, O.BETAS[0], O.BETAS[1], O.EPS, momentum, wd, losses.ptr(0),
                                     C.c_void_p(scratch.data_ptr()), n, None), "umlh_ae_train_steps")
    torch.cuda.synchronize()
    out = [a.read(f"ae_train_steps {w}") for a, w in ((aP, "P"), (aM, "M"), (aV, "V"))]
    ls = losses.read("ae_train_steps losses")[0]
    assert all_written(ls), "a loss was not written"
    assert _scratch_tail_ok(scratch, n), "written behind the scratch"
    return out[0], out[1], out[2], ls


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def live_state(c, seed=11):
    """Non-zero moments of the gradients' size."""
    rng = np.random.default_rng(seed)
    g = ref_of(c, "xy")["grads"]
    M, V = [], []
    for k, p in enumerate(c["P"]):
        s = float(np.abs(g[k]).max()) if g[k] is not None and np.abs(g[k]).max() > 0 else 1e-3
        M.append((rng.standard_normal(p.shape) * s).astype(F32))
        V.append((rng.uniform(0.5, 2.0, p.shape) * s * s).astype(F32))
    return M, V


# ---------------------------------------------------------------------------------------------------------------------------- #
# umlh_ae_forward
# ---------------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("indexed", [True, False], ids=["indexed", "rows"])
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_forward_against_float64(lib, case, indexed):
    c = case_of(case)
    ref = ref_of(c, "xy", indexed)
    got = run_forward(lib, c, indexed)
    bad = []
    for v, name in enumerate(("loss_x", "loss_y")):
        if c["rows"][v] == 0:
            assert got[0][v] == 0.0
            continue
        e = R.rel_err(got[0][v], ref["losses"][v])
        note((R.case_id(case), name), e)
        if not e <= R.BOUNDS[case][name]:
            bad.append(f"{name}: 2^{np.log2(e):.1f}")
    for v in range(2):
        if c["rows"][v] == 0:
            assert got[1 + v] is None and got[3 + v] is None
            continue
        for name, g, r in (("rec", got[1 + v], ref["rec"][v]), ("emb", got[3 + v], ref["emb"][v])):
            e = R.tensor_err(g, r)
            note((R.case_id(case), name), e)
            if not e <= R.BOUNDS[case][name]:
                bad.append(f"{name}[{v}]: 2^{np.log2(e):.1f}")
    assert not bad, bad


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[2], R.CASES[5]], ids=R.case_id)
def test_forward_is_reproducible_and_row_local(lib, case):
    c = case_of(case)
    a = run_forward(lib, c)
    b = run_forward(lib, c)
    s = run_forward(lib, c, stream=torch.cuda.Stream())
    for x, y, z in zip(a, b, s):
        assert bits_equal(x, y) and bits_equal(x, z)
    # the same rows at other positions of the batch: a row's reconstruction and embedding move with it, bit for bit
    rng = np.random.default_rng(3)
    perm = [rng.permutation(r) for r in c["rows"]]
    p = run_forward(lib, c, idx=[c["idx"][v][perm[v]] for v in range(2)])
    for v in range(2):
        assert bits_equal(p[1 + v], a[1 + v][perm[v]]) and bits_equal(p[3 + v], a[3 + v][perm[v]])
    # the outputs are optional one by one: the embeddings alone, the losses alone
    e = run_forward(lib, c, want=(False, False, True))
    assert e[0] is None and e[1] is None and bits_equal(e[3], a[3]) and bits_equal(e[4], a[4])
    l = run_forward(lib, c, want=(True, False, False))
    assert bits_equal(l[0], a[0])
    # one view at a time gives that view's numbers
    x_only = run_forward(lib, c, idx=[c["idx"][0], np.zeros(0, np.int32)])
    assert bits_equal(x_only[1], a[1]) and x_only[0][0] == a[0][0] and x_only[0][1] == 0.0


# ---------------------------------------------------------------------------------------------------------------------------- #
# the gradient, read exactly
# ---------------------------------------------------------------------------------------------------------------------------- #
def sgd_probe(lib, c, mode, indexed=True):
    """(gradients [16], P after, losses): sgd with momentum 0, no decay and zero moments leaves the gradient in M."""
    zeros = [np.zeros(p.shape, F32) for p in c["P"]]
    V = [np.full(p.shape, 0.25, F32) for p in c["P"]]
    P1, M1, V1, ls = run_steps(lib, c, "sgd", mode, c["P"], zeros, V, indexed=indexed)
    for a, b in zip(V1, V):
        assert bits_equal(a, b), "sgd touched V"
    return M1, P1, ls


@pytest.mark.parametrize("mode", ["xy", "x"])
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_gradient_of_every_tensor(lib, case, mode):
    c = case_of(case)
    ref = ref_of(c, mode)
    g, P1, ls = sgd_probe(lib, c, mode)
    bad = []
    for j, name in enumerate(("loss_x", "loss_y", "loss")):
        e = R.rel_err(ls[0][j], ref["losses"][j])
        note((R.case_id(case), name), e)
        if not e <= R.BOUNDS[case][name]:
            bad.append(f"{name}: 2^{np.log2(e):.1f}")
    for k in range(16):
        if ref["grads"][k] is None:                                     # not touched at all
            assert not g[k].any() and bits_equal(P1[k], c["P"][k]), R.NAMES[k]
            continue
        e = R.tensor_err(g[k], ref["grads"][k])
        note((R.case_id(case), R.group_key(k)), e)
        if not e <= R.BOUNDS[case][R.group_key(k)]:
            bad.append(f"{R.NAMES[k]}: 2^{np.log2(e):.1f} > 2^{np.log2(R.BOUNDS[case][R.group_key(k)]):.0f}")
        want = (c["P"][k].astype(F64) - LR * g[k].astype(F64))          # p - lr * m on the gradient the kernel formed
        assert O.ulp_err(P1[k], want, c["P"][k]) <= O.BOUNDS["sgd"]["p"], R.NAMES[k]
    assert not bad, bad


def test_gradient_with_unindexed_rows_and_null_v(lib):
    c = case_of(R.CASES[2])
    ref = ref_of(c, "xy", indexed=False)
    g, _, _ = sgd_probe(lib, c, "xy", indexed=False)
    for k in range(16):
        assert R.tensor_err(g[k], ref["grads"][k]) <= R.BOUNDS[R.CASES[2]][R.group_key(k)], R.NAMES[k]
    zeros = [np.zeros(p.shape, F32) for p in c["P"]]
    P1, M1, _, _ = run_steps(lib, c, "sgd", "xy", c["P"], zeros, zeros, indexed=False, v_null=True)
    assert all(bits_equal(a, b) for a, b in zip(M1, g))


# ---------------------------------------------------------------------------------------------------------------------------- #
# a real step, mode 'x', chains
# ---------------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("kind", ["adam", "adamw"])
@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[2], R.CASES[5]], ids=R.case_id)
def test_real_step_from_a_live_state(lib, case, kind):
    """Step 7 from non-zero moments, in ulps against opt_ref ON THE GRADIENT THE KERNEL FORMED (read by the sgd probe: the launches
    are bit-reproducible), under the bounds of tests/test_optstep_gpu.py; the gradient itself is held to float64 above."""
    c = case_of(case)
    g, _, _ = sgd_probe(lib, c, "xy")
    M, V = live_state(c)
    P1, M1, V1, _ = run_steps(lib, c, kind, "xy", c["P"], M, V, step=7, wd=0.1)
    bad = []
    for k in range(16):
        ref = O.opt_ref(kind, c["P"][k], g[k], M[k], V[k], LR, 7, wd=0.1)
        for o, got, want, before in (("p", P1[k], ref[0], c["P"][k]), ("m", M1[k], ref[1], M[k]), ("v", V1[k], ref[2], V[k])):
            e = O.ulp_err(got, want, before)
            note(f"{kind}_{o}_ulps", e)
            if not e <= O.BOUNDS[kind][o]:
                bad.append(f"{R.NAMES[k]} {o}: {e:.1f} ulps > {O.BOUNDS[kind][o]:.0f}")
    assert not bad, bad


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[2]], ids=R.case_id)
def test_mode_x_leaves_the_y_heads_alone(lib, case):
    c = case_of(case)
    M, V = live_state(c)
    P1, M1, V1, ls = run_steps(lib, c, "adamw", "x", c["P"], M, V, step=7, wd=0.1)
    for k in (2, 3, 14, 15):
        assert bits_equal(P1[k], c["P"][k]) and bits_equal(M1[k], M[k]) and bits_equal(V1[k], V[k]), R.NAMES[k]
    for k in (0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13):
        assert not bits_equal(P1[k], c["P"][k]), R.NAMES[k]
    ref = ref_of(c, "x")
    assert R.rel_err(ls[0][1], ref["losses"][1]) <= R.LOSS_BOUNDS["loss_y"]            # loss_y is still reported
    assert ls[0][2] == ls[0][0]


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[2], R.CASES[4]], ids=R.case_id)
def test_nine_steps_in_one_call_equal_nine_calls(lib, case):
    c = case_of(case)
    rng = np.random.default_rng(9)
    n = 9
    idx = [rng.integers(0, len(c["tables"][v]), n * c["rows"][v]).astype(np.int32) for v in range(2)]
    M, V = live_state(c)
    P9, M9, V9, l9 = run_steps(lib, c, "adam", "xy", c["P"], M, V, step=3, n_steps=n, idx=idx)
    P, l1 = c["P"], []
    for s in range(n):
        one = [idx[v][s * c["rows"][v]:(s + 1) * c["rows"][v]] for v in range(2)]
        P, M, V, ls = run_steps(lib, c, "adam", "xy", P, M, V, step=3 + s, idx=one)
        l1.append(ls[0])
    assert bits_equal(l9, np.stack(l1))
    for a, b in zip(P9 + M9 + V9, P + M + V):
        assert bits_equal(a, b)
    assert not bits_equal(P9[4], c["P"][4])
