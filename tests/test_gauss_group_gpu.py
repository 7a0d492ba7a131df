"""GPU: the grouped forms of the Gaussian toy's entry points against the single-run ones, bit for bit.  The single-run path is held
to float64 by tests/test_gauss_kernels_gpu.py; here every parameter, moment, loss, reconstruction and embedding a grouped call
leaves is compared as uint32 words with what umlh_ae_train_steps / umlh_ae_forward leave for that member alone.  No tolerance
appears.  All tensors a call writes are carved from one allocation with guard gaps of a NaN pattern, which must survive.  Row ids
are addresses: each is drawn from [0, n) of its table and that is asserted on the host before any call."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from _gemm_ref import SENTINEL_BITS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SENT = np.uint32(SENTINEL_BITS)
GUARD = 24
OPT = {"sgd": 0, "adam": 1, "adamw": 2}
STEPS = 9


@pytest.fixture(scope="module")
def lib():
    import umlh
    return umlh.load_library()


def shapes_of(D, Cc, L):
    return [(Cc, D), (Cc,), (Cc, D), (Cc,), (L, Cc), (L,), (L, L), (L,), (L, L), (L,), (Cc, L), (Cc,), (D, Cc), (D,), (D, Cc), (D,)]


class Arena:
    """Arrays carved out of one sentinel-filled device buffer, GUARD sentinel words around each."""

    def __init__(self, arrays):
        self.shapes = [tuple(np.shape(a)) for a in arrays]
        self.offs, off = [], GUARD
        for a in arrays:
            self.offs.append(off)
            off += int(np.size(a)) + GUARD
        host = np.full(off, SENT, np.uint32)
        for a, o in zip(arrays, self.offs):
            if not isinstance(a, Blank):
                host[o:o + np.size(a)] = np.asarray(a, F32).ravel().view(np.uint32)
        self.buf = torch.from_numpy(host.view(np.int32)).to(DEV)

    def addr(self, i):
        return self.buf.data_ptr() + 4 * self.offs[i]

    def read(self, what):
        """The arrays as uint32 words; asserts that every guard word survived."""
        bits = self.buf.cpu().numpy().view(np.uint32)
        keep = np.ones(bits.size, bool)
        out = []
        for s, o in zip(self.shapes, self.offs):
            n = int(np.prod(s))
            keep[o:o + n] = False
            out.append(bits[o:o + n].reshape(s).copy())
        assert (bits[keep] == SENT).all(), f"{what}: written outside a tensor"
        return out


class Blank:
    """An output of this shape: left as sentinels until it is written."""

    def __init__(self, *shape):
        self.shape = tuple(shape)
        self.size = int(np.prod(shape))


_TABLES = {}


def table(key, n, D, ld=None):
    """A [n, D] fp32 device table (row stride ld), made once per key and never changed."""
    if key not in _TABLES:
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        host = rng.standard_normal((n, ld or D)).astype(F32)
        _TABLES[key] = torch.from_numpy(host).to(DEV)
    return _TABLES[key]


def ids(rng, count, n):
    a = rng.integers(0, n, count).astype(np.int32)
    assert a.size == count and (a >= 0).all() and (a < n).all()          # an id is an address
    return a


class Run:
    """One training run: shapes, hyperparameters, tables, row ids and the initial state."""

    def __init__(self, seed, D, Cc, L, bx, by, mode, opt, *, lr, first_step, alpha=(1.0, 1.0), wd=0.0, tables=None, n_rows=70, steps=STEPS):
        rng = np.random.default_rng(seed)
        self.D, self.Cc, self.L, self.bx, self.by, self.mode, self.opt = D, Cc, L, bx, by, mode, opt
        self.lr, self.first_step, self.alpha, self.wd, self.steps = lr, first_step, alpha, wd, steps
        self.x, self.y = tables if tables is not None else (table(("x", seed), n_rows, D), table(("y", seed), n_rows, D))
        self.idx_x = torch.from_numpy(ids(rng, steps * bx, self.x.shape[0])).to(DEV) if bx else None
        self.idx_y = torch.from_numpy(ids(rng, steps * by, self.y.shape[0])).to(DEV) if by else None
        self.P = [(rng.standard_normal(s) / np.sqrt(s[-1] if len(s) == 2 else 4.0)).astype(F32) for s in shapes_of(D, Cc, L)]
        self.M = [(rng.standard_normal(s) * 1e-2).astype(F32) for s in shapes_of(D, Cc, L)]
        self.V = [(rng.uniform(0.5, 2.0, s) * 1e-4).astype(F32) for s in shapes_of(D, Cc, L)]

    def arrays(self, steps):
        return self.P + self.M + self.V + [Blank(steps, 3)]


def _ptr16(arena, base):
    return (C.c_void_p * 16)(*[arena.addr(base + i) for i in range(16)])


def _raw(t, off=0):
    return None if t is None else t.data_ptr() + off


def _split(words):
    return dict(P=words[0:16], M=words[16:32], V=words[32:48], losses=words[48])


def run_single(lib, r, steps=None):
    """P, M, V and [steps, 3] losses (uint32 words) after one umlh_ae_train_steps call from the run's initial state."""
    from umlh._lib import AeCfg
    steps = r.steps if steps is None else steps
    cfg = AeCfg(r.D, r.Cc, r.L)
    arena = Arena(r.arrays(steps))
    n = lib.umlh_ae_scratch(C.byref(cfg), r.bx, r.by, 1)
    assert n > 0
    scratch = torch.empty(n, dtype=torch.uint8, device=DEV)
    rc = lib.umlh_ae_train_steps(C.byref(cfg), _ptr16(arena, 0), _ptr16(arena, 16), None if r.opt == "sgd" else _ptr16(arena, 32),
                                 _raw(r.x), r.x.stride(0), _raw(r.idx_x), r.bx, _raw(r.y), r.y.stride(0), _raw(r.idx_y), r.by, steps,
                                 1 if r.mode == "xy" else 0, r.alpha[0], r.alpha[1], OPT[r.opt], r.lr, r.first_step, 0.9, 0.999, 1e-8, 0.9,
                                 r.wd, arena.addr(48), scratch.data_ptr(), n, None)
    assert rc == 0, lib.umlh_last_error()
    torch.cuda.synchronize()
    return _split(arena.read("umlh_ae_train_steps"))


def run_group(lib, runs, steps=None, calls=1, poison=None):
    """The same per member after ``calls`` consecutive umlh_ae_train_steps_grouped calls of ``steps`` steps each, all members'
    tensors in one arena.  poison: the member whose parameters start as NaN."""
    from umlh._lib import AeCfg, AeGroupItem
    steps = runs[0].steps // calls if steps is None else steps
    arrays = []
    for i, r in enumerate(runs):
        a = r.arrays(steps * calls)
        if i == poison:
            a[:16] = [np.full_like(p, np.nan) for p in a[:16]]
        arrays += a
    arena = Arena(arrays)
    keep = []
    for c in range(calls):
        items = (AeGroupItem * len(runs))()
        for i, (it, r) in enumerate(zip(items, runs)):
            base = 49 * i
            ptrs = [_ptr16(arena, base), _ptr16(arena, base + 16), _ptr16(arena, base + 32)]
            keep.append(ptrs)
            it.cfg = AeCfg(r.D, r.Cc, r.L)
            it.P, it.M = C.cast(ptrs[0], C.POINTER(C.c_void_p)), C.cast(ptrs[1], C.POINTER(C.c_void_p))
            it.V = None if r.opt == "sgd" else C.cast(ptrs[2], C.POINTER(C.c_void_p))
            it.x, it.ldx, it.idx_x, it.batch_x = _raw(r.x), r.x.stride(0), _raw(r.idx_x, 4 * c * steps * r.bx), r.bx
            it.y, it.ldy, it.idx_y, it.batch_y = _raw(r.y), r.y.stride(0), _raw(r.idx_y, 4 * c * steps * r.by), r.by
            it.backward_y, it.alpha_x, it.alpha_y = 1 if r.mode == "xy" else 0, r.alpha[0], r.alpha[1]
            it.optimizer, it.lr, it.first_step = OPT[r.opt], r.lr, r.first_step + c * steps
            it.beta1, it.beta2, it.eps, it.momentum, it.weight_decay = 0.9, 0.999, 1e-8, 0.9, r.wd
            it.losses = arena.addr(base + 48) + 4 * 3 * c * steps
        n = lib.umlh_ae_group_scratch(items, len(runs), steps)
        assert n > 0 and n % 256 == 0
        scratch = torch.empty(n, dtype=torch.uint8, device=DEV)
        rc = lib.umlh_ae_train_steps_grouped(items, len(runs), steps, scratch.data_ptr(), n, None)
        assert rc == 0, lib.umlh_last_error()
    torch.cuda.synchronize()
    words = arena.read("umlh_ae_train_steps_grouped")
    return [_split(words[49 * i:49 * (i + 1)]) for i in range(len(runs))]


def same(a, b, opt):
    """Every P / M / V tensor and the losses, word for word (V of an sgd run is not touched by either path: still compared)."""
    return all(np.array_equal(x, y) for k in ("P", "M", "V") for x, y in zip(a[k], b[k])) and np.array_equal(a["losses"], b["losses"])


def differing(a, b):
    return [f"{k}[{i}]" for k in ("P", "M", "V") for i, (x, y) in enumerate(zip(a[k], b[k])) if not np.array_equal(x, y)] + \
        ([] if np.array_equal(a["losses"], b["losses"]) else ["losses"])


_SIX = {}


def six(lib):
    """The six members of the issue's table and their isolated nine-step results, computed once."""
    if not _SIX:
        shared = (table(("x", "shared"), 70, 50), table(("y", "shared"), 70, 50))
        runs = [Run(1, 50, 128, 10, 32, 32, "xy", "adam", lr=1e-2, first_step=1, tables=shared),
                Run(2, 50, 128, 10, 32, 32, "x", "adam", lr=3e-3, first_step=7, tables=shared),
                Run(3, 17, 15, 4, 17, 1, "xy", "sgd", lr=5e-2, first_step=1000),
                Run(4, 1, 1, 1, 1, 1, "x", "adamw", lr=2e-2, first_step=3, wd=0.1),
                Run(5, 12, 16, 40, 16, 48, "xy", "adam", lr=1e-3, first_step=42, alpha=(1.0, 0.3)),
                Run(6, 50, 128, 10, 0, 20, "xy", "adam", lr=7e-3, first_step=2)]
        _SIX["runs"] = runs
        _SIX["alone"] = [run_single(lib, r) for r in runs]
    return _SIX["runs"], _SIX["alone"]


# ---------------------------------------------------------------------------------------------------------------------------- #
# training
# ---------------------------------------------------------------------------------------------------------------------------- #
def test_six_members_in_one_call_equal_six_isolated_runs(lib):
    runs, alone = six(lib)
    got = run_group(lib, runs)
    for i, (g, a, r) in enumerate(zip(got, alone, runs)):
        assert same(g, a, r.opt), (i, differing(g, a))
        assert not (g["losses"] == SENT).any(), (i, "a loss was not written")
    # the equality is not vacuous: members 1 and 2 start from different states and end in different ones, the runs moved their
    # parameters, and mode 'x' left member 2's y heads alone
    assert not np.array_equal(alone[0]["P"][4], alone[1]["P"][4]) and not np.array_equal(alone[0]["losses"], alone[1]["losses"])
    for a, r in zip(alone, runs):
        assert not np.array_equal(a["P"][4], np.asarray(r.P[4], F32).view(np.uint32))
    for k in (2, 3, 14, 15):
        assert np.array_equal(alone[1]["P"][k], runs[1].P[k].view(np.uint32))


def test_member_order_does_not_matter(lib):
    runs, alone = six(lib)
    got = run_group(lib, runs[::-1])[::-1]
    for i, (g, a, r) in enumerate(zip(got, alone, runs)):
        assert same(g, a, r.opt), (i, differing(g, a))


@pytest.mark.parametrize("which", [0, 2, 3, 5])
def test_a_group_of_one_is_the_single_call(lib, which):
    runs, alone = six(lib)
    got = run_group(lib, [runs[which]])[0]
    assert same(got, alone[which], runs[which].opt), differing(got, alone[which])


def test_nine_calls_of_one_step_equal_one_call_of_nine(lib):
    runs, alone = six(lib)
    got = run_group(lib, runs, steps=1, calls=STEPS)
    for i, (g, a, r) in enumerate(zip(got, alone, runs)):
        assert same(g, a, r.opt), (i, differing(g, a))


def test_sixty_four_members_and_not_one_more(lib):
    runs = [Run(100 + i, 1, 1, 1, 1, 1, "xy" if i % 2 else "x", "adam", lr=1e-2 * (1 + i % 5), first_step=1 + i, n_rows=5, steps=3)
            for i in range(64)]
    got = run_group(lib, runs)
    for i, (g, r) in enumerate(zip(got, runs)):
        a = run_single(lib, r)
        assert same(g, a, r.opt), (i, differing(g, a))
    assert len({g["losses"].tobytes() for g in got}) > 32            # distinct seeds: distinct runs
    from umlh._lib import AeGroupItem
    items = (AeGroupItem * 65)()
    assert lib.umlh_ae_group_scratch(items, 65, 3) == 0
    assert lib.umlh_ae_train_steps_grouped(items, 65, 3, 4096, 1 << 40, None) == -1
    assert b"n_items=65" in lib.umlh_last_error()


def test_a_poisoned_member_does_not_reach_the_others(lib):
    runs, alone = six(lib)
    trio = [runs[0], runs[2], runs[4]]
    got = run_group(lib, trio, poison=1)                               # the arena's guard gaps are checked in there
    assert same(got[0], alone[0], "adam"), differing(got[0], alone[0])
    assert same(got[2], alone[4], "adam"), differing(got[2], alone[4])
    assert np.isnan(got[1]["P"][4].view(F32)).all() and np.isnan(got[1]["losses"].view(F32)[:, 0]).all()


# ---------------------------------------------------------------------------------------------------------------------------- #
# forward
# ---------------------------------------------------------------------------------------------------------------------------- #
class Eval:
    """One evaluation member: its parameters, views (table, row ids, rows) and which outputs it asks for."""

    def __init__(self, seed, D, Cc, L, nx, ny, *, indexed=False, ld=None, want=(True, True, True)):
        rng = np.random.default_rng(seed)
        self.D, self.Cc, self.L, self.want = D, Cc, L, want
        self.P = [(rng.standard_normal(s) / np.sqrt(s[-1] if len(s) == 2 else 4.0)).astype(F32) for s in shapes_of(D, Cc, L)]
        n_tab = 50
        self.tabs = [table(("ex", seed), n_tab, D, ld)[:, :D] if nx else None, table(("ey", seed), n_tab, D, ld)[:, :D] if ny else None]
        self.rows = [nx, ny]
        self.idx = [torch.from_numpy(ids(rng, n, n_tab)).to(DEV) if indexed and n else None for n in (nx, ny)]
        assert all(n <= n_tab for n in self.rows)

    def outputs(self):
        """losses, rec_x, rec_y, emb_x, emb_y: one row longer than needed, or None."""
        w_l, w_r, w_e = self.want
        return [Blank(2 + 1) if w_l else None] + [Blank(n + 1, self.D) if w_r and n else None for n in self.rows] + \
            [Blank(n + 1, self.L) if w_e and n else None for n in self.rows]


def _eval_args(e, outs, base):
    """(P array, x, ldx, idx_x, n_x, y, ldy, idx_y, n_y, five output addresses) of one member; outs: the arena of all outputs."""
    out_addr = []
    for o in e.outputs():
        out_addr.append(None if o is None else outs.addr(base[0]))
        base[0] += o is not None
    ld = [t.stride(0) if t is not None else e.D for t in e.tabs]
    return [_raw(e.tabs[0]), ld[0], _raw(e.idx[0]), e.rows[0], _raw(e.tabs[1]), ld[1], _raw(e.idx[1]), e.rows[1]] + out_addr


def _eval_read(members, outs):
    """Per member the five outputs as words without their extra last row (None where not asked for); the extra rows are intact."""
    words, k, res = outs.read("forward outputs"), 0, []
    for e in members:
        got = []
        for o in e.outputs():
            if o is None:
                got.append(None)
                continue
            w = words[k]
            k += 1
            assert (w[-1:] == SENT).all(), "written behind an output"
            assert not (w[:-1] == SENT).any(), "an output that was asked for was not written"
            got.append(w[:-1])
        res.append(got)
    return res


def test_grouped_forward_equals_the_single_forwards(lib):
    from umlh._lib import AeCfg, AeEvalItem
    members = [Eval(21, 50, 128, 10, 40, 40, indexed=True), Eval(22, 17, 15, 4, 33, 0, want=(True, False, True)),
               Eval(23, 12, 16, 40, 0, 17, want=(False, True, True)), Eval(24, 5, 9, 3, 16, 31, ld=11, want=(True, True, False))]
    assert members[3].tabs[0].stride(0) == 11
    flat = lambda: [o for e in members for o in e.outputs() if o is not None]
    # one by one
    outs = Arena(flat())
    params = [Arena(e.P) for e in members]
    base = [0]
    for e, pa in zip(members, params):
        cfg = AeCfg(e.D, e.Cc, e.L)
        n = lib.umlh_ae_scratch(C.byref(cfg), e.rows[0], e.rows[1], 0)
        scratch = torch.empty(n, dtype=torch.uint8, device=DEV)
        a = _eval_args(e, outs, base)
        rc = lib.umlh_ae_forward(C.byref(cfg), _ptr16(pa, 0), *a, scratch.data_ptr(), n, None)
        assert rc == 0, lib.umlh_last_error()
    torch.cuda.synchronize()
    alone = _eval_read(members, outs)
    # all in one call
    outs = Arena(flat())
    items = (AeEvalItem * len(members))()
    base, keep = [0], []
    for it, e, pa in zip(items, members, params):
        arr = _ptr16(pa, 0)
        keep.append(arr)
        it.cfg, it.P = AeCfg(e.D, e.Cc, e.L), C.cast(arr, C.POINTER(C.c_void_p))
        (it.x, it.ldx, it.idx_x, it.n_x, it.y, it.ldy, it.idx_y, it.n_y, it.losses, it.rec_x, it.rec_y, it.emb_x,
         it.emb_y) = _eval_args(e, outs, base)
    n = lib.umlh_ae_eval_group_scratch(items, len(members))
    assert n > 0 and n % 256 == 0
    scratch = torch.empty(n, dtype=torch.uint8, device=DEV)
    rc = lib.umlh_ae_forward_grouped(items, len(members), scratch.data_ptr(), n, None)
    assert rc == 0, lib.umlh_last_error()
    torch.cuda.synchronize()
    got = _eval_read(members, outs)
    names = ("losses", "rec_x", "rec_y", "emb_x", "emb_y")
    for i, (g, a) in enumerate(zip(got, alone)):
        for name, x, y in zip(names, g, a):
            assert (x is None) == (y is None)
            assert x is None or np.array_equal(x, y), (i, name)
    for pa, e in zip(params, members):                                # a forward changes no parameter
        for w, p in zip(pa.read("forward parameters"), e.P):
            assert np.array_equal(w, p.view(np.uint32))
    assert got[0][0] is not None and got[1][1] is None and got[2][0] is None and got[3][3] is None
    assert not np.array_equal(got[0][1], got[0][2])


def test_python_wrappers_equal_the_single_run_wrappers():
    """umlh.ae_train_steps_grouped / ae_forward_grouped against umlh.ae_train_steps / ae_forward on torch tensors."""
    import umlh
    gen = torch.Generator().manual_seed(5)
    members, lone = [], []
    for D, Cc, L, b, mode, opt in ((6, 8, 3, 4, "xy", "adam"), (9, 5, 7, 3, "x", "sgd")):
        shapes = umlh.gauss.tensor_shapes(D, Cc, L)
        P = [torch.randn(s, generator=gen).mul_(0.3).to(DEV) for s in shapes]
        M = [torch.zeros(s, device=DEV) for s in shapes]
        V = None if opt == "sgd" else [torch.zeros(s, device=DEV) for s in shapes]
        x, y = torch.randn(20, D, generator=gen).to(DEV), torch.randn(20, D, generator=gen).to(DEV)
        ix = torch.randint(0, 20, (5 * b,), generator=gen).to(torch.int32)
        iy = torch.randint(0, 20, (5 * b,), generator=gen).to(torch.int32)
        assert int(ix.min()) >= 0 and int(ix.max()) < 20 and int(iy.min()) >= 0 and int(iy.max()) < 20
        kw = dict(x=x, y=y, idx_x=ix.to(DEV), idx_y=iy.to(DEV), batch_x=b, batch_y=b, mode=mode, optimizer=opt, lr=1e-2, first_step=3)
        clone = lambda ts: None if ts is None else [t.clone() for t in ts]
        members.append(dict(params=P, m=M, v=V, **kw))
        lone.append(dict(params=clone(P), m=clone(M), v=clone(V), **kw))
    losses = umlh.ae_train_steps_grouped(members, 5)
    for mb, ln, ls in zip(members, lone, losses):
        ref = umlh.ae_train_steps(n_steps=5, **ln)
        assert torch.equal(ls.view(torch.int32), ref.view(torch.int32))
        for k in ("params", "m", "v"):
            if mb[k] is not None:
                assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(mb[k], ln[k])), k
    outs = umlh.ae_forward_grouped([dict(params=mb["params"], x=mb["x"], y=mb["y"]) for mb in members])
    for mb, got in zip(members, outs):
        ref = umlh.ae_forward(mb["params"], mb["x"], mb["y"])
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, ref))
    # which of the 48 shared tensors is named depends on their addresses: the check sorts the pointers
    with pytest.raises(umlh.UmlhError, match=r"member 1: ([PMV])\[(\d+)\] is also member 0's \1\[\2\]"):
        umlh.ae_train_steps_grouped([members[0], dict(members[0])], 5)          # two members over the same tensors


# ---------------------------------------------------------------------------------------------------------------------------- #
# end to end
# ---------------------------------------------------------------------------------------------------------------------------- #
def test_sweep_grouped_equals_the_runs_alone():
    from gaussian import sweep
    from gaussian.train import train_model_steps_fused
    grid = dict(dim_obs=12, dim_common=16, dim_latent=4, train_num_samples=64, batch_size=16, val_num_samples=40, num_steps=12, lr=1e-3,
                seed=[0, 1], mode=["xy", "x"], alpha_y=[1.0, 0.5])
    points = sweep.expand_grid(grid)
    assert len(points) == 8
    logs, runs = sweep.sweep_grouped(points, eval_every=4, alignment=True, group_size=3, device=DEV, return_runs=True)
    assert len(logs) == 8
    seen = []
    for point, log, (model, optimizer) in zip(points, logs, runs):
        train, train2, val = sweep.make_data(point)
        ds, gen, lone, opt = sweep.build_point(point, DEV)
        ref = train_model_steps_fused(lone, ds, opt, 12, val["x"], val["y"], DEV, batch_size=16, generator=gen, mode=point["mode"],
                                      alpha_x=1.0, alpha_y=point["alpha_y"], eval_every=4, alignment=True)
        assert set(log) == set(ref) and all(log[k] == ref[k] for k in ref), point
        assert len(log["loss"]) == 12 and len(log["val_loss_x"]) == 3 and len(log["val_cka"]) == 3 and len(log["val_mknn"]) == 3
        a, b = model.state_dict(), lone.state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a), point
        assert optimizer.step_count == opt.step_count == 12
        for q, q2 in zip(model.parameters(), lone.parameters()):
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(optimizer.state_for(q)[k].view(torch.int32), opt.state_for(q2)[k].view(torch.int32)), (point, k)
        seen.append(log["loss"])
    # different runs: mode 'x' does not look at alpha_y (loss = loss_x), so its two points per seed agree and all others differ
    assert len({tuple(s) for s in seen}) == 6


def test_sweep_grouped_leaves_the_optimizers_where_the_lone_runs_do():
    from gaussian import sweep
    from gaussian.fused import FusedTrainer, GroupedTrainer
    grid = dict(dim_obs=12, dim_common=16, dim_latent=4, train_num_samples=64, batch_size=16, val_num_samples=40, num_steps=12, lr=1e-3,
                seed=[0, 1], mode=["xy", "x"])
    points = sweep.expand_grid(grid)
    built = [sweep.build_point(p, DEV) for p in points]
    trainers = [FusedTrainer(m, o, ds, 16, g, DEV, span_steps=12, total_steps=12) for ds, g, m, o in built]
    GroupedTrainer(trainers, [(p["mode"], 1.0, 1.0) for p in points]).steps(12)
    for p, (ds, g, m, o) in zip(points, built):
        ds2, g2, m2, o2 = sweep.build_point(p, DEV)
        FusedTrainer(m2, o2, ds2, 16, g2, DEV, span_steps=12, total_steps=12).steps(12, mode=p["mode"])
        assert o.step_count == o2.step_count == 12 and torch.equal(g.get_state(), g2.get_state())
        for q, q2 in zip(m.parameters(), m2.parameters()):
            assert torch.equal(q.data.view(torch.int32), q2.data.view(torch.int32))
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(o.state_for(q)[k].view(torch.int32), o2.state_for(q2)[k].view(torch.int32)), (p, k)
