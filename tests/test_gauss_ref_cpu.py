"""No GPU: the float64 statement of the Gaussian toy's fused step (tests/_gauss_ref.py) against torch float64 autograd, the
calibration of the GPU bounds, the kink-free data, the wrong variants the bounds must reject, gaussian.fused.batch_order against
torch's DataLoader itself, and the new entry points' place in the ABI and their argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import _gauss_ref as R
import _optstep_ref as O

E_INVALID = -1


# ---------------------------------------------------------------------------------------------------------------------------- #
# the float64 statement
# ---------------------------------------------------------------------------------------------------------------------------- #
def _torch_model(P):
    D, Cc, L = P[0].shape[1], P[0].shape[0], P[4].shape[0]
    lin = torch.nn.Linear
    m = torch.nn.ModuleDict(dict(in_head_x=lin(D, Cc), in_head_y=lin(D, Cc),
                                 shared_encoder=torch.nn.Sequential(lin(Cc, L), torch.nn.ReLU(), lin(L, L)),
                                 shared_decoder=torch.nn.Sequential(lin(L, L), torch.nn.ReLU(), lin(L, Cc)),
                                 out_head_x=lin(Cc, D), out_head_y=lin(Cc, D))).double()
    assert [k for k, _ in m.named_parameters()] == list(R.NAMES)
    with torch.no_grad():
        for p, v in zip(m.parameters(), P):
            p.copy_(torch.from_numpy(np.asarray(v, np.float64)))
    return m


def _torch_view(m, a0, v):
    h = m["in_head_" + v](a0)
    emb = m["shared_encoder"](h)
    rec = m["out_head_" + v](m["shared_decoder"](emb))
    return torch.nn.functional.mse_loss(rec, a0), rec, emb


AUTOGRAD = [((5, 17, 3, 15, 33), "xy"), ((5, 17, 3, 15, 33), "x"), ((50, 128, 10, 130, 130), "xy"), ((50, 128, 10, 130, 130), "x"),
            ((33, 64, 128, 0, 130), "xy"), ((33, 64, 128, 130, 0), "xy"), ((33, 64, 128, 130, 0), "x")]


@pytest.mark.parametrize("case,mode", AUTOGRAD, ids=[R.case_id(c) + "_" + m for c, m in AUTOGRAD])
def test_float64_statement_matches_torch_autograd(case, mode):
    c = R.build_case(case, 0)
    ax, ay = R.gathered(c)
    alpha = (1.0, 0.5)
    ref = R.step_grads(c["P"], ax, ay, mode, alpha)
    m = _torch_model(c["P"])
    zero = torch.zeros((), dtype=torch.float64)
    lx, recx, embx = _torch_view(m, torch.from_numpy(ax.astype(np.float64)), "x") if ax is not None else (zero, None, None)
    ly, recy, emby = _torch_view(m, torch.from_numpy(ay.astype(np.float64)), "y") if ay is not None else (zero, None, None)
    loss = alpha[0] * lx + alpha[1] * ly if mode == "xy" else lx
    loss.backward()
    close = lambda a, b: np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(b).max())))
    close(ref["losses"][0], lx.item()); close(ref["losses"][1], ly.item()); close(ref["losses"][2], loss.item())
    for got, want in ((ref["rec"][0], recx), (ref["rec"][1], recy), (ref["emb"][0], embx), (ref["emb"][1], emby)):
        assert (got is None) == (want is None)
        if got is not None:
            close(got, want.detach().numpy())
    for k, (name, p) in enumerate(m.named_parameters()):
        if ref["grads"][k] is None:
            assert p.grad is None or not p.grad.any(), name
        else:
            close(ref["grads"][k], p.grad.numpy())


def test_update_is_opt_ref_per_tensor():
    c = R.build_case((5, 17, 3, 15, 33), 0)
    ax, ay = R.gathered(c)
    g = R.step_grads(c["P"], ax, ay, "x")["grads"]
    M = [np.full(p.shape, 0.01) for p in c["P"]]
    V = [np.full(p.shape, 1e-4) for p in c["P"]]
    P1, M1, V1 = R.apply_update("adamw", c["P"], g, M, V, 1e-2, 7, wd=0.1)
    for k in (2, 3, 14, 15):                                            # mode 'x': the y heads and their moments stay
        np.testing.assert_array_equal(P1[k], c["P"][k]); np.testing.assert_array_equal(M1[k], M[k]); np.testing.assert_array_equal(V1[k], V[k])
    p, m, v = O.opt_ref("adamw", c["P"][4], g[4], M[4], V[4], 1e-2, 7, wd=0.1)
    np.testing.assert_array_equal(P1[4], p)


# ---------------------------------------------------------------------------------------------------------------------------- #
# calibration, kinks, wrong variants
# ---------------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_recorded_levels_cover_the_measured_ones_and_bounds_follow(case):
    lv, rec, bounds = R.measure_levels(case), R.LEVELS_LOG2[case], R.BOUNDS[case]
    for k in R.OUTPUTS:
        if rec[k] is None:                                              # exact in the restatement: exact on the GPU
            assert lv[k] == 0 and bounds[k] == 0.0, k
            continue
        assert lv[k] > 0, k
        assert np.log2(lv[k]) <= rec[k], (k, np.log2(lv[k]))
        assert np.log2(lv[k]) > rec[k] - 0.5, (k, np.log2(lv[k]))                    # the record is not stale
        level = R.LOSS_LEVELS_LOG2[k] if k in R.LOSS_KEYS else rec[k]
        assert bounds[k] == 2.0 ** int(np.ceil(level + 3 - 1e-9))
        assert 8 * lv[k] <= bounds[k]
        if k not in R.LOSS_KEYS:
            assert bounds[k] < 16 * 2.0 ** rec[k]


def test_loss_levels_are_the_tables_largest():
    for k in R.LOSS_KEYS:
        assert R.LOSS_LEVELS_LOG2[k] == max(d[k] for d in R.LEVELS_LOG2.values() if d[k] is not None)
    assert set(R.LEVELS_LOG2) == set(R.CASES)


def test_k_order_is_a_permutation():
    for K in (1, 3, 4, 5, 15, 16, 17, 50, 500):
        assert sorted(R.k_order(K)) == list(range(K))
    assert R.k_order(17)[:6] == [0, 4, 8, 12, 1, 5] and R.k_order(17)[-1] == 16


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_case_data_has_no_relu_kink(case):
    for seed in R.SEEDS:
        c = R.build_case(case, seed)
        for indexed in (True, False):
            assert R.kink_margin(c["P"], *R.gathered(c, indexed)) > R.KINK, (seed, indexed)
        c2 = R.build_case(case, seed)                                   # a function of (case, seed) alone
        assert all(np.array_equal(a, b) for a, b in zip(c["P"], c2["P"]))


@pytest.mark.parametrize("case", R.VARIANT_CASES, ids=R.case_id)
@pytest.mark.parametrize("name", R.WRONG_VARIANTS)
def test_bounds_reject_wrong_variant(name, case):
    """On a small case, at the paper's widths and at L = 500; a zero gradient and a gradient with one tile missing among them."""
    assert R.variant_excess(name, case) >= 8.0


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_gradient_bounds_reject_zero_and_one_missing_tile_per_tensor(case):
    """Every gradient tensor of every case on its own: all zero, and the last 16 x 16 tile left at zero."""
    c = R.build_case(case, 0)
    ref = R.step_grads(c["P"], *R.gathered(c), "xy")
    for k, g in enumerate(ref["grads"]):
        if g is None or not np.abs(g).max() > 0:
            continue
        b = R.BOUNDS[case][R.group_key(k)]
        assert R.tensor_err(np.zeros_like(g), g) >= 8 * b, R.NAMES[k]
        if np.abs(g - R.drop_last_tile(g)).max() > 0:
            assert R.tensor_err(R.drop_last_tile(g), g) >= 8 * b, R.NAMES[k]


@pytest.mark.parametrize("name,kind", [("step_off_by_one", "adam"), ("decay_after_update", "adamw")])
def test_ulp_bounds_reject_wrong_update(name, kind):
    c = R.build_case(R.VARIANT_CASES[0], 0)
    g = R.step_grads(c["P"], *R.gathered(c), "xy")["grads"]
    rng = np.random.default_rng(5)
    worst = 0.0
    for k in range(16):
        m = (g[k] * rng.uniform(0.2, 1.0, g[k].shape)).astype(np.float32)
        v = (g[k] ** 2 * rng.uniform(0.5, 2.0, g[k].shape)).astype(np.float32)
        ref = O.opt_ref(kind, c["P"][k], g[k], m, v, O.LR, 7, wd=0.1)
        got = O.opt_ref(kind, c["P"][k], g[k], m, v, O.LR, 7, wd=0.1, wrong=(name,))
        worst = max(worst, O.ulp_err(got[0], ref[0], c["P"][k]) / O.BOUNDS[kind]["p"])
    assert worst >= 8.0


# ---------------------------------------------------------------------------------------------------------------------------- #
# the batch order against torch's DataLoader
# ---------------------------------------------------------------------------------------------------------------------------- #
def _loader_order(len_x, len_y, batch, seed, steps):
    """Row numbers (x, y) of the first `steps` batches of the reference's loader cycled as train_model_steps cycles it."""
    from torch.utils.data import DataLoader
    from gaussian.data import UnpairedDataset
    ds = UnpairedDataset(torch.arange(len_x), torch.arange(len_y))
    g = torch.Generator()
    g.manual_seed(seed)
    loader = DataLoader(ds, batch_size=batch, shuffle=True, drop_last=True, generator=g)
    it = iter(loader)
    xs, ys = [], []
    for _ in range(steps):
        try:
            b = next(it)
        except StopIteration:
            it = iter(loader)
            b = next(it)
        xs.append(b["x"]); ys.append(b["y"])
    return torch.cat(xs), torch.cat(ys)


@pytest.mark.parametrize("len_x,len_y,batch", [(10, 10, 3), (12, 12, 3), (12, 12, 4), (7, 7, 7), (5, 5, 1), (600, 600, 128), (11, 7, 3), (9, 13, 4)])
def test_batch_order_is_the_loaders(len_x, len_y, batch):
    from gaussian.fused import BatchOrder, batch_order
    n = max(len_x, len_y)
    steps = 3 * (n // batch) + 1                                        # three whole epochs and the first batch of the fourth
    want_x, want_y = _loader_order(len_x, len_y, batch, 42, steps)
    g = torch.Generator()
    g.manual_seed(42)
    order = batch_order(n, batch, g, steps)
    assert order.dtype == torch.int64 and order.shape == (steps * batch,)
    assert torch.equal(order % len_x, want_x) and torch.equal(order % len_y, want_y)
    g.manual_seed(42)
    spans = BatchOrder(n, batch, g)
    k = n // batch + 1 if steps > n // batch + 1 else 1
    assert torch.equal(torch.cat([spans.take(k), spans.take(steps - k)]), order)      # two consecutive spans = one long span


def test_batch_order_rejects_a_batch_longer_than_the_data():
    from gaussian.fused import batch_order
    with pytest.raises(ValueError, match="batch_size"):
        batch_order(4, 5, torch.Generator(), 1)


# ---------------------------------------------------------------------------------------------------------------------------- #
# ABI and argument checks
# ---------------------------------------------------------------------------------------------------------------------------- #
NEW = ("umlh_ae_scratch", "umlh_ae_forward", "umlh_ae_train_steps")


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_abi_placement_and_prototypes(lib):
    from test_abi_cpu import prototype_mismatches
    from umlh import _lib
    assert prototype_mismatches(_lib.PROTOTYPES) == []
    names = list(_lib.PROTOTYPES)
    assert lib.umlh_version() == 11
    for n in NEW:
        fn = getattr(lib, n)
        assert fn.restype is _lib.PROTOTYPES[n][0] and list(fn.argtypes) == list(_lib.PROTOTYPES[n][1])
        assert names.index("umlh_rows_gather") < names.index(n) < names.index("umlh_seq_first_nonzero")
    assert lib.umlh_ae_scratch.restype is C.c_uint64 and not any(n.endswith("_scratch_bytes") for n in NEW)
    assert "umlh_kernels_gauss.hip" in _lib.SOURCES
    hdr = open(_lib._INCLUDE + "/umlh.h").read()
    assert hdr.index("umlh_rows_gather(") < hdr.index("uint64_t umlh_ae_scratch(") < hdr.index("umlh_seq_first_nonzero(")
    import umlh
    assert umlh.ae_forward is umlh.gauss.ae_forward and umlh.ae_train_steps is umlh.gauss.ae_train_steps


def _ptrs(hole=None):
    return (C.c_void_p * 16)(*[None if i == hole else 64 + 64 * i for i in range(16)])


FAKE = C.c_void_p(4096)        # never dereferenced: every check comes before the first HIP call


def _forward(lib, D=50, Cc=128, L=10, nx=4, ny=4, P=None, ldx=None, ldy=None, x=FAKE, y=FAKE, scratch=FAKE, nbytes=1 << 40):
    from umlh._lib import AeCfg
    cfg = AeCfg(D, Cc, L)
    rc = lib.umlh_ae_forward(C.byref(cfg), _ptrs() if P is None else P, x, D if ldx is None else ldx, None, nx, y,
                             D if ldy is None else ldy, None, ny, FAKE, None, None, None, None, scratch, nbytes, None)
    return rc, lib.umlh_last_error().decode()


def _train(lib, D=50, Cc=128, L=10, bx=4, by=4, steps=1, P=None, M=None, V=None, ldx=None, opt=1, back=1, scratch=FAKE, nbytes=1 << 40,
           losses=FAKE):
    from umlh._lib import AeCfg
    cfg = AeCfg(D, Cc, L)
    rc = lib.umlh_ae_train_steps(C.byref(cfg), _ptrs() if P is None else P, _ptrs() if M is None else M, _ptrs() if V is None else V,
                                 FAKE, D if ldx is None else ldx, FAKE, bx, FAKE, D, FAKE, by, steps, back, 1.0, 1.0, opt, 1e-3, 1, 0.9,
                                 0.999, 1e-8, 0.9, 0.0, losses, scratch, nbytes, None)
    return rc, lib.umlh_last_error().decode()


def _query(lib, D=50, Cc=128, L=10, rx=4, ry=4, train=1):
    from umlh._lib import AeCfg
    return lib.umlh_ae_scratch(C.byref(AeCfg(D, Cc, L)), rx, ry, train)


ENVELOPE = [  # keyword, last valid value, first invalid values, the word the message must carry
    ("D", (1, 1024), (0, 1025), "dim_obs"), ("Cc", (1, 512), (0, 513), "dim_common"), ("L", (1, 512), (0, 513), "dim_latent")]


@pytest.mark.parametrize("key,good,bad,word", ENVELOPE, ids=[e[0] for e in ENVELOPE])
def test_dimension_envelope(lib, key, good, bad, word):
    for v in good:
        assert _query(lib, **{key: v}) > 0 and _query(lib, train=0, **{key: v}) > 0
    for v in bad:
        assert _query(lib, **{key: v}) == 0 and _query(lib, train=0, **{key: v}) == 0
        for call, who in ((_forward, "umlh_ae_forward"), (_train, "umlh_ae_train_steps")):
            rc, msg = call(lib, **{key: v})
            assert rc == E_INVALID and who in msg and word in msg, msg


def test_row_step_and_stride_envelope(lib):
    assert _query(lib, rx=65536, ry=0) > 0 and _query(lib, rx=0, ry=65536) > 0
    assert _query(lib, rx=1 << 20, ry=1 << 20, train=0) > 0
    for kw in (dict(rx=65537), dict(ry=65537), dict(rx=-1), dict(ry=-1), dict(rx=0, ry=0), dict(train=2), dict(train=-1),
               dict(rx=(1 << 20) + 1, train=0), dict(ry=(1 << 20) + 1, train=0), dict(rx=0, ry=0, train=0)):
        assert _query(lib, **kw) == 0, kw
    for kw, word in ((dict(bx=65537), "batch_x"), (dict(by=65537), "batch_y"), (dict(bx=-1), "batch_x"), (dict(by=-1), "batch_y"),
                     (dict(bx=0, by=0), "both views absent"), (dict(steps=0), "n_steps"), (dict(steps=65537), "n_steps"),
                     (dict(ldx=49), "ldx"), (dict(opt=3), "optimizer"), (dict(opt=-1), "optimizer"), (dict(back=2), "backward_y"),
                     (dict(scratch=None), "scratch"), (dict(nbytes=8), "scratch"), (dict(losses=None), "losses")):
        rc, msg = _train(lib, **kw)
        assert rc == E_INVALID and "umlh_ae_train_steps" in msg and word in msg, (kw, msg)
    for kw, word in ((dict(nx=(1 << 20) + 1), "n_x"), (dict(ny=(1 << 20) + 1), "n_y"), (dict(nx=-1), "n_x"), (dict(ny=-1), "n_y"),
                     (dict(nx=0, ny=0), "both views absent"), (dict(ldx=49), "ldx"), (dict(ldy=49), "ldy"), (dict(x=None), "x is NULL"),
                     (dict(y=None), "y is NULL"), (dict(scratch=None), "scratch"), (dict(nbytes=8), "scratch")):
        rc, msg = _forward(lib, **kw)
        assert rc == E_INVALID and "umlh_ae_forward" in msg and word in msg, (kw, msg)


def test_null_tensor_pointers(lib):
    for hole in (0, 7, 15):
        rc, msg = _forward(lib, P=_ptrs(hole))
        assert rc == E_INVALID and "umlh_ae_forward" in msg and "P[%d]" % hole in msg
        for name in "PMV":
            rc, msg = _train(lib, **{name: _ptrs(hole)})
            assert rc == E_INVALID and "umlh_ae_train_steps" in msg and "%s[%d]" % (name, hole) in msg
    from umlh._lib import AeCfg
    cfg = AeCfg(50, 128, 10)
    assert lib.umlh_ae_forward(C.byref(cfg), None, FAKE, 50, None, 4, FAKE, 50, None, 4, FAKE, None, None, None, None, FAKE, 1 << 40,
                               None) == E_INVALID
    assert "P is NULL" in lib.umlh_last_error().decode()
    assert lib.umlh_ae_scratch(None, 4, 4, 1) == 0


def test_scratch_query_is_the_plan(lib):
    """2 D + 4 C + 6 L floats per row and one fp64 partial per 16-row tile, every region rounded up to 256 bytes."""
    up = lambda b: (b + 255) // 256 * 256
    D, Cc, L, rx, ry = 50, 128, 10, 130, 33
    want = 0
    for rows in (rx, ry):
        want += up(8 * ((rows + 15) // 16)) + sum(2 * up(4 * rows * w) for w in (D, Cc, L, L, L, Cc))
    assert _query(lib, D, Cc, L, rx, ry, 1) == want
    assert _query(lib, D, Cc, L, rx, ry, 0) == up(8 * 9) + up(8 * 3)
