"""No GPU: the grouped forms of the Gaussian toy's entry points (umlh_ae_train_steps_grouped, umlh_ae_forward_grouped and their size
queries): their place in the ABI, every argument check with pointers that are never dereferenced, the scratch queries, the grid
expansion of gaussian.sweep against itertools.product, and GroupedTrainer's bookkeeping against a lone FusedTrainer's through stubs."""
import ctypes as C
import itertools

import pytest
import torch

E_INVALID = -1
NEW = ("umlh_ae_group_scratch", "umlh_ae_eval_group_scratch", "umlh_ae_train_steps_grouped", "umlh_ae_forward_grouped")
FAKE = 4096          # never dereferenced: every check comes before the first HIP call


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


# ---------------------------------------------------------------------------------------------------------------------------- #
# ABI
# ---------------------------------------------------------------------------------------------------------------------------- #
def test_abi_placement_and_prototypes(lib):
    from test_abi_cpu import prototype_mismatches
    from umlh import _lib
    assert prototype_mismatches(_lib.PROTOTYPES) == []
    names = list(_lib.PROTOTYPES)
    assert lib.umlh_version() == 11
    at = names.index("umlh_ae_train_steps")
    assert tuple(names[at + 1:at + 5]) == NEW and names[at + 5] == "umlh_seq_first_nonzero"
    assert names[-5:] == ["umlh_seq_first_nonzero", "umlh_seq_column_standardize_scratch", "umlh_seq_column_standardize",
                          "umlh_seq_standardize", "umlh_seq_gather_pad"]
    for n in NEW:
        fn = getattr(lib, n)
        assert fn.restype is _lib.PROTOTYPES[n][0] and list(fn.argtypes) == list(_lib.PROTOTYPES[n][1])
        assert not n.endswith("_scratch_bytes")
    assert lib.umlh_ae_group_scratch.restype is C.c_uint64 and lib.umlh_ae_eval_group_scratch.restype is C.c_uint64
    hdr = open(_lib._INCLUDE + "/umlh.h").read()
    pos = [hdr.index(w) for w in ("int  umlh_ae_train_steps(", "uint64_t umlh_ae_group_scratch(", "uint64_t umlh_ae_eval_group_scratch(",
                                  "int  umlh_ae_train_steps_grouped(", "int  umlh_ae_forward_grouped(", "umlh_seq_first_nonzero(")]
    assert pos == sorted(pos)
    assert "#define UMLH_AE_MAX_GROUP 64" in hdr and _lib.AE_MAX_GROUP == 64
    import umlh
    assert umlh.ae_train_steps_grouped is umlh.gauss.ae_train_steps_grouped and umlh.ae_forward_grouped is umlh.gauss.ae_forward_grouped


# ---------------------------------------------------------------------------------------------------------------------------- #
# argument checks
# ---------------------------------------------------------------------------------------------------------------------------- #
_KEEP = []


def _ptrs(base, hole=None):
    """16 distinct fake device pointers from ``base`` on; the array is kept alive for the module."""
    arr = (C.c_void_p * 16)(*[None if i == hole else base + 64 * i for i in range(16)])
    _KEEP.append(arr)
    return C.cast(arr, C.POINTER(C.c_void_p))


def _item(i=0, D=50, Cc=128, L=10, bx=4, by=4, opt=1, back=1, **over):
    from umlh._lib import AeCfg, AeGroupItem
    base = (1 << 20) * (i + 1)
    it = AeGroupItem(cfg=AeCfg(D, Cc, L), P=_ptrs(base), M=_ptrs(base + 4096), V=_ptrs(base + 8192), x=FAKE, ldx=D, idx_x=FAKE, batch_x=bx,
                     y=FAKE, ldy=D, idx_y=FAKE, batch_y=by, backward_y=back, alpha_x=1.0, alpha_y=1.0, optimizer=opt, lr=1e-3,
                     first_step=1, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.9, weight_decay=0.0, losses=FAKE)
    for k, v in over.items():
        setattr(it, k, v)
    return it


def _eval_item(i=0, D=50, Cc=128, L=10, nx=4, ny=4, **over):
    from umlh._lib import AeCfg, AeEvalItem
    it = AeEvalItem(cfg=AeCfg(D, Cc, L), P=_ptrs((1 << 20) * (i + 1)), x=FAKE, ldx=D, idx_x=None, n_x=nx, y=FAKE, ldy=D, idx_y=None, n_y=ny,
                    losses=FAKE, rec_x=None, rec_y=None, emb_x=None, emb_y=None)
    for k, v in over.items():
        setattr(it, k, v)
    return it


def _array(items):
    arr = (type(items[0]) * len(items))(*items)
    _KEEP.append(arr)
    return arr


def _train(lib, items, steps=1, scratch=FAKE, nbytes=1 << 40, n=None):
    rc = lib.umlh_ae_train_steps_grouped(_array(items) if items else None, len(items) if n is None else n, steps, scratch, nbytes, None)
    return rc, lib.umlh_last_error().decode()


def _forward(lib, items, scratch=FAKE, nbytes=1 << 40, n=None):
    rc = lib.umlh_ae_forward_grouped(_array(items) if items else None, len(items) if n is None else n, scratch, nbytes, None)
    return rc, lib.umlh_last_error().decode()


def test_group_count_and_null_items(lib):
    for call, who in ((_train, "umlh_ae_train_steps_grouped"), (_forward, "umlh_ae_forward_grouped")):
        make = _item if call is _train else _eval_item
        rc, msg = call(lib, [], n=1)
        assert rc == E_INVALID and who in msg and "items is NULL" in msg, msg
        for n in (0, -1, 65):
            rc, msg = call(lib, [make(i) for i in range(2)], n=n)
            assert rc == E_INVALID and who in msg and "n_items" in msg, msg


TRAIN_BAD = [  # what is wrong with member 1, the word the message must carry
    (dict(D=0), "dim_obs"), (dict(D=1025), "dim_obs"), (dict(Cc=513), "dim_common"), (dict(L=0), "dim_latent"), (dict(bx=65537), "batch_x"),
    (dict(by=-1), "batch_y"), (dict(bx=0, by=0), "both views absent"), (dict(ldx=49), "ldx"), (dict(ldy=49), "ldy"),
    (dict(x=None), "x is NULL"), (dict(y=None), "y is NULL"), (dict(opt=3), "optimizer"), (dict(back=2), "backward_y"),
    (dict(losses=None), "losses"), (dict(P=None), "P is NULL"), (dict(M=None), "M is NULL"), (dict(V=None), "V is NULL")]


@pytest.mark.parametrize("bad,word", TRAIN_BAD, ids=[w[1] + str(i) for i, w in enumerate(TRAIN_BAD)])
def test_a_member_outside_the_single_run_envelope_is_named(lib, bad, word):
    rc, msg = _train(lib, [_item(0), _item(1, **bad), _item(2)])
    assert rc == E_INVALID and "umlh_ae_train_steps_grouped" in msg and "member 1" in msg and word in msg, msg


def test_train_tensor_holes_steps_scratch_and_sgd(lib):
    for name in "PMV":
        rc, msg = _train(lib, [_item(0), _item(1), _item(2, **{name: _ptrs(1 << 30, hole=7)})])
        assert rc == E_INVALID and "member 2" in msg and "%s[7]" % name in msg, msg
    for steps in (0, 65537):
        rc, msg = _train(lib, [_item(0)], steps=steps)
        assert rc == E_INVALID and "umlh_ae_train_steps_grouped" in msg and "n_steps" in msg, msg
    items = [_item(0), _item(1)]
    need = lib.umlh_ae_group_scratch(_array(items), 2, 3)
    for kw in (dict(scratch=None), dict(nbytes=need - 1), dict(scratch=FAKE + 4)):
        rc, msg = _train(lib, items, steps=3, **kw)
        assert rc == E_INVALID and "umlh_ae_train_steps_grouped" in msg and "scratch" in msg, (kw, msg)


def test_shared_parameter_or_moment_tensors_are_refused(lib):
    a, b = _item(0), _item(1)
    b.M = a.P                                                   # member 1's M is member 0's P
    rc, msg = _train(lib, [a, b])
    assert rc == E_INVALID and "umlh_ae_train_steps_grouped" in msg and "member 1" in msg and "member 0" in msg and "M[" in msg \
        and "P[" in msg, msg
    a, b, c = _item(0), _item(1), _item(2)
    c.V = a.V
    rc, msg = _train(lib, [a, b, c])
    assert rc == E_INVALID and "member 2" in msg and "member 0" in msg and "V[" in msg, msg
    a = _item(0)
    a.M = a.P                                                   # twice within one member
    rc, msg = _train(lib, [a])
    assert rc == E_INVALID and "member 0" in msg and "share" in msg, msg
    # V of an sgd member is not looked at: NULL is fine there, and so is anything else.  The call then gets as far as the
    # scratch check, which is the last one before the device
    a, b = _item(0), _item(1, opt=0, V=None)
    rc, msg = _train(lib, [a, b], nbytes=8)
    assert rc == E_INVALID and "scratch of 8 bytes" in msg, msg
    b = _item(1, opt=0)
    b.V = a.V
    rc, msg = _train(lib, [a, b], nbytes=8)
    assert rc == E_INVALID and "scratch of 8 bytes" in msg, msg
    # tables and row ids may be shared: every item above names the same fake table


FWD_BAD = [(dict(D=1025), "dim_obs"), (dict(nx=(1 << 20) + 1), "n_x"), (dict(ny=-1), "n_y"), (dict(nx=0, ny=0), "both views absent"),
           (dict(ldx=49), "ldx"), (dict(y=None), "y is NULL"), (dict(P=None), "P is NULL")]


@pytest.mark.parametrize("bad,word", FWD_BAD, ids=[w[1] + str(i) for i, w in enumerate(FWD_BAD)])
def test_an_evaluation_member_outside_the_envelope_is_named(lib, bad, word):
    rc, msg = _forward(lib, [_eval_item(0), _eval_item(1), _eval_item(2, **bad)])
    assert rc == E_INVALID and "umlh_ae_forward_grouped" in msg and "member 2" in msg and word in msg, msg


def test_forward_scratch_checks(lib):
    items = [_eval_item(0), _eval_item(1, P=_ptrs(1 << 29, hole=15))]
    rc, msg = _forward(lib, items)
    assert rc == E_INVALID and "member 1" in msg and "P[15]" in msg, msg
    items = [_eval_item(0), _eval_item(1)]
    need = lib.umlh_ae_eval_group_scratch(_array(items), 2)
    for kw in (dict(scratch=None), dict(nbytes=need - 1), dict(scratch=FAKE + 4)):
        rc, msg = _forward(lib, items, **kw)
        assert rc == E_INVALID and "umlh_ae_forward_grouped" in msg and "scratch" in msg, (kw, msg)


# ---------------------------------------------------------------------------------------------------------------------------- #
# scratch queries
# ---------------------------------------------------------------------------------------------------------------------------- #
def test_group_scratch_query(lib):
    from umlh._lib import AeCfg
    shapes = [(50, 128, 10, 32, 32), (17, 15, 4, 17, 1), (1, 1, 1, 1, 1), (12, 16, 40, 16, 48), (50, 128, 10, 0, 20)]
    items = [_item(i, D, Cc, L, bx, by) for i, (D, Cc, L, bx, by) in enumerate(shapes)]
    arr = _array(items)
    single = sum(lib.umlh_ae_scratch(C.byref(AeCfg(D, Cc, L)), bx, by, 1) for D, Cc, L, bx, by in shapes)
    sizes = [lib.umlh_ae_group_scratch(arr, len(items), s) for s in (1, 2, 3, 1000)]
    assert all(n >= single and n % 256 == 0 for n in sizes)
    assert sizes[0] < sizes[2] < sizes[3]
    # the optimizer table is the only part that grows with the steps: a fixed number of bytes per (step, member), rounded to 256
    per = (sizes[3] - sizes[0]) / (999 * len(items))
    assert 32 <= per <= 128 and abs((sizes[2] - sizes[0]) - 2 * per * len(items)) <= 256
    assert lib.umlh_ae_group_scratch(arr, 1, 1) < sizes[0]
    for bad in ((None, 1, 1), (arr, 0, 1), (arr, 65, 1), (arr, -1, 1), (arr, 2, 0), (arr, 2, 65537)):
        assert lib.umlh_ae_group_scratch(*bad) == 0, bad
    for kw in (dict(D=0), dict(Cc=513), dict(L=513), dict(bx=65537), dict(bx=0, by=0), dict(by=-1)):
        assert lib.umlh_ae_group_scratch(_array([_item(0), _item(1, **kw)]), 2, 1) == 0, kw


def test_eval_group_scratch_query(lib):
    from umlh._lib import AeCfg
    shapes = [(50, 128, 10, 40, 40), (17, 15, 4, 33, 0), (12, 16, 40, 0, 17)]
    arr = _array([_eval_item(i, D, Cc, L, nx, ny) for i, (D, Cc, L, nx, ny) in enumerate(shapes)])
    single = sum(lib.umlh_ae_scratch(C.byref(AeCfg(D, Cc, L)), nx, ny, 0) for D, Cc, L, nx, ny in shapes)
    n = lib.umlh_ae_eval_group_scratch(arr, 3)
    assert n >= single and n % 256 == 0
    for bad in ((None, 1), (arr, 0), (arr, 65)):
        assert lib.umlh_ae_eval_group_scratch(*bad) == 0, bad
    for kw in (dict(D=1025), dict(nx=(1 << 20) + 1), dict(nx=0, ny=0)):
        assert lib.umlh_ae_eval_group_scratch(_array([_eval_item(0), _eval_item(1, **kw)]), 2) == 0, kw


# ---------------------------------------------------------------------------------------------------------------------------- #
# grids
# ---------------------------------------------------------------------------------------------------------------------------- #
def _paper(**over):
    g = dict(dim_common=[128], dim_latent=[10], data_dim_common=[10], data_dim_x=[5], data_dim_y=[5], dim_obs=[50], num_steps=[10000],
             noise_std=[0.09], train_num_samples=[10000], batch_size=[512], val_num_samples=[2000], lr=[1.0e-3], seed=[0, 1, 2], alpha_x=[1.0],
             alpha_y=[1.0], mode=["xy", "x"], attenuation=[0.05], tag=["original"], unrelated_info=[False])
    g.update(over)
    return g


GRIDS = {  # six grids of the reference's configs/, key order as in the files, and their run counts
    "original": (_paper(), 6),
    "diff_dim_latent": (_paper(dim_latent=[5, 10, 20, 50, 100], tag=["different_dim_latent"]), 30),
    "diff_batch_sizes": (_paper(batch_size=[1, 2, 4, 8, 16, 32, 64, 128, 256, 512], tag=["different_batch_sizes"]), 60),
    "diff_dim_common": (_paper(dim_common=[16, 32, 64, 128, 256], tag=["different_dim_common_new"]), 30),
    "diff_attenuation": (_paper(attenuation=[0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 1.0], tag=["different_attenuation_new"]), 54),
    "unrelated_information": (_paper(mode=["xy"], tag=["unrelated_information"], unrelated_info=[True, False]), 6),
}


@pytest.mark.parametrize("name", list(GRIDS))
def test_expand_grid_is_the_reference_product(name):
    from gaussian.sweep import expand_grid
    grid, count = GRIDS[name]
    points = expand_grid(grid)
    keys = list(grid)
    want = [dict(zip(keys, v)) for v in itertools.product(*grid.values())]
    assert len(points) == count and points == want
    assert all(list(p) == keys for p in points)
    # a scalar behaves as a one-element list
    scalars = {k: (v[0] if len(v) == 1 else v) for k, v in grid.items()}
    assert expand_grid(scalars) == points


def test_expand_grid_order_is_last_key_fastest():
    from gaussian.sweep import expand_grid
    pts = expand_grid(dict(seed=[0, 1], mode=["xy", "x"], alpha_y=[1.0, 0.5], lr=1e-3))
    assert [(p["seed"], p["mode"], p["alpha_y"]) for p in pts[:3]] == [(0, "xy", 1.0), (0, "xy", 0.5), (0, "x", 1.0)]
    assert len(pts) == 8 and all(p["lr"] == 1e-3 for p in pts)


def test_load_grid_reads_yaml(tmp_path):
    from gaussian.sweep import expand_grid, load_grid
    path = tmp_path / "grid.yaml"
    path.write_text("dim_latent: [5, 10]\nseed: [0,1,2]\nmode: ['xy', 'x']\nlr: [1.0e-3]\nunrelated_info: [false]\ntag: 'one'\n")
    pts = load_grid(str(path))
    assert pts == expand_grid(dict(dim_latent=[5, 10], seed=[0, 1, 2], mode=["xy", "x"], lr=[1e-3], unrelated_info=[False], tag="one"))
    assert len(pts) == 12 and pts[0]["unrelated_info"] is False


def test_make_data_is_cached_by_what_it_depends_on():
    from gaussian.sweep import make_data
    base = dict(dim_obs=6, data_dim_common=3, data_dim_x=2, data_dim_y=2, train_num_samples=12, val_num_samples=5, noise_std=0.09)
    a = make_data(dict(base, seed=0, mode="xy"))
    assert make_data(dict(base, seed=1, mode="x", dim_latent=4, alpha_y=0.5)) is a
    assert make_data(dict(base, attenuation=0.5)) is not a
    train, train2, val = a
    assert train["x"].shape == (12, 6) and train2["y"].shape == (12, 6) and val["x"].shape == (5, 6)
    assert not torch.equal(train["y"], train2["y"])


# ---------------------------------------------------------------------------------------------------------------------------- #
# GroupedTrainer bookkeeping
# ---------------------------------------------------------------------------------------------------------------------------- #
def _trainer(seed, n_rows, batch, span, total, opt_name="adam"):
    from engine.optimizer.optim import build_optimizer
    from gaussian.data import UnpairedDataset
    from gaussian.fused import FusedTrainer
    from gaussian.model import SharedAutoencoder
    torch.manual_seed(seed)
    ds = UnpairedDataset(torch.randn(n_rows, 6), torch.randn(n_rows - 3, 6))
    g = torch.Generator()
    g.manual_seed(100 + seed)
    model = SharedAutoencoder(dim_obs=6, dim_common=8, dim_latent=3)
    opt = build_optimizer(model.parameters(), opt_name, 1e-3 * (seed + 1), 0.0)
    return FusedTrainer(model, opt, ds, batch, g, "cpu", span_steps=span, total_steps=total), g


def _record(log):
    def call(**kw):
        log.append(dict(n_steps=kw["n_steps"], idx_x=kw["idx_x"].clone(), idx_y=kw["idx_y"].clone(), first_step=kw["first_step"],
                        batch=(kw["batch_x"], kw["batch_y"]), mode=kw["mode"], alpha=(kw["alpha_x"], kw["alpha_y"]), lr=kw["lr"],
                        optimizer=kw["optimizer"], losses=tuple(kw["losses"].shape), x=kw["x"].data_ptr(), m=kw["m"][0].data_ptr()))
    return call


def _flatten(calls):
    """The per-step view of a list of recorded calls: what each step was given, whatever the split into calls."""
    steps = []
    for c in calls:
        bx, by = c["batch"]
        for s in range(c["n_steps"]):
            steps.append((c["idx_x"][s * bx:(s + 1) * bx].tolist(), c["idx_y"][s * by:(s + 1) * by].tolist(), c["first_step"] + s, c["mode"],
                          c["alpha"], c["lr"], c["optimizer"], c["x"], c["m"]))
        assert c["losses"] == (c["n_steps"], 3)
    return steps


SPECS = [  # seed, rows, batch, span_steps, total_steps, optimizer, (mode, alpha_x, alpha_y): members run out of ids at different steps
    (0, 40, 8, 4, None, "adam", ("xy", 1.0, 1.0)), (1, 23, 5, 7, 30, "sgd", ("x", 1.0, 1.0)), (2, 64, 16, 3, None, "adamw", ("xy", 1.0, 0.3))]
CALLS = (5, 1, 9, 2, 11)


def test_grouped_trainer_passes_what_the_lone_trainers_pass(monkeypatch):
    from gaussian.fused import GroupedTrainer
    from umlh import gauss
    lone_logs = []
    for spec in SPECS:
        tr, g = _trainer(*spec[:6])
        log = []
        monkeypatch.setattr(gauss, "ae_train_steps", _record(log))
        for n in CALLS:
            out = tr.steps(n, *spec[6])
            assert tuple(out.shape) == (n, 3)
        lone_logs.append((log, g.get_state(), tr.optimizer.step_count))

    members = [_trainer(*spec[:6]) for spec in SPECS]
    group_log = [[] for _ in SPECS]

    def grouped(ms, n_steps):
        assert len(ms) == len(SPECS)
        for log, mb in zip(group_log, ms):
            _record(log)(n_steps=n_steps, **mb)
        return [mb["losses"] for mb in ms]

    monkeypatch.setattr(gauss, "ae_train_steps_grouped", grouped)
    monkeypatch.setattr(gauss, "ae_train_steps", lambda **kw: pytest.fail("the grouped trainer called the single-run entry point"))
    gt = GroupedTrainer([t for t, _ in members], [spec[6] for spec in SPECS])
    for n in CALLS:
        outs = gt.steps(n)
        assert [tuple(o.shape) for o in outs] == [(n, 3)] * len(SPECS)
    for (tr, g), log, (lone, state, count), spec in zip(members, group_log, lone_logs, SPECS):
        a, b = _flatten(log), _flatten(lone)
        assert len(a) == sum(CALLS)
        # tables and moments are each trainer's own: compare everything but the two addresses
        assert [s[:7] for s in a] == [s[:7] for s in b]
        assert len({s[7] for s in a}) == 1 and len({s[8] for s in a}) == 1
        assert torch.equal(g.get_state(), state) and tr.optimizer.step_count == count == sum(CALLS)


def test_fused_trainer_takes_device_tables_without_copying():
    from engine.optimizer.optim import build_optimizer
    from gaussian.data import UnpairedDataset
    from gaussian.fused import FusedTrainer
    from gaussian.model import SharedAutoencoder
    x, y = torch.randn(20, 6), torch.randn(20, 6)
    ds = UnpairedDataset(x[:10], y[:10])
    trainers = []
    for _ in range(2):
        model = SharedAutoencoder(dim_obs=6, dim_common=8, dim_latent=3)
        trainers.append(FusedTrainer(model, build_optimizer(model.parameters(), "adam", 1e-3, 0.0), ds, 4, torch.Generator(), "cpu",
                                     tables=(x, y)))
    assert all(t.x.data_ptr() == x.data_ptr() and t.y.data_ptr() == y.data_ptr() for t in trainers)
    with pytest.raises(ValueError, match="tables"):
        model = SharedAutoencoder(dim_obs=6, dim_common=8, dim_latent=3)
        FusedTrainer(model, build_optimizer(model.parameters(), "adam", 1e-3, 0.0), ds, 4, torch.Generator(), "cpu", tables=(x[:5], y))
