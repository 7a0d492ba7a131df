"""GPU: the robustness test sets.  ``umlh_seq_perturb`` through ctypes against the numpy statement of tests/_robust_ref.py, its
counter-stream element drop, ``multibench.data.robust_loaders`` against every batch the reference's own code recorded in
tests/golden/robust_noise.npz, and ``multibench.train.evaluate_robustness`` against ``evaluate``.

Bounds.  The kernel against the statement: equal as uint32 words -- the contract is one IEEE fp64 add and one conversion, there is
no tolerance to choose (a NaN result equals any NaN; without ``eps`` a NaN keeps its bits).  ``start_out``: equal to
``umlh.seqload.first_nonzero`` of the result.  Outputs sit in NaN / sentinel buffers one row (one entry) longer than needed:
everything inside is written, nothing behind it.  The element stream: the kept fraction within 5 sigma of 1 - p and the agreement
of the streams ``seed`` and ``seed + 1`` at most 5 sigma above independence, binomial sigma over 128 000 elements.  The families
without normalisation: bit for bit, inds, lengths and labels included.  With ``vision_norm``: max |got - ref64| / max |ref64| per
block at most ``_robust_ref.vnorm_bound(family)``, 8 times the reference's own fp32 error rounded up to a power of two (2^-15,
2^-17, 2^-17; measured and pinned in tests/test_robust_cpu.py).  Every measured figure is printed before it is asserted."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _robust_ref as RR
import _seqload_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77


@pytest.fixture(scope="module")
def fx():
    return RR.load_fixture()


@pytest.fixture(scope="module")
def lib():
    import umlh
    return umlh.load_library()


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _table(rng, n, T, d):
    """A float32 table with NaN, +-Inf, -0.0, +0.0 and denormals sprinkled over about a third of its elements."""
    x = rng.standard_normal((n, T, d)).astype(np.float32)
    kind = rng.integers(0, 18, x.shape)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40)):
        x[kind == k] = v
    return x


def _draws(rng, units):
    eps = rng.standard_normal(units) * 0.3
    eps[rng.random(units) < 0.2] = 0.0                          # -0.0 + 0.0 = +0.0
    return eps, (rng.random(units) >= 0.4).astype(np.uint8)


def _perturb(lib, x, per_step, eps, keep, in_place=False, shift=0, with_start=True, elem_p=0.0, seed=0, stream=None):
    """umlh_seq_perturb into a NaN buffer one row longer than the table, ``shift`` words past its aligned base, and a sentinel
    start buffer one entry longer: (result [n, T, d], start [n])."""
    n, T, d = x.shape
    words = n * T * d
    buf = torch.full((shift + words + d,), float("nan"), dtype=torch.float32, device=DEV)
    dst = buf[shift:]
    assert dst.data_ptr() % 16 == (4 * shift) % 16
    if in_place:
        dst[:words] = _dev(x).reshape(-1)
        src = dst
    else:
        src = _dev(x)
    start = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=DEV)
    e = None if eps is None else _dev(eps, np.float64)
    k = None if keep is None else _dev(keep, np.uint8)
    st = torch.cuda.current_stream(DEV) if stream is None else stream
    rc = lib.umlh_seq_perturb(src.data_ptr(), n, T, d, 1 if per_step else T, None if e is None else e.data_ptr(),
                              None if k is None else k.data_ptr(), C.c_float(elem_p), seed, dst.data_ptr(),
                              start.data_ptr() if with_start else None, C.c_void_p(st.cuda_stream))
    assert rc == 0, lib.umlh_last_error()
    st.synchronize()
    flat, s = buf.cpu().numpy(), start.cpu().numpy()
    assert np.isnan(flat[:shift]).all() and np.isnan(flat[shift + words:]).all(), "written outside the table"
    assert s[n] == SENTINEL and (with_start or (s == SENTINEL).all())
    return flat[shift:shift + words].reshape(n, T, d), s[:n], dst[:words].view(n, T, d)


def _check_against_statement(lib, x, per_step, use_eps, use_keep, rng, **how):
    n, T, d = x.shape
    units = (n, T) if per_step else (n,)
    eps, keep = _draws(rng, units)
    eps, keep = (eps if use_eps else None), (keep if use_keep else None)
    got, start, dst = _perturb(lib, x, per_step, eps, keep, **how)
    want, want_start = RR.perturb(x, eps, keep)
    what = (x.shape, per_step, use_eps, use_keep, how)
    if use_eps:
        assert RR.same_bits(got, want), what
    else:
        assert np.array_equal(_bits(got), _bits(want)), what      # identity outside dropped units: NaN payloads included
    if how.get("with_start", True):
        from umlh import seqload
        assert np.array_equal(start, want_start), what
        assert np.array_equal(start, seqload.first_nonzero(dst.contiguous()).cpu().numpy()), what
    return got, start


COMBOS = [(True, False), (False, True), (True, True), (False, False)]


@pytest.mark.parametrize("d", [1, 3, 4, 5, 7, 130])
def test_kernel_is_the_statement_word_for_word(lib, d):
    rng = np.random.default_rng(100 + d)
    for n in (1, 2, 23, 67):
        for T in (1, 3, 12):
            x = _table(rng, n, T, d)
            for per_step in (False, True):
                for use_eps, use_keep in COMBOS:
                    _check_against_statement(lib, x, per_step, use_eps, use_keep, rng)
    x = _table(rng, 23, 12, d)
    for per_step in (False, True):
        for use_eps, use_keep in COMBOS:
            _check_against_statement(lib, x, per_step, use_eps, use_keep, rng, in_place=True)
            _check_against_statement(lib, x, per_step, use_eps, use_keep, rng, shift=1)
            _check_against_statement(lib, x, per_step, use_eps, use_keep, rng, in_place=True, shift=1, with_start=False)


@pytest.mark.parametrize("shape", [(1, 1, 255), (1, 1, 256), (1, 1, 257), (1, 255, 1), (1, 256, 1), (1, 257, 1), (3, 85, 1), (1, 1, 70001),
                                   (1, 70001, 1), (7, 1429, 7)])
def test_kernel_at_the_flat_sizes_around_a_workgroup_step(lib, shape):
    rng = np.random.default_rng(shape[1] + shape[2])
    x = _table(rng, *shape)
    for per_step in (False, True):
        for use_eps, use_keep in COMBOS:
            _check_against_statement(lib, x, per_step, use_eps, use_keep, rng)
        _check_against_statement(lib, x, per_step, True, True, rng, in_place=True, shift=1)


def test_specials_in_dropped_and_kept_units_and_the_start_rule(lib):
    """A dropped unit is +0.0 whatever it held; a kept one follows IEEE; a sample that becomes all zero has start = T; per-step
    drops move the start."""
    T, d = 6, 4
    x = np.ones((4, T, d), dtype=np.float32)
    x[0, 0], x[1, 0], x[2, 0], x[3, 0] = (np.nan, np.inf, -np.inf, -2.0), (np.nan, np.inf, -np.inf, -0.0), -0.0, 1e-40
    x[2, 1:] = 0.0
    got, start = _check_against_statement_fixed(lib, x, False, np.zeros(4), np.array([0, 1, 1, 1], dtype=np.uint8))
    assert (_bits(got[0]) == 0).all() and start[0] == T                       # NaN, Inf, negative: assigned +0.0
    assert np.isnan(got[1, 0, 0]) and got[1, 0, 1] == np.inf and got[1, 0, 2] == -np.inf and _bits(got[1, 0, 3]) == 0 and start[1] == 0
    assert (_bits(got[2]) == 0).all() and start[2] == T                       # -0.0 + 0.0 = +0.0: the sample is all zero
    assert got[3, 0, 0] == np.float32(1e-40) and start[3] == 0                # a denormal is a nonzero
    keep = np.ones((4, T), dtype=np.uint8)
    keep[0, :3], keep[1, 0], keep[3] = 0, 0, 0
    got, start = _check_against_statement_fixed(lib, x, True, None, keep)
    assert start.tolist() == [3, 1, T, T] and (_bits(got[0, :3]) == 0).all() and np.array_equal(_bits(got[0, 3:]), _bits(x[0, 3:]))
    assert np.array_equal(_bits(got[2]), _bits(x[2]))                         # kept and no eps: -0.0 stays -0.0, and is no nonzero


def _check_against_statement_fixed(lib, x, per_step, eps, keep):
    got, start, _ = _perturb(lib, x, per_step, eps, keep)
    want, want_start = RR.perturb(x, eps, keep)
    assert RR.same_bits(got, want) and np.array_equal(start, want_start)
    return got, start


def test_two_calls_and_two_streams_give_the_same_bits(lib):
    rng = np.random.default_rng(5)
    x = _table(rng, 67, 12, 130)
    eps, keep = _draws(rng, (67, 12))
    a, sa, _ = _perturb(lib, x, True, eps, keep, elem_p=0.25, seed=9)
    b, sb, _ = _perturb(lib, x, True, eps, keep, elem_p=0.25, seed=9)
    c, sc, _ = _perturb(lib, x, True, eps, keep, elem_p=0.25, seed=9, stream=torch.cuda.Stream(DEV))
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    assert np.array_equal(sa, sb) and np.array_equal(sa, sc)


# ---- the element stream ----
N_ELEM = (50, 40, 64)


def _mask(p, seed, shape=N_ELEM):
    from umlh import seqload
    out = seqload.perturb(torch.ones(shape, dtype=torch.float32, device=DEV), elem_p=p, seed=seed).cpu().numpy()
    assert ((out == 0) | (out == 1)).all() and not np.signbit(out).any()
    return out != 0


def test_element_stream_is_a_mask_with_a_prefix_property():
    from umlh import seqload
    full = _mask(0.3, 17)
    assert np.array_equal(_mask(0.3, 17, (25, 40, 64)), full[:25])           # the mask of a prefix is the prefix of the mask
    assert np.array_equal(_mask(0.3, 17, (1, 1, 77)).reshape(-1), full.reshape(-1)[:77])
    assert _mask(0.0, 17).all() and not _mask(1.0, 17).any()
    x = torch.randn(N_ELEM, device=DEV)
    got = seqload.perturb(x, elem_p=0.3, seed=17)
    assert torch.equal(got, torch.where(torch.from_numpy(full).to(DEV), x, torch.zeros_like(x)))      # no rescaling
    start = torch.empty(N_ELEM[0], dtype=torch.int32, device=DEV)
    got = seqload.perturb(x, elem_p=0.999, seed=3, start_out=start)
    assert torch.equal(start, seqload.first_nonzero(got)) and (start > 0).any()


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5, 0.9])
def test_element_stream_statistics(p):
    n = int(np.prod(N_ELEM))
    assert n >= 10 ** 5
    a, b = _mask(p, 1234), _mask(p, 1235)
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"p={p}: kept {a.mean():.5f} and {b.mean():.5f}, expected {1 - p:.5f}, sigma {sigma:.5f}")
    assert abs(a.mean() - (1 - p)) <= 5 * sigma and abs(b.mean() - (1 - p)) <= 5 * sigma
    q = p * p + (1 - p) * (1 - p)                                # agreement of two independent streams
    agree = float((a == b).mean())
    print(f"p={p}: streams seed and seed + 1 agree on {agree:.5f}, independence {q:.5f}, sigma {math.sqrt(q * (1 - q) / n):.5f}")
    assert agree <= q + 5 * math.sqrt(q * (1 - q) / n)


def test_wrapper_refuses_what_the_kernel_cannot_take():
    from umlh import seqload
    x = torch.ones((3, 4, 5), device=DEV)
    with pytest.raises(ValueError, match="eps"):
        seqload.perturb(x, eps=torch.zeros(3, device=DEV))                    # float32 draws
    with pytest.raises(ValueError, match="keep"):
        seqload.perturb(x, keep=torch.ones(12, dtype=torch.uint8, device=DEV))   # per-step count without per_step
    with pytest.raises(ValueError, match="out"):
        seqload.perturb(x, out=torch.ones((3, 4, 6), device=DEV))
    flat = torch.ones(3 * 4 * 5 + 4, device=DEV)
    with pytest.raises(Exception, match="overlaps"):
        seqload.perturb(flat[:60].view(3, 4, 5), out=flat[4:64].view(3, 4, 5))
    with pytest.raises(Exception, match="elem_p"):
        seqload.perturb(x, elem_p=1.5)
    assert seqload.perturb(x, out=x) is x


# ---- multibench.robustness against the reference's noise function ----
@pytest.mark.parametrize("case", ["table", "list3", "table64", "steps"])
def test_add_timeseries_noise_is_the_reference_bit_for_bit(fx, case):
    from multibench import robustness
    arrays = RR.noise_inputs(fx, case)
    tables = [_dev(a, np.float32) for a in arrays]
    before = [t.clone() for t in tables]
    for li, p in enumerate(RR.LEVELS_P):
        got = robustness.add_timeseries_noise(tables, p, rand_drop=False, rng=int(fx[f"noise/{case}/seed"]) + li,
                                              per_step=case == "steps", table_dtype=[a.dtype for a in arrays])
        for g, w in zip(got, RR.noise_outputs(fx, case, li)):
            assert RR.same_bits(g.cpu().numpy(), w.astype(np.float32)), (case, p)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(tables, before))      # inputs are not modified


def test_the_three_steps_by_name(fx):
    from multibench import robustness
    x = [_dev(a) for a in RR.noise_inputs(fx, "list3")]
    e = robustness.draw_timeseries_noise([6, 6, 6], 0.3, struct_drop=False, rng=4)
    for g, a, (eps, _) in zip(robustness.white_noise(x, 0.3, rng=4), x, e):
        assert RR.same_bits(g.cpu().numpy(), RR.perturb(a.cpu().numpy(), eps)[0])
    k = robustness.draw_timeseries_noise([6, 6, 6], 0.5, gaussian_noise=False, rng=4)
    for g, a, (_, keep) in zip(robustness.structured_drop(x, 0.5, rng=4), x, k):
        assert RR.same_bits(g.cpu().numpy(), RR.perturb(a.cpu().numpy(), None, keep)[0])
    ones = [torch.ones(N_ELEM, device=DEV), torch.ones(N_ELEM, device=DEV)]
    a, b = robustness.random_drop(ones, 0.3, seed=17)
    assert np.array_equal(a.cpu().numpy() != 0, _mask(0.3, 17)) and np.array_equal(b.cpu().numpy() != 0, _mask(0.3, 18))
    full = robustness.add_timeseries_noise(x, 1.5, rng=0)                     # every step on, a level beyond 1: everything is dropped
    assert all((_bits(g.cpu().numpy()) == 0).all() for g in full)


# ---- the families against the reference ----
def _family_loaders(fx, case, family, **kw):
    from multibench.data import robust_loaders
    vision_norm, bs, seed = (int(v) for v in fx[f"fam/{case}/config"])
    data = {"test": RR.test_split(fx)}
    return robust_loaders(data, family, batch_size=bs, data_type="mosi", vision_norm=bool(vision_norm), device=DEV,
                          rng=seed + list(RR.FAMILIES).index(family), **kw)


@pytest.mark.parametrize("family", list(RR.FAMILIES))
def test_families_without_normalisation_are_the_reference_bit_for_bit(fx, family):
    levels = _family_loaders(fx, "plain", family)
    assert len(levels) == 10
    assert [len(levels[i].table) for i in range(10)] == fx[f"fam/plain/{family}/sizes"].tolist()
    for level in RR.RECORDED:
        ref = RR.family_batches(fx, "plain", family, level)
        got = list(levels[level])
        assert len(got) == len(ref)
        for batch, (xs, ls, inds, labels) in zip(got, ref):
            for m in range(3):
                assert R.same_bits(batch[0][m].cpu().numpy(), xs[m]), (family, level, m)
                assert np.array_equal(batch[1][m].cpu().numpy(), ls[m])
            assert np.array_equal(batch[2].numpy(), inds) and R.same_bits(batch[3].numpy(), labels)
    if family == "robust_timeseries":                            # the second drop: kept positions and ids follow it
        t = levels[9].table
        assert len(t) < 22 and t.ids.reshape(-1).tolist() == [100 + int(i) for i in t.kept] and 2 not in t.kept


@pytest.mark.parametrize("family", list(RR.FAMILIES))
def test_families_with_vision_norm_stay_inside_the_reference_error_bound(fx, family):
    levels = _family_loaders(fx, "vnorm", family)
    _, _, seed = (int(v) for v in fx["fam/vnorm/config"])
    st = RR.family_levels(RR.test_split(fx), family, seed + list(RR.FAMILIES).index(family))
    worst = 0.0
    for level in RR.RECORDED:
        table = RR.family_table(st[level], "mosi", True)
        ref = RR.family_batches(fx, "vnorm", family, level)
        got = list(levels[level])
        assert len(got) == len(ref) and np.array_equal(levels[level].table.kept, table["kept"])
        for batch, (xs, ls, inds, labels) in zip(got, ref):
            want = R.batch(table, inds.reshape(-1))
            worst = max(worst, R.rel_err(batch[0][0].cpu().numpy(), want[0][0]))
            for m in (1, 2):                                     # the unnormalised modalities stay bit-exact
                assert R.same_bits(batch[0][m].cpu().numpy(), xs[m]), (family, level, m)
            assert np.array_equal(batch[1][0].cpu().numpy(), ls[0]) and np.array_equal(batch[2].numpy(), inds)
            assert R.same_bits(batch[3].numpy(), labels)
    print(f"{family}: worst vision block 2^{np.log2(max(worst, 1e-30)):.1f} (bound 2^{RR.VNORM_BOUND_LOG2[family]})")
    assert worst <= RR.vnorm_bound(family)


@pytest.mark.parametrize("family", list(RR.FAMILIES))
def test_level_zero_is_the_clean_test_loader(fx, family):
    from multibench.data import AffectTable, SequenceLoader
    clean = list(SequenceLoader(AffectTable(RR.test_split(fx), data_type="mosi", device=DEV), 4))
    got = list(_family_loaders(fx, "plain", family)[0])
    assert len(got) == len(clean)
    noisy, signed = RR.FAMILIES[family][0], 0
    for a, b in zip(got, clean):
        for m in range(3):
            x, y = a[0][m].cpu().numpy(), b[0][m].cpu().numpy()
            assert np.array_equal(x, y) and torch.equal(a[1][m], b[1][m])
            minus_zero = np.signbit(y) & (y == 0)
            signed += int(minus_zero.sum())
            if m in noisy:                                       # x + 0.0: a -0.0 of the clean table becomes +0.0, nothing else moves
                assert np.array_equal(_bits(x), np.where(minus_zero, np.uint32(0), _bits(y)))
            else:
                assert np.array_equal(_bits(x), _bits(y))
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    print(f"{family}: {signed} elements -0.0 in the clean batches")


def test_per_step_loaders_follow_the_per_step_statement(fx):
    """``per_step=True``: the draws of one reference call per sample; the vision of every kept sample is the statement's."""
    levels = _family_loaders(fx, "plain", "robust_vision", per_step=True)
    split = RR.test_split(fx)
    kept = np.flatnonzero(R.first_rows(split["text"]) < split["text"].shape[1])
    rng = np.random.RandomState(int(fx["fam/plain/config"][2]))
    for level in range(4):
        want = RR.add_timeseries_noise([split["vision"][kept]], level / 10, rng, per_step=True)[0]
        if level == 3:
            got = levels[3].table
            assert len(got) == 22 and R.same_bits(got.tables[0].cpu().numpy(), want)
            assert ((want == 0).all(axis=2).any(axis=1) & ~(want == 0).all(axis=(1, 2))).any()    # rows dropped inside a sample


# ---- evaluate_robustness ----
def test_evaluate_robustness_against_evaluate(fx):
    from multibench.data import AffectTable, SequenceLoader, robust_loaders
    from multibench.models import Linear, Transformer, UML
    from multibench.train import evaluate, evaluate_robustness
    seq = R.load_fixture()
    data = {"train": R.fixture_split(seq, "toy_b", "train"), "valid": R.fixture_split(seq, "toy_b", "valid"), "test": RR.test_split(fx)}
    loaders = {s: SequenceLoader(AffectTable(data[s], data_type="mosi", device=DEV), 4) for s in data}
    cfg = {"train": list(loaders["train"]), "val": list(loaders["valid"]), "test": list(loaders["test"])}
    torch.manual_seed(3)
    z = 10
    model = UML(Linear(5, z), Linear(7, z), Transformer(z, z, nhead=5, num_layers=1, conv1d=True, out_last=False, pos_embd=True,
                                                      pos_learnable=False, max_len=128), [Linear(z, 5), Linear(z, 7)], modality="xy").to(DEV)
    base = evaluate(model, cfg, "mosi", device=DEV)
    robust = {f: robust_loaders(data, f, batch_size=4, device=DEV, rng=50 + i) for i, f in enumerate(RR.FAMILIES)}
    res = evaluate_robustness(model, cfg, robust, "mosi", device=DEV)
    print({k: v for k, v in res.items() if "mean" in k or k.endswith("/n")})
    assert set(res) == {f"robust/{f}/{k}" for f in RR.FAMILIES for k in ("score_x", "score_y", "score_xy", "loss_x", "loss_y", "n",
                                                                         "mean_score_x", "mean_score_y", "mean_score_xy")}
    for f in RR.FAMILIES:
        for k in ("score_x", "score_y", "score_xy", "loss_x", "loss_y"):
            assert len(res[f"robust/{f}/{k}"]) == 10 and all(np.isfinite(v) for v in res[f"robust/{f}/{k}"])
            assert res[f"robust/{f}/{k}"][0] == base[f"test/{k}"], (f, k)     # level 0 is the clean test set
        for k in ("x", "y", "xy"):
            assert res[f"robust/{f}/mean_score_{k}"] == float(np.mean(res[f"robust/{f}/score_{k}"]))
        assert res[f"robust/{f}/n"] == [len(robust[f][i].table) for i in range(10)]
    for k in ("score_x", "score_y", "score_xy", "loss_x", "loss_y"):          # the model reads modalities 0 and 2: audio noise is invisible
        assert len(set(res[f"robust/robust_audio/{k}"])) == 1, k
    assert res["robust/robust_audio/n"] == [22] * 10 and res["robust/robust_vision/n"] == [22] * 10
    assert min(res["robust/robust_timeseries/n"]) < 22 and res["robust/robust_timeseries/n"][0] == 22
    assert len(set(res["robust/robust_vision/loss_x"])) > 1 and len(set(res["robust/robust_timeseries/loss_y"])) > 1
    assert evaluate(model, cfg, "mosi", device=DEV) == pytest.approx(base, nan_ok=True, abs=0)       # and evaluate is what it was
    host = {f: [list(robust[f][i]) for i in range(2)] for f in ("robust_vision",)}                    # batch lists work as loaders do
    part = evaluate_robustness(model, cfg, host, "mosi", device=DEV)
    assert part["robust/robust_vision/score_xy"] == res["robust/robust_vision/score_xy"][:2]
    assert part["robust/robust_vision/loss_x"] == res["robust/robust_vision/loss_x"][:2]
