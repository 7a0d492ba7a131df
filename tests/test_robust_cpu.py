"""No-GPU checks of the robustness test sets (multibench/robustness.py, multibench.data.robust_loaders, umlh_seq_perturb):

  * ``draw_timeseries_noise`` plus the kernel contract of tests/_robust_ref.py reproduce, bit for bit, what the reference's own
    ``add_timeseries_noise`` gave (tests/golden/robust_noise.npz): one float32 table, a list of three float32 tables of different
    widths, one float64 table, and the per-step order (one call per sample on its [T, d] arrays), at levels 0, 0.3 and 1.0;
  * vectorised draws equal scalar draws, and ``rng=None`` consumes numpy's global state;
  * five deliberately wrong statements, each caught on the fixture;
  * the families' statement (first drop, noise, build) against every recorded batch of the reference's own
    drop_entry / add_timeseries_noise / Affectdataset / _process_1: bit for bit without normalisation, and with ``vision_norm``
    the reference's own fp32 error, which sets the bound of the GPU test;
  * the C ABI: exported, declared, refusing bad arguments before any HIP call; the refusals of the Python side.

Which sum the reference forms.  numpy adds the Python float of a draw to a float32 slice in float32 with the draw rounded to
float32 first, and to a float64 slice in float64 (checked below on the fixture, which was written by numpy 2.2.6; value-based
casting of numpy 1.x gives the same).  The kernel's one expression, float32(float64(x) + e), covers both: for two float32 values
the fp64 sum is exact when their exponents are at most 29 apart and otherwise leaves the larger one, so it rounds to float32 as
their float32 sum does; the draws only have to be rounded through float32 for a float32 table (``table_dtype``).  The variant
'fp32_add' (float32 add of a float32-rounded draw) is therefore the right answer on a float32 table and can only be told apart on
the float64 table and on the constructed case x = 1, e = 2^-24 + 2^-50: the fp64 sum rounds up to 1 + 2^-23, the fp32 form ties
to 1.

The reference's own fp32 error under vision_norm, max |ref32 - ref64| / max |ref64| over the blocks of the recorded levels
(ref32: the reference's batches, ref64: the statement), measured on the fixture:
    robust_vision 2^-18.5      robust_audio 2^-20.9      robust_timeseries 2^-20.7
(numpy's fp32 column mean and std over the N*T rows of the noisy vision table; at vision level 9 nine samples in ten are zero).
Times 8, rounded up to a power of two: 2^-15, 2^-17, 2^-17, ``_robust_ref.VNORM_BOUND_LOG2``."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _robust_ref as RR
import _seqload_ref as R

NOISE_CASES = ("table", "list3", "table64", "steps")


@pytest.fixture(scope="module")
def fx():
    return RR.load_fixture()


def _project(fx, case, li):
    """The project's host draws plus the kernel contract on one noise case and level: the float32 results."""
    from multibench.robustness import draw_timeseries_noise
    arrays = RR.noise_inputs(fx, case)
    rng = np.random.RandomState(int(fx[f"noise/{case}/seed"]) + li)
    counts = [(a.shape[0], a.shape[1]) if case == "steps" else a.shape[0] for a in arrays]
    draws = draw_timeseries_noise(counts, RR.LEVELS_P[li], rng=rng, table_dtype=[a.dtype for a in arrays])
    return [RR.perturb(a.astype(np.float32), eps, keep)[0] for a, (eps, keep) in zip(arrays, draws)], draws


def _restated(fx, case, li, variant=None):
    arrays = RR.noise_inputs(fx, case)
    rng = np.random.RandomState(int(fx[f"noise/{case}/seed"]) + li)
    return RR.add_timeseries_noise(arrays, RR.LEVELS_P[li], rng, per_step=case == "steps", variant=variant)


def _equal(got, want):
    return all(RR.same_bits(g, np.asarray(w).astype(np.float32)) for g, w in zip(got, want))


# ---- the noise function ----
def test_fixture_holds_what_it_must(fx):
    table = RR.noise_inputs(fx, "table")[0]
    assert table.dtype == np.float32 and np.isnan(table).any() and np.isposinf(table).any() and np.isneginf(table).any()
    assert (np.signbit(table) & (table == 0)).any() and ((table != 0) & (np.abs(table) < np.finfo(np.float32).tiny)).any()
    assert [a.shape[2] for a in RR.noise_inputs(fx, "list3")] == [2, 5, 1]
    t64 = RR.noise_inputs(fx, "table64")[0]
    assert t64.dtype == np.float64 and (t64.astype(np.float32) == t64).all()
    assert len(RR.noise_inputs(fx, "steps")) == 3 and all(a.dtype == np.float32 for a in RR.noise_inputs(fx, "steps"))
    for case in NOISE_CASES:                                     # level 0.3 drops some units and keeps some; level 1 drops all
        out = RR.noise_outputs(fx, case, 1)
        zero = [(o == 0).all(axis=-1) for o in out]
        assert any(z.any() for z in zero) and not all(z.all() for z in zero), case
        assert all((np.nan_to_num(o) == 0).all() and not np.isnan(o).any() for o in RR.noise_outputs(fx, case, 2)), case
    dropped_nan = np.isnan(table) & (RR.noise_outputs(fx, "table", 2)[0] == 0)
    assert dropped_nan.any()                                     # an assignment: the NaN of a dropped unit is gone


@pytest.mark.parametrize("case", NOISE_CASES)
@pytest.mark.parametrize("li", [0, 1, 2])
def test_draws_and_statement_reproduce_the_reference_bit_for_bit(fx, case, li):
    got, draws = _project(fx, case, li)
    want = RR.noise_outputs(fx, case, li)
    assert _equal(got, want)
    assert all(np.signbit(g[g == 0]).sum() == 0 for g in got) if li == 2 else True     # dropped: +0.0, never -0.0
    if case == "table64":                                        # the reference's float64 sum itself, before its loader rounds it
        x, (eps, keep) = RR.noise_inputs(fx, case)[0], draws[0]
        assert np.array_equal(want[0], np.where(keep[:, None, None] != 0, x + eps[:, None, None], 0.0), equal_nan=True)


@pytest.mark.parametrize("case", NOISE_CASES)
def test_vectorised_draws_equal_scalar_draws(fx, case):
    from multibench.robustness import draw_timeseries_noise
    arrays = RR.noise_inputs(fx, case)
    per_step = case == "steps"
    for p in (0.0, 0.3, 1.0):
        a, b = np.random.RandomState(99), np.random.RandomState(99)
        counts = [(x.shape[0], x.shape[1]) if per_step else x.shape[0] for x in arrays]
        got = draw_timeseries_noise(counts, p, rng=a, table_dtype=np.float64)
        want = RR.draws([x.shape[0] for x in arrays], p, b, t_len=arrays[0].shape[1], per_step=per_step)
        for (e1, k1), (e2, k2) in zip(got, want):
            assert e1.dtype == np.float64 and k1.dtype == np.uint8 and e1.shape == e2.shape == k1.shape
            assert np.array_equal(e1, e2) and np.array_equal(k1, k2)
        assert a.random_sample() == b.random_sample()            # and both consumed the same number of draws


def test_steps_off_draw_nothing_and_rounding_follows_the_table_dtype():
    from multibench.robustness import draw_timeseries_noise
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    (eps, keep), = draw_timeseries_noise([5], 0.3, gaussian_noise=False, rng=a)
    assert eps is None and np.array_equal(keep, (~(b.random_sample(5) < 0.3)).astype(np.uint8))
    (eps, keep), = draw_timeseries_noise([5], 0.3, struct_drop=False, rng=a)
    raw = b.normal(0, 0.3, size=5)
    assert keep is None and np.array_equal(eps, raw.astype(np.float32).astype(np.float64)) and not np.array_equal(eps, raw)
    assert np.array_equal(draw_timeseries_noise([5], 0.3, rng=7, table_dtype=np.float64)[0][0], np.random.RandomState(7).normal(0, 0.3, size=5))


def test_rng_none_consumes_the_global_state():
    from multibench.robustness import draw_timeseries_noise
    state = np.random.get_state()
    try:
        np.random.seed(1234)
        got = draw_timeseries_noise([4, 6], 0.3, rng=None)
        after = np.random.random_sample()
        want_rng = np.random.RandomState(1234)
        want = draw_timeseries_noise([4, 6], 0.3, rng=want_rng)
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got, want))
        assert after == want_rng.random_sample()
    finally:
        np.random.set_state(state)


@pytest.mark.parametrize("counts", [[5, 5, 5], [(5, 4)] * 3], ids=["per_sample", "per_step"])
@pytest.mark.parametrize("as_state", [False, True], ids=["int_seed", "RandomState"])
def test_inner_draws_on_a_resolved_stream_equal_the_public_function(counts, as_state):
    """``robust_loaders`` and ``draw_mimic_noise`` resolve their stream once and call the inner function level after level:
    it must draw what ``draw_timeseries_noise`` draws, and leave the stream where that leaves it."""
    from multibench.robustness import _draw, _rng, draw_timeseries_noise
    seed, dtypes = 77, [np.float32, np.float64, np.float32]
    pub = np.random.RandomState(seed) if as_state else seed
    inner = _rng(np.random.RandomState(seed) if as_state else seed)
    assert isinstance(inner, np.random.RandomState) and _rng(inner) is inner and _rng(None) is np.random
    for p, gauss, drop in ((0.3, True, True), (0.5, True, False), (0.5, False, True)):
        want = draw_timeseries_noise(counts, p, gauss, drop, pub, dtypes)
        got = _draw(inner, counts, p, gauss, drop, dtypes)
        if not as_state:                                         # an int seed starts the public function afresh at every call
            inner = _rng(seed)
        for (e1, k1), (e2, k2) in zip(got, want):
            assert (e1 is None) == (e2 is None) == (not gauss) and (k1 is None) == (k2 is None) == (not drop)
            assert e1 is None or (e1.dtype == e2.dtype and e1.shape == e2.shape and e1.tobytes() == e2.tobytes())
            assert k1 is None or (k1.dtype == k2.dtype and k1.shape == k2.shape and k1.tobytes() == k2.tobytes())
    if as_state:                                                 # three calls on one stream: the same state afterwards
        assert np.array_equal(inner.get_state()[1], pub.get_state()[1]) and inner.get_state()[2] == pub.get_state()[2]
    ref = np.random.RandomState(seed)                            # and after one call, the state of a stream that drew as much
    draw_timeseries_noise(counts, 0.3, rng=ref, table_dtype=dtypes)
    one = _rng(seed)
    _draw(one, counts, 0.3, True, True, dtypes)
    assert np.array_equal(one.get_state()[1], ref.get_state()[1]) and one.get_state()[2] == ref.get_state()[2]


def test_draw_mimic_noise_equals_the_recorded_draws(golden_dir):
    """tests/golden/mimic_draws.npz was drawn by the code before the draw function was split (scripts/make_golden_mimic_draws.py):
    one stream through all levels, per level drop, carry, eps, elem, keep."""
    import os
    from multibench.mimic import draw_mimic_noise
    with np.load(os.path.join(golden_dir, "mimic_draws.npz"), allow_pickle=False) as z:
        want = {k: z[k] for k in z.files}
    assert len(want) == 15
    for rng in (11, np.random.RandomState(11)):
        drawn = draw_mimic_noise(7, levels=3, rng=rng)
        assert len(drawn) == 3
        for k, lv in enumerate(drawn):
            for key in ("drop", "carry", "eps", "elem", "keep"):
                w = want[f"{k}/{key}"]
                assert lv[key].dtype == w.dtype and lv[key].shape == w.shape and lv[key].tobytes() == w.tobytes(), (k, key)
    assert any(want[f"{k}/drop"].any() for k in (1, 2)) and want["2/eps"].any()        # the recording is not a trivial one


# ---- wrong statements ----
def _caught(fx, variant, cases):
    return any(not _equal(_restated(fx, case, li, variant), RR.noise_outputs(fx, case, li)) for case in cases for li in (0, 1, 2))


def test_the_right_statement_passes_the_check_that_catches_the_wrong_ones(fx):
    assert not _caught(fx, None, NOISE_CASES)


@pytest.mark.parametrize("variant,cases", [("per_step_noise", ("table", "list3", "table64")), ("shared_drop", ("list3",)),
                                           ("multiply_drop", ("table",)), ("fp32_add", ("table64",)),
                                           ("drops_first", ("table", "list3", "table64"))])
def test_wrong_statements_are_caught(fx, variant, cases):
    assert variant in RR.VARIANTS
    for case in cases:
        assert _caught(fx, variant, (case,)), (variant, case)


def test_fp32_add_is_what_numpy_does_on_a_float32_table_and_not_on_a_float64_one(fx):
    """See the module's docstring: on float32 tables the reference's sum IS the fp32 add of the fp32-rounded draw, and the
    kernel's fp64 expression with the rounded draw is the same number; on the float64 table it is not."""
    for case in ("table", "list3", "steps"):
        assert not _caught(fx, "fp32_add", (case,)), case
    assert _caught(fx, "fp32_add", ("table64",))
    x = np.ones((1, 1, 1), dtype=np.float32)
    e = np.array([2.0 ** -24 + 2.0 ** -50])
    assert RR.perturb(x, e)[0][0, 0, 0] == np.float32(1.0 + 2.0 ** -23)
    assert RR.perturb(x, e, variant="fp32_add")[0][0, 0, 0] == np.float32(1.0)
    rng = np.random.RandomState(0)                               # the equivalence the float32 path rests on, on random operands
    a = (rng.standard_normal(20000) * 2.0 ** rng.randint(-40, 40, 20000)).astype(np.float32)
    b = (rng.standard_normal(20000) * 2.0 ** rng.randint(-40, 40, 20000)).astype(np.float32)
    assert np.array_equal((a.astype(np.float64) + b.astype(np.float64)).astype(np.float32), a + b)


# ---- the families ----
def _family_compare(fx, case, family):
    """(worst relative error, all blocks bit-equal, structure equal) of the statement against the reference's recorded batches."""
    vision_norm, bs, seed = (int(v) for v in fx[f"fam/{case}/config"])
    levels = RR.family_levels(RR.test_split(fx), family, seed + list(RR.FAMILIES).index(family))
    worst, bits, structure = 0.0, True, True
    for level in RR.RECORDED:
        table = RR.family_table(levels[level], "mosi", bool(vision_norm))
        structure &= len(table["kept"]) == int(fx[f"fam/{case}/{family}/sizes"][level])
        for xs, ls, inds, labels in RR.family_batches(fx, case, family, level):
            got = R.batch(table, inds.reshape(-1))
            for m in range(3):
                structure &= got[0][m].shape == xs[m].shape and np.array_equal(got[1][m], ls[m])
                bits &= R.same_bits(got[0][m], xs[m])
                worst = max(worst, R.rel_err(xs[m], got[0][m]))
            structure &= R.same_bits(got[3], labels)
        n = sum(len(b[2]) for b in RR.family_batches(fx, case, family, level))
        structure &= n == len(table["kept"])
    return worst, bits, structure


def test_family_fixture_holds_what_it_must(fx):
    split = RR.test_split(fx)
    T = split["text"].shape[1]
    assert all(split[m].dtype == np.float32 for m in R.MODALITIES) and split["text"].shape[0] == 23
    assert (R.first_rows(split["text"]) == T).sum() == 1 and np.isneginf(split["audio"]).sum() == 1
    for case in ("plain", "vnorm"):
        sizes = fx[f"fam/{case}/robust_timeseries/sizes"]
        assert sizes[0] == 22 and min(sizes[3], sizes[9]) < 22   # a text dropped by the noise disappears
        assert (fx[f"fam/{case}/robust_vision/sizes"] == 22).all() and (fx[f"fam/{case}/robust_audio/sizes"] == 22).all()


@pytest.mark.parametrize("family", list(RR.FAMILIES))
def test_family_statement_is_the_reference_bit_for_bit(fx, family):
    worst, bits, structure = _family_compare(fx, "plain", family)
    assert structure and bits and worst == 0.0


@pytest.mark.parametrize("family", list(RR.FAMILIES))
def test_reference_fp32_error_sets_the_vision_norm_bound(fx, family):
    worst, _, structure = _family_compare(fx, "vnorm", family)
    print(f"{family}: reference fp32 error 2^{math.log2(worst):.1f}, bound 2^{RR.VNORM_BOUND_LOG2[family]}")
    assert structure and 0.0 < worst < 2.0 ** -16
    assert math.ceil(math.log2(8.0 * worst)) == RR.VNORM_BOUND_LOG2[family]


# ---- refusals ----
def test_robust_loaders_refuses_the_text_family_and_unknown_ones():
    from multibench import data
    with pytest.raises(NotImplementedError, match="GloVe"):
        data.robust_loaders({}, "robust_text")
    with pytest.raises(ValueError, match="robust_colour"):
        data.robust_loaders({}, "robust_colour")
    for fn in (lambda: data.get_dataloader({}, robust_test=True), lambda: data.AffectTable({}, robust_test=True)):
        with pytest.raises(NotImplementedError, match="robust_test"):
            fn()


def test_draw_arguments_are_checked():
    from multibench.robustness import draw_timeseries_noise
    with pytest.raises(TypeError, match="rng"):
        draw_timeseries_noise([3], 0.1, rng="seed")
    with pytest.raises(ValueError, match="dtypes"):
        draw_timeseries_noise([3, 3], 0.1, rng=0, table_dtype=[np.float32])
    with pytest.raises(ValueError, match="per-step"):
        draw_timeseries_noise([(3, 4), (2, 4)], 0.1, rng=0)


# ---- C ABI ----
@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_entry_point_is_exported_and_declared(lib):
    from test_abi_cpu import prototype_mismatches
    from umlh import _lib
    assert lib.umlh_version() == 11                              # additive
    fn = lib.umlh_seq_perturb
    assert fn.restype is _lib.PROTOTYPES["umlh_seq_perturb"][0] and list(fn.argtypes) == list(_lib.PROTOTYPES["umlh_seq_perturb"][1])
    assert prototype_mismatches(_lib.PROTOTYPES) == []


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: replayed only where no GPU is visible")
def test_refusals_come_before_any_hip_call(lib):
    E_INVALID = -1
    p = 1 << 20                                                  # fake addresses: every call below is refused before they are used
    base = [p, 22, 12, 7, 12, p, p, C.c_float(0.0), 0, 4 * p, p, None]
    for i, value, words in [(0, None, ["null"]), (9, None, ["null"]), (1, 0, ["n=0"]), (1, 1 << 31, ["n="]), (2, 0, ["t_len=0"]),
                            (3, 0, ["d=0"]), (3, (1 << 20) + 1, ["d="]), (4, 2, ["unit_rows=2"]), (4, 0, ["unit_rows=0"]),
                            (4, 24, ["unit_rows=24"]), (7, C.c_float(-0.1), ["elem_p"]), (7, C.c_float(1.5), ["elem_p"]),
                            (7, C.c_float(float("nan")), ["elem_p"]), (9, p + 4, ["overlaps"]), (9, p - 4, ["overlaps"]),
                            (9, p + 22 * 12 * 7 * 4 - 4, ["overlaps"])]:
        args = list(base)
        args[i] = value
        assert lib.umlh_seq_perturb(*args) == E_INVALID, (i, value)
        msg = lib.umlh_last_error().decode()
        assert msg.startswith("umlh_seq_perturb:") and all(w in msg for w in words), (i, value, msg)
