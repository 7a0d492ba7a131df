"""No-GPU checks of the MIMIC loader (multibench/mimic.py, umlh/seqload.py, umlh_kernels_tabular.hip):

  * the float64 statement of tests/_mimic_ref.py against the fixture tests/golden/mimic*.npz, which the reference's own loader
    wrote: standardised tables, split, labels, the batch order of two train epochs and the noise levels 0, 3 and 10, bit for bit;
  * seven deliberately wrong statements, each of which differs from the fixture;
  * the host code of multibench.mimic: ``labels_for_task``, ``split_indices`` (and the global ``random`` state it must not
    touch), ``draw_mimic_noise`` against the recorded levels, also with one family disabled;
  * the C ABI: exported, in the header and the prototype table, the loader section still the last, every bad argument refused
    before any HIP call with the function and the argument named."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import _mimic_ref as R


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


def _test_rows(fx, case):
    idx = fx[f"{case}/split/test"]
    return fx[f"{case}/std/static"][idx], fx[f"{case}/std/series"][idx]


# ---- the statement against the fixture ----
@pytest.mark.parametrize("case", R.CASES)
def test_fixture_holds_what_it_must(fx, case):
    n, bs, _, _ = R.config(fx, case)
    df = R.datafile(fx, case)
    assert n % 5 and n % 10 and df["adm_features_all"].shape == (n, 5) and df["ep_tdata"].shape == (n, 24, 12)
    assert df["adm_features_all"].dtype == np.float64 and df["ep_tdata"].dtype == np.float64
    for a in (df["adm_features_all"], df["ep_tdata"]):
        assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any()
    xs, xt = R.clean(df["adm_features_all"]), R.clean(df["ep_tdata"]).reshape(-1, 12)
    const = (xs.std(0) == 0, xt.std(0) == 0)
    assert const[0].sum() == const[1].sum() == (1 if case == "const31" else 0)
    with np.errstate(all="ignore"):
        ratio = max((np.abs(xs.mean(0)) / xs.std(0))[~const[0]].max(), (np.abs(xt.mean(0)) / xt.std(0))[~const[1]].max())
    assert 4.0 < ratio <= 8.0                                   # column means far from 0, within the 8 std the GPU bound assumes
    assert set(np.unique(fx[f"{case}/labels/7/train"])) == {0, 1}
    if case != "const31":
        assert len(np.unique(np.concatenate([fx[f"{case}/labels/-1/{s}"] for s in ("train", "valid", "test")]))) == 6


@pytest.mark.parametrize("case", R.CASES)
def test_statement_reproduces_the_reference_tables_split_and_labels(fx, case):
    n, _, _, _ = R.config(fx, case)
    df = R.datafile(fx, case)
    static, series = R.standardize(df)
    assert R.same_bits(static, fx[f"{case}/std/static"]) and R.same_bits(series, fx[f"{case}/std/series"])
    sp = R.split(n)
    for name in ("valid", "test", "train"):
        assert sp[name] == fx[f"{case}/split/{name}"].tolist()
        for task in (7, -1):
            want = fx[f"{case}/labels/{task}/{name}"]
            got = R.labels(df, task)[sp[name]]
            assert np.array_equal(got, want) and got.dtype == df["y_icd9" if task >= 0 else "adm_labels_all"].dtype


@pytest.mark.parametrize("case", R.CASES)
def test_batch_order_of_both_epochs(fx, case):
    from multibench.data import SequenceSampler
    n, bs, _, tseed = R.config(fx, case)
    train = np.asarray(R.split(n)["train"])
    static, series = R.standardize(R.datafile(fx, case))
    for name in ("plain", "shuffled"):
        torch.manual_seed(tseed)
        batches = list(SequenceSampler(len(train), bs, shuffle=name == "shuffled"))
        assert [len(b) for b in batches] == fx[f"{case}/epoch/{name}/sizes"].tolist()
        assert train[[i for b in batches for i in b]].tolist() == fx[f"{case}/epoch/{name}/index"].tolist()
        for which, b in (("first", batches[0]), ("last", batches[-1])):
            assert R.same_bits(static[train[b]], fx[f"{case}/epoch/{name}/{which}/static"])
            assert R.same_bits(series[train[b]], fx[f"{case}/epoch/{name}/{which}/series"])
            assert np.array_equal(R.labels(R.datafile(fx, case), 7)[train[b]], fx[f"{case}/epoch/{name}/{which}/labels"])
    assert fx[f"{case}/epoch/shuffled/index"].tolist() != fx[f"{case}/epoch/plain/index"].tolist()


@pytest.mark.parametrize("case", R.CASES)
def test_statement_reproduces_the_noise_levels_bit_for_bit(fx, case):
    _, _, seed, _ = R.config(fx, case)
    static, series = _test_rows(fx, case)
    got = R.levels(static, series, seed)
    for k in R.RECORDED:
        assert R.same_values(got[k][0], fx[f"{case}/level/{k}/static"]), k
        assert R.same_values(got[k][1], fx[f"{case}/level/{k}/series"]), k
        assert np.array_equal(fx[f"{case}/level/{k}/labels"], fx[f"{case}/labels/7/test"])
    finite = ~np.isnan(static)
    assert (fx[f"{case}/level/10/static"] == 0).all() and (fx[f"{case}/level/10/series"] == 0).all()      # p = 1 drops everything
    assert np.array_equal(fx[f"{case}/level/0/static"][finite], static[finite])


def _differs(fx, case, variant):
    n, _, seed, _ = R.config(fx, case)
    if variant in ("sample_std", "stats_before_clean"):
        static, series = R.standardize(R.datafile(fx, case), variant)
        return not (R.same_values(static, fx[f"{case}/std/static"]) and R.same_values(series, fx[f"{case}/std/series"]))
    static, series = _test_rows(fx, case)
    got = R.levels(static, series, seed, variant)
    return not all(R.same_values(got[k][0], fx[f"{case}/level/{k}/static"]) and R.same_values(got[k][1], fx[f"{case}/level/{k}/series"])
                   for k in R.RECORDED)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_wrong_statements_are_caught(fx, variant):
    assert len(R.VARIANTS) >= 7
    # the order of drop and carry shows only in a row where a carrying column or its left neighbour is dropped: level 3 of the
    # six test rows of n57 holds no such row, the twenty of n203 do
    for case in ("n203",) if variant == "carry_before_drop" else ("n57", "n203"):
        assert _differs(fx, case, variant), (variant, case)
        assert not _differs(fx, case, None), case


# ---- the host code of multibench.mimic ----
@pytest.mark.parametrize("case", R.CASES)
def test_split_indices_and_labels_for_task(fx, case):
    from multibench.mimic import labels_for_task, split_indices
    n, _, _, _ = R.config(fx, case)
    random.seed(12345)
    state = random.getstate()
    valid, test, train = split_indices(n)
    assert random.getstate() == state                              # the global stream is untouched
    assert (valid, test, train) == tuple(fx[f"{case}/split/{s}"].tolist() for s in ("valid", "test", "train"))
    df = R.datafile(fx, case)
    before = {k: v.copy() for k, v in df.items()}
    for task in (7, -1):
        y = labels_for_task(df, task)
        for name, idx in (("valid", valid), ("test", test), ("train", train)):
            assert np.array_equal(y[idx], fx[f"{case}/labels/{task}/{name}"])
    assert all(R.same_bits(df[k], before[k]) for k in df)          # the caller's arrays stay as they were
    assert np.array_equal(labels_for_task(df, -1), R.labels(df, -1)) and np.array_equal(labels_for_task(df, 3), R.labels(df, 3))


def _module_levels(static, series, drawn):
    out = []
    for lv in drawn:
        st = static.copy() if lv["drop"] is None else R.tabular(static, lv["drop"], lv["carry"])
        se = series.copy() if lv["eps"] is None else R.series_noise(series, lv["eps"], lv["elem"], lv["keep"])
        out.append((st, se))
    return out


@pytest.mark.parametrize("case", R.CASES)
def test_draw_mimic_noise_gives_the_recorded_levels(fx, case):
    from multibench.mimic import draw_mimic_noise
    _, _, seed, _ = R.config(fx, case)
    static, series = _test_rows(fx, case)
    n = static.shape[0]
    drawn = draw_mimic_noise(n, rng=seed)
    assert len(drawn) == 11
    lv = drawn[3]
    assert lv["drop"].shape == (n, 5) and lv["carry"].shape == (n, 4) and lv["elem"].shape == (n, 288) and lv["keep"].shape == (n,)
    assert all(lv[k].dtype == np.uint8 for k in ("drop", "carry", "elem", "keep")) and lv["eps"].dtype == np.float64 and lv["eps"].shape == (n,)
    got = _module_levels(static, series, drawn)
    for k in R.RECORDED:
        assert R.same_values(got[k][0], fx[f"{case}/level/{k}/static"]) and R.same_values(got[k][1], fx[f"{case}/level/{k}/series"])
    np.random.seed(seed)                                           # rng=None: numpy's global legacy stream, as the reference
    again = draw_mimic_noise(n)
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(drawn, again) for k in a)


def test_a_disabled_family_draws_nothing(fx):
    from multibench.mimic import draw_mimic_noise
    _, _, seed, _ = R.config(fx, "n57")
    static, series = _test_rows(fx, "n57")
    n = static.shape[0]
    notab = draw_mimic_noise(n, tabular_robust=False, rng=seed)
    assert all(lv["drop"] is None and lv["carry"] is None and lv["eps"] is not None for lv in notab)
    got = _module_levels(static, series, notab)[3]
    assert R.same_values(got[0], fx["n57/notab/static"]) and R.same_values(got[1], fx["n57/notab/series"])
    nots = draw_mimic_noise(n, timeseries_robust=False, rng=seed)
    assert all(lv["eps"] is None and lv["elem"] is None and lv["keep"] is None and lv["drop"] is not None for lv in nots)
    got = _module_levels(static, series, nots)[3]
    assert R.same_values(got[0], fx["n57/nots/static"]) and R.same_values(got[1], fx["n57/nots/series"])
    assert not R.same_values(fx["n57/notab/series"], fx["n57/level/3/series"])      # the draws really moved
    rs = np.random.RandomState(5)
    state = rs.get_state()[1].copy()
    draw_mimic_noise(n, tabular_robust=False, timeseries_robust=False, rng=rs)
    assert np.array_equal(rs.get_state()[1], state)


def test_config_and_run_name():
    from multibench import mimic
    from multibench.data import DATASETS
    assert "mimic" not in DATASETS and not any(k.startswith("mimic") for k in DATASETS)
    assert (mimic.MIMIC["batch_size"], mimic.MIMIC["eval_batch_size"], mimic.MIMIC["indims"], mimic.MIMIC["task"]) == (128, 40, [5, 12], 7)


# ---- C ABI ----
NEW_NAMES = ["umlh_tab_standardize_scratch", "umlh_tab_standardize", "umlh_tab_perturb", "umlh_rows_gather"]
LOADER_NAMES = ["umlh_seq_first_nonzero", "umlh_seq_column_standardize_scratch", "umlh_seq_column_standardize", "umlh_seq_standardize",
                "umlh_seq_gather_pad"]


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_entry_points_are_exported_and_declared(lib):
    from test_abi_cpu import prototype_mismatches
    from umlh import _lib
    assert lib.umlh_version() == 11                              # additive
    names = list(_lib.PROTOTYPES)
    assert names[-len(LOADER_NAMES):] == LOADER_NAMES            # the loader section is still the last
    at = names.index("umlh_seq_perturb")
    assert names[at + 1:at + 1 + len(NEW_NAMES)] == NEW_NAMES    # behind the robustness section, in front of the loader's
    for name in NEW_NAMES:
        fn = getattr(lib, name)
        assert fn.restype is _lib.PROTOTYPES[name][0] and list(fn.argtypes) == list(_lib.PROTOTYPES[name][1]), name
        assert not name.endswith("_scratch_bytes")
    assert prototype_mismatches(_lib.PROTOTYPES) == []
    assert "umlh_kernels_tabular.hip" in _lib.SOURCES
    import os
    header = open(os.path.join(os.path.dirname(_lib._INCLUDE), "include", "umlh.h")).read()
    assert all(header.index(n + "(") < header.index("umlh_seq_first_nonzero(") for n in NEW_NAMES)
    assert "swap_entry" in header and "swaps nothing" in header


def test_scratch_query_is_the_column_standardize_plan(lib):
    q, old = lib.umlh_tab_standardize_scratch, lib.umlh_seq_column_standardize_scratch
    for rows in (1, 2, 255, 256, 257, 4097, 36000 * 24):
        for d in (1, 5, 12, 33):
            assert q(rows, d) == old(rows, d) and q(rows, d) % 256 == 0 and q(rows, d) >= 8 * min(rows, 256) * d
    assert q(0, 5) == 0 and q(5, 0) == 0 and q(1 << 40, 5) == 0 and q(5, (1 << 20) + 1) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: replayed only where no GPU is visible")
def test_refusals_come_before_any_hip_call(lib):
    E_INVALID = -1
    p = 1 << 20                                                   # a fake address: every call below is refused before it is used

    def refused(entry, args, *words):
        assert getattr(lib, entry)(*args) == E_INVALID, (entry, args)
        msg = lib.umlh_last_error().decode()
        assert msg.startswith(entry + ":") and all(w in msg for w in words), (entry, args, msg)

    def each(entry, base, changes):
        for i, value, words in changes:
            args = list(base)
            args[i] = value
            refused(entry, args, *words)

    need = lib.umlh_tab_standardize_scratch(264, 5)
    q = 8 * p                                                     # x, out, stats, scratch far apart
    for f64 in (0, 1):
        each("umlh_tab_standardize", [p, f64, 264, 5, 5, 2 * q, 5, 3 * q, 4 * q, need, None],
             [(0, None, ["null"]), (5, None, ["null"]), (7, None, ["null"]), (8, None, ["null"]), (2, 0, ["rows=0"]), (2, 1 << 40, ["rows="]),
              (3, 0, ["d=0"]), (3, (1 << 20) + 1, ["d="]), (4, 4, ["ldx=4"]), (6, 4, ["ldo=4"]), (9, need - 1, ["scratch", str(need)]),
              (8, 4 * q + 4, ["8-byte aligned"]), (1, 2, ["x_is_f64=2"])])
    # in place: fine for a float source with equal strides (refused here only for the scratch), never for a double source
    refused("umlh_tab_standardize", [p, 0, 264, 5, 5, p, 6, 3 * q, 4 * q, need, None], "in place", "ldo=6")
    refused("umlh_tab_standardize", [p, 0, 264, 5, 5, p, 5, 3 * q, 4 * q, need - 1, None], "scratch")
    refused("umlh_tab_standardize", [p, 1, 264, 5, 5, p, 5, 3 * q, 4 * q, need, None], "aliases", "double")
    for shift in (4, 4 * (263 * 5 + 5) - 4, -4 * (263 * 5 + 5) + 4):                             # a float out shifted against a float x
        refused("umlh_tab_standardize", [p, 0, 264, 5, 5, p + shift, 5, 3 * q, 4 * q, need, None], "overlaps", "partially")
    refused("umlh_tab_standardize", [p, 0, 264, 5, 7, p + 4 * (263 * 7 + 5) - 4, 5, 3 * q, 4 * q, need, None], "overlaps")      # padded rows count
    refused("umlh_tab_standardize", [p, 1, 264, 5, 5, p + 8 * (263 * 5 + 5) - 4, 5, 3 * q, 4 * q, need, None], "aliases")   # last word
    refused("umlh_tab_standardize", [p + 4 * (263 * 5 + 5) - 8, 1, 264, 5, 5, p, 5, 3 * q, 4 * q, need, None], "aliases")

    base = [p, 100, 5, 5, 3 * q, 4 * q, 0.0, 0.0, 0, 2 * q, 5, None]
    each("umlh_tab_perturb", base,
         [(0, None, ["null"]), (9, None, ["null"]), (1, 0, ["n=0"]), (1, 1 << 31, ["n="]), (2, 0, ["d=0"]), (2, (1 << 20) + 1, ["d="]),
          (3, 4, ["lds=4"]), (10, 4, ["ldd=4"]), (6, -0.1, ["p_drop"]), (6, 1.5, ["p_drop"]), (6, float("nan"), ["p_drop"]),
          (7, -0.1, ["p_carry"]), (7, 1.0001, ["p_carry"]), (7, float("nan"), ["p_carry"]),
          (9, p + 4, ["overlaps", "partially"]), (9, p + 4 * (99 * 5 + 5) - 4, ["overlaps"]), (9, p - 4 * (99 * 5 + 5) + 4, ["overlaps"])])
    args = list(base)
    args[9], args[10], args[3] = p, 7, 5                          # the same base with another stride is no in-place call
    refused("umlh_tab_perturb", args, "overlaps")
    args = list(base)
    args[9], args[1] = p, 0                                       # in place with equal strides is legal: refused for n only
    refused("umlh_tab_perturb", args, "n=0")

    srcs, outs = (C.c_void_p * 3)(p, 2 * p, 3 * p), (C.c_void_p * 3)(4 * p, 5 * p, 6 * p)
    widths = (C.c_int32 * 3)(5, 288, 7)
    base = [srcs, widths, 3, 22, p, 4, outs, None]
    each("umlh_rows_gather", base,
         [(0, None, ["null"]), (1, None, ["null"]), (6, None, ["null"]), (4, None, ["null"]), (2, 0, ["n_src=0"]), (2, 4, ["n_src=4"]),
          (3, 0, ["n=0"]), (3, 1 << 31, ["n="]), (5, 0, ["b=0"]), (5, 65536, ["b=65536"]),
          (1, (C.c_int32 * 3)(5, 0, 7), ["widths[1]=0"]), (1, (C.c_int32 * 3)(5, 288, -1), ["widths[2]=-1"]),
          (0, (C.c_void_p * 3)(None, None, None), ["every source is NULL"]),
          (6, (C.c_void_p * 3)(4 * p, None, 6 * p), ["source 1 has no destination"])])
    args = list(base)
    args[0], args[1], args[5] = (C.c_void_p * 3)(p, None, 3 * p), (C.c_int32 * 3)(5, -9, 7), 0      # a skipped source's width is not read
    refused("umlh_rows_gather", args, "b=0")
