"""CPU-side checks of the feature capture: the four class-statistics symbols and their prototypes, the argument checks of the
two entry points (every one of them precedes the first HIP call, so they run without a GPU), the reference module against
the golden run of the reference's own train(), and the host-side sampling helpers of finetune.py."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import _featcap_ref as R
from conftest import load_golden

E_INVALID = -1
SYMBOLS = ("umlh_class_index_scratch_bytes", "umlh_class_index", "umlh_class_stats_scratch_bytes", "umlh_class_stats")


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_the_four_symbols_are_exported(lib):
    import umlh
    from umlh import _lib
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES and name in _lib.EXPORTS
    assert "umlh_kernels_classstats.hip" in _lib.SOURCES
    assert umlh.class_index is umlh.capture.class_index and umlh.class_stats is umlh.capture.class_stats


def test_prototype_table_agrees_with_the_header():
    from test_abi_cpu import header_prototypes, prototype_mismatches
    from umlh import _lib
    hdr = header_prototypes()
    assert hdr["umlh_class_index_scratch_bytes"] == ("u64", ["i64", "i32"])
    assert hdr["umlh_class_index"] == ("i32", ["pointer", "i64", "i32", "pointer", "pointer", "pointer", "u64", "pointer"])
    assert hdr["umlh_class_stats_scratch_bytes"] == ("u64", ["i64", "i32", "i32"])
    assert hdr["umlh_class_stats"] == ("i32", ["pointer", "i64", "i64", "i32", "pointer", "pointer", "i32", "pointer", "i64", "pointer",
                                               "pointer", "pointer", "u64", "pointer"])
    assert prototype_mismatches(_lib.PROTOTYPES) == []


def test_scratch_queries_return_zero_on_bad_arguments(lib):
    assert lib.umlh_class_index_scratch_bytes(1000, 10) > 0
    for n, c in ((0, 10), (-5, 10), (1000, 0), (1000, -1), (1 << 31, 10), (1 << 30, 1 << 20)):     # last: over 2^28 block counts
        assert lib.umlh_class_index_scratch_bytes(n, c) == 0, (n, c)
    assert lib.umlh_class_stats_scratch_bytes(1000, 64, 10) > 0
    for n, d, c in ((0, 64, 10), (1000, 0, 10), (1000, 64, 0), (-1, 64, 10), (1000, -3, 10), (1 << 31, 64, 10)):
        assert lib.umlh_class_stats_scratch_bytes(n, d, c) == 0, (n, d, c)
    # the several-chunk path's partial sums: 2 n / 256 slots of d doubles
    assert lib.umlh_class_stats_scratch_bytes(70001, 24, 3) >= (2 * 70001 // 256) * 24 * 8


def _invalid(lib, rc, who, what):
    msg = lib.umlh_last_error()
    assert rc == E_INVALID, (who, what, rc, msg)
    assert who.encode() in msg and what.encode() in msg, (who, what, msg)


def test_class_index_rejects_every_invalid_argument_before_any_hip_call(lib):
    fake = C.c_void_p(256)                                  # never dereferenced: every check comes first
    need = lib.umlh_class_index_scratch_bytes(1000, 10)
    call = lambda labels=fake, n=1000, c=10, order=fake, offsets=fake, scratch=fake, nbytes=need: lib.umlh_class_index(
        labels, n, c, order, offsets, scratch, nbytes, None)
    who = "umlh_class_index"
    _invalid(lib, call(labels=None), who, "labels")
    _invalid(lib, call(order=None), who, "order")
    _invalid(lib, call(offsets=None), who, "offsets")
    _invalid(lib, call(scratch=None), who, "scratch")
    _invalid(lib, call(n=0), who, "n=0")
    _invalid(lib, call(n=1 << 31), who, "n=")
    _invalid(lib, call(c=0), who, "n_class=0")
    _invalid(lib, call(nbytes=need - 1), who, "scratch of")
    _invalid(lib, call(n=1 << 30, c=1 << 20), who, "n_class")


def test_class_stats_rejects_every_invalid_argument_before_any_hip_call(lib):
    n, d, c = 1000, 64, 10
    feats, means, other = C.c_void_p(1 << 20), C.c_void_p(1 << 30), C.c_void_p(256)     # far apart; never dereferenced
    need = lib.umlh_class_stats_scratch_bytes(n, d, c)

    def call(**kw):
        a = dict(feats=feats, ld=d, n=n, d=d, order=other, offsets=other, n_class=c, means=means, ld_means=d, dist=other, out2=other,
                 scratch=other, nbytes=need)
        a.update(kw)
        return lib.umlh_class_stats(a["feats"], a["ld"], a["n"], a["d"], a["order"], a["offsets"], a["n_class"], a["means"],
                                    a["ld_means"], a["dist"], a["out2"], a["scratch"], a["nbytes"], None)
    who = "umlh_class_stats"
    for name in ("feats", "order", "offsets", "means", "dist", "out2", "scratch"):
        _invalid(lib, call(**{name: None}), who, name)
    _invalid(lib, call(n=0), who, "n=0")
    _invalid(lib, call(d=0), who, "d=0")
    _invalid(lib, call(n_class=0), who, "n_class=0")
    _invalid(lib, call(ld=d - 1), who, "ld=63")
    _invalid(lib, call(ld_means=d - 1), who, "ld_means=63")
    _invalid(lib, call(nbytes=need - 1), who, "scratch of")
    # means inside, straddling the start of, and straddling the end of feats
    span = ((n - 1) * d + d) * 4
    for at in ((1 << 20) + 128, (1 << 20) - 64, (1 << 20) + span - 4):
        _invalid(lib, call(means=C.c_void_p(at)), who, "means overlaps feats")


# ---- the reference module against the reference's own run ----
def test_reference_module_reproduces_the_golden_inclass_distance_of_run_a():
    g = load_golden("feature_capture")
    feats, y, logged = g["A::file::all_iter_image_features"], g["A::file::all_iter_image_labels"], g["A::inclass_distance"]
    c = int(g["A::cfg"][2])
    assert feats.shape[0] == logged.shape[0] == 6 and np.all(logged > 0.1)
    order, offsets = R.class_index(y, c)
    worst = 0.0
    for s in range(feats.shape[0]):
        v32, per, means32 = R.reference_fp32(feats[s], y, c)
        m64, dist, o2, rows = R.class_stats(feats[s], order, offsets, c)
        rel = abs(o2[0] - logged[s]) / logged[s]
        worst = max(worst, rel)
        print(f"step {s}: logged {logged[s]:.9g} fp32 restatement {v32:.9g} float64 {o2[0]:.12g} rel {rel:.3e}")
        assert v32 == logged[s]                                  # the restatement IS the reference's arithmetic
        np.testing.assert_array_equal(per, g["A::inclass_per_class"][s])
        assert rel <= R.FP32_FORM_BOUND
        assert np.all(np.abs(means32 - m64) <= 2.0 ** -22)        # unit-norm rows: a few fp32 roundings of values below 1
    assert 8 * worst <= R.FP32_FORM_BOUND < 32 * worst           # the bound is the measured error x 8, rounded up to a power of two
    assert np.all(g["A::cka_score"] == 0) and np.all(g["A::mknn_score"] == 0)
    assert np.all(g["B::inclass_distance"] == 0) and np.all(g["B::cka_score"] > 0.1) and np.all(g["B::mknn_score"] > 0.5)


def test_class_index_reference_on_hand_cases():
    order, offsets = R.class_index([2, 0, -1, 2, 3, 0, 1], 3)
    assert order.tolist() == [1, 5, 6, 0, 3] and offsets.tolist() == [0, 2, 3, 5]
    rows = R.class_rows([4, -1, 7, 0, 2], [0, 3, 1, 9], 3, 5)     # stale: entries outside [0, 5), a decreasing offset, one past n
    assert [r.tolist() for r in rows] == [[4], [], [0, 2]]


@pytest.mark.parametrize("variant", sorted(R.WRONG))
def test_wrong_variants_break_the_gpu_bounds(variant):
    """Each deliberately wrong variant misses the float64 statement by at least 8 x the bound the GPU tests assert, on the
    GPU tests' own cases: a kernel that computed it would fail them."""
    hit = 0
    for name, (x, y, c) in R.stats_cases().items():
        order, offsets = R.class_index(y, c)
        m64, dist, o2, rows = R.class_stats(x, order, offsets, c)
        w_dist, w_o2 = R.WRONG[variant](x, rows)
        bad_d = R.broken(w_dist, dist, R.dist_rel_bound(x.shape[1], rows))
        bad_o = R.broken(w_o2[:1], o2[:1], (c + 4) * 2.0 ** -53)
        print(f"{variant} / {name}: classes broken {int(bad_d.sum())}/{c}, out2[0] broken {bool(bad_o[0])}")
        hit += int(bad_d.any() or bad_o[0])
    if variant == "empty classes skipped":
        assert hit >= 1                                           # only a case with an empty class can tell
    else:
        assert hit >= len(R.stats_cases()) - 2                    # (a single class IS all rows; d = 1 one-row classes are 0 either way)


# ---- host-side helpers of finetune.py ----
def test_train_signature_and_the_ignored_notice():
    import finetune as ft
    sig = inspect.signature(ft.train).parameters
    assert sig["capture_features_during_training"].default is False and "capture_samples" in sig and "features_pth" in sig
    assert inspect.signature(ft.setup_feature_run).parameters["capture_features_during_training"].default is False
    assert inspect.signature(ft.setup).parameters["capture_features_during_training"].default is False
    assert "(ignored)" not in inspect.getsource(ft)
    import feature_capture
    assert sorted(feature_capture.FILES.values()) == sorted(f"all_iter_{k}.pth" for k in (
        "image_raw_features", "image_features", "image_labels", "text_features", "text_labels"))


def test_take_capture_samples_takes_the_first_rows_of_each_class_in_table_order():
    import finetune as ft
    from engine.datasets.utils import FeatureLoader, FeatureTable
    g = load_golden("feature_capture")
    table = FeatureTable(torch.from_numpy(g["A::x_img"]), torch.from_numpy(g["A::y_img"]), "cpu")
    rows, labels = ft.take_capture_samples(FeatureLoader(table, 16, shuffle=True, kind="image"), shot=5)
    np.testing.assert_array_equal(rows.numpy(), g["A::sample_x"])
    np.testing.assert_array_equal(labels.numpy(), g["A::sample_y"])
    rows, labels = ft.take_capture_samples(FeatureLoader(table, 16, kind="image"), shot=100)
    np.testing.assert_array_equal(labels.numpy(), g["A::y_img"])


def test_get_n_text_features_consumes_the_loader_as_the_reference_does():
    import finetune as ft
    from engine.datasets.utils import FeatureLoader, FeatureTable
    from engine.tools.utils import set_random_seed
    x, y = torch.arange(40, dtype=torch.float32).reshape(20, 2), torch.arange(20)
    loader = FeatureLoader(FeatureTable(x, y, "cpu"), 8, shuffle=True, kind="text")
    set_random_seed(3)
    want = torch.cat([b[1] for b in loader])                      # one epoch under the same seed
    for n, rows in ((5, 5), (8, 8), (13, 13), (1000, 20)):
        set_random_seed(3)
        f, lab = ft.get_n_text_features(loader, n)
        assert f.shape == (rows, 2) and torch.equal(lab, want[:rows]) and torch.equal(f, x[lab])
    set_random_seed(3)
    ft.get_n_text_features(loader, 5)
    after = torch.empty((), dtype=torch.int64).random_().item()
    set_random_seed(3)
    next(iter(loader))
    assert after == torch.empty((), dtype=torch.int64).random_().item()     # two draws: the iterator's and the sampler's seed
