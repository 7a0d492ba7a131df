"""No-GPU checks of the affect datasets' device loader (multibench/data.py, umlh/seqload.py, umlh_kernels_seqload.hip):

  * order: ``SequenceSampler`` against ``torch.utils.data.DataLoader`` itself (shuffle, generator seeded 42), alone and as two
    zipped samplers, for four epochs -- batch lists and the generator's final state -- and against the inds the reference's
    loaders recorded in the fixture;
  * the float64 statement of tests/_seqload_ref.py against the fixture tests/golden/seq_loader*.npz: bit for bit without
    normalisation, and with it the reference's own fp32 error, which sets the bound of the GPU tests;
  * the conditions the fixture must meet for that comparison to mean something, asserted on its inputs;
  * six deliberately wrong statements, each caught;
  * the C ABI: exported, in the prototype table, refusing bad arguments before any HIP call;
  * the unsupported options of the reference's loader raise with their name.

The reference's own fp32 error, max |ref32 - ref64| / max |ref64| over the blocks of a case (ref32: the recorded batches of the
reference's loader, ref64: the statement), measured on the fixture:
    toy_sarcasm_vnorm   2^-21.1      wide_sarcasm_vnorm  2^-18.2      (numpy's fp32 column mean and std over N*T rows)
    toy_mosei_znorm     2^-21.9      wide_mosei_znorm    2^-22.1      (torch's fp32 mean and std per sequence)
Times 8, rounded up to a power of two: the bounds 2^-18, 2^-15, 2^-18, 2^-19 of ``_seqload_ref.BOUND_LOG2`` that the GPU tests
hold the kernels to.  The cases without normalisation have error 0 and are compared bit for bit."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _seqload_ref as R

EPOCHS = 4


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


# ---- order ----
def _torch_loader(n, bs, seed=42):
    g = torch.Generator().manual_seed(seed)
    return torch.utils.data.DataLoader(range(n), batch_size=bs, shuffle=True, generator=g), g


def _sampler(n, bs, seed=42):
    from multibench.data import SequenceSampler
    g = torch.Generator().manual_seed(seed)
    return SequenceSampler(n, bs, shuffle=True, generator=g), g


@pytest.mark.parametrize("bs", [4, 2, 11])
def test_sampler_follows_torch_alone(bs):
    (dl, g_t), (s, g_s) = _torch_loader(22, bs), _sampler(22, bs)
    assert len(s) == len(dl)
    for _ in range(EPOCHS):
        assert [b for b in s] == [b.tolist() for b in dl]
        assert torch.equal(g_s.get_state(), g_t.get_state())


@pytest.mark.parametrize("bs", [4, 2, 11])
def test_sampler_follows_torch_zipped(bs):
    (d1, gt1), (d2, gt2) = _torch_loader(22, bs), _torch_loader(22, bs)
    (s1, gs1), (s2, gs2) = _sampler(22, bs), _sampler(22, bs)
    same = []
    for _ in range(EPOCHS):
        want = [(a.tolist(), b.tolist()) for a, b in zip(d1, d2)]
        got = [(a, b) for a, b in zip(s1, s2)]
        assert got == want
        assert torch.equal(gs1.get_state(), gt1.get_state()) and torch.equal(gs2.get_state(), gt2.get_state())
        same.append(all(a == b for a, b in got))
    # both loaders start from seed 42: identical orders in every epoch unless bs divides n, then only in epoch 0
    assert same == ([True] * EPOCHS if 22 % bs else [True] + [False] * (EPOCHS - 1))


def test_sampler_deep_copy_replays_the_next_epoch():
    s, g = _sampler(22, 4)
    list(s)
    c = copy.deepcopy(s)
    state = g.get_state().clone()
    replay = [list(c), list(c)]
    assert torch.equal(g.get_state(), state)
    assert [list(s), list(s)] == replay


def test_sampler_unshuffled_and_len():
    from multibench.data import SequenceSampler
    for n, bs in ((22, 4), (22, 11), (9, 4), (3, 8), (1, 1)):
        s = SequenceSampler(n, bs)
        want = [list(range(i, min(i + bs, n))) for i in range(0, n, bs)]
        assert list(s) == want and list(s) == want and len(s) == len(want) == math.ceil(n / bs)
    with pytest.raises(ValueError):
        SequenceSampler(0, 4)


def test_sampler_without_generator_draws_from_the_global_one_as_torch_does():
    from multibench.data import SequenceSampler
    torch.manual_seed(7)
    want = [b.tolist() for b in torch.utils.data.DataLoader(range(22), batch_size=4, shuffle=True)]
    after = torch.get_rng_state()
    torch.manual_seed(7)
    assert list(SequenceSampler(22, 4, shuffle=True)) == want
    assert torch.equal(torch.get_rng_state(), after)


@pytest.mark.parametrize("case", ["toy_mosi", "toy_mosi_bs11", "wide_mosei_znorm"])
def test_sampler_gives_the_order_the_reference_recorded(fx, case):
    bs = int(fx[f"case/{case}/config"][4])
    s, _ = _sampler(22, bs)
    for epoch in ("train0", "train1"):
        assert [b for b in s] == [inds.reshape(-1).tolist() for _, _, inds, _ in R.fixture_batches(fx, case, epoch)]


# ---- the float64 statement against the fixture ----
def _config(fx, case):
    ds, data_type, zn, vn, bs = fx[f"case/{case}/config"]
    return str(ds), str(data_type), bool(int(zn)), bool(int(vn)), int(bs)


def _compare(fx, case, variant=None):
    """(worst relative error, all blocks bit-equal, structure equal) of the statement against the recorded batches of a case."""
    ds, data_type, zn, vn, _ = _config(fx, case)
    worst, bits, structure = 0.0, True, True
    for split, loaders in (("train", ("train0", "train1")), ("valid", ("valid",))):
        table = R.build_table(R.fixture_split(fx, ds, split), data_type, zn, vn, variant=variant)
        for loader in loaders:
            for xs, ls, inds, labels in R.fixture_batches(fx, case, loader):
                got = R.batch(table, inds.reshape(-1), variant=variant)
                for m in range(3):
                    structure &= got[0][m].shape == xs[m].shape and np.array_equal(got[1][m], ls[m])
                    bits &= R.same_bits(got[0][m], xs[m])
                    worst = max(worst, R.rel_err(xs[m], got[0][m]))
                structure &= np.array_equal(got[2], inds) and R.same_bits(got[3], labels) and labels.shape == (len(inds), 1)
    return worst, bits, structure


def test_fixture_holds_what_it_must(fx):
    assert list(fx["cases"]) == list(R.BOUND_LOG2)
    for ds in fx["datasets"]:
        train, valid = R.fixture_split(fx, ds, "train"), R.fixture_split(fx, ds, "valid")
        T = train["text"].shape[1]
        assert train["text"].shape[0] == 23 and valid["text"].shape[0] == 9
        assert (T, tuple(train[m].shape[2] for m in R.MODALITIES)) in ((12, (5, 4, 7)), (50, (130, 3, 67)))
        assert train["text"].dtype == np.float32 and valid["text"].dtype == np.float64           # a float64 split
        assert (valid["vision"].astype(np.float32) != valid["vision"]).any()                     # that fp32 cannot hold
        start = R.first_rows(train["text"])
        assert (start == T).sum() == 1 and (start == 0).any() and (start == T - 1).any()         # dropped, start 0, length 1
        assert np.isneginf(train["audio"]).sum() == 1
        front = np.arange(T)[None, :, None] < start[:, None, None]
        assert (np.signbit(train["text"]) & (train["text"] == 0) & front).any()                  # -0.0 in a front row
        nan = np.isnan(train["text"])
        assert nan.any() == str(ds).endswith("_a")
        if nan.any():                                                                            # the NaN decides a start
            i, t, _ = np.argwhere(nan)[0]
            assert start[i] == t and (np.nan_to_num(train["text"][i, t]) == 0).all()
    assert {_config(fx, c)[1:4] for c in fx["cases"]} == {("mosi", False, False), ("sarcasm", False, True), ("mosei", True, False)}
    assert 22 % _config(fx, "toy_mosi_bs11")[4] == 0 and all(_config(fx, c)[4] == 4 for c in fx["cases"] if c != "toy_mosi_bs11")


def test_fixture_meets_the_conditions_of_the_comparison(fx):
    """Under z_norm every (sample, column) is exactly constant with a value whose fp32 mean is exact (0 or a small integer), or has
    a sample std of at least 2^-3 of its largest magnitude; under vision_norm every vision column has sigma > 2^-3."""
    checked = 0
    for case in fx["cases"]:
        ds, data_type, zn, vn, _ = _config(fx, case)
        for split in ("train", "valid"):
            t = R.build_table(R.fixture_split(fx, ds, split), data_type)                          # dropped, -inf -> 0, untouched else
            if vn:
                rows = t["tables"][0].reshape(-1, t["tables"][0].shape[2])
                assert (rows.std(0) > 2.0 ** -3).all(), (case, split)
            if zn:
                for a in t["tables"]:
                    for i in range(a.shape[0]):
                        seq = a[i, t["start"][0][i]:]
                        const = (seq == seq[0]).all(0)
                        assert (np.abs(seq[0][const]) <= 8).all() and (seq[0][const] == np.round(seq[0][const])).all(), (case, split, i)
                        if seq.shape[0] > 1:
                            assert (seq[:, ~const].std(0, ddof=1) >= 2.0 ** -3 * np.abs(seq[:, ~const]).max(0)).all(), (case, split, i)
                        else:
                            assert const.all()
                        checked += seq.shape[1]
    assert checked > 1000


@pytest.mark.parametrize("case", ["toy_mosi", "toy_mosi_bs11", "wide_mosi"])
def test_statement_without_normalisation_is_the_reference_bit_for_bit(fx, case):
    worst, bits, structure = _compare(fx, case)
    assert structure and bits and worst == 0.0


@pytest.mark.parametrize("case", ["toy_sarcasm_vnorm", "wide_sarcasm_vnorm", "toy_mosei_znorm", "wide_mosei_znorm"])
def test_reference_fp32_error_sets_the_recorded_bound(fx, case):
    worst, _, structure = _compare(fx, case)
    print(f"{case}: reference fp32 error 2^{math.log2(worst):.1f}, bound 2^{R.BOUND_LOG2[case]}")
    assert structure and 0.0 < worst < 2.0 ** -16
    assert math.ceil(math.log2(8.0 * worst)) == R.BOUND_LOG2[case]
    assert R.bound(case) == 2.0 ** R.BOUND_LOG2[case]


def test_unnormalised_modalities_of_a_normalised_case_stay_bit_exact(fx):
    ds, data_type, zn, vn, _ = _config(fx, "wide_sarcasm_vnorm")
    table = R.build_table(R.fixture_split(fx, ds, "train"), data_type, zn, vn)
    for xs, _, inds, _ in R.fixture_batches(fx, "wide_sarcasm_vnorm", "train1"):
        got = R.batch(table, inds.reshape(-1))
        assert R.same_bits(got[0][1], xs[1]) and R.same_bits(got[0][2], xs[2])


def _caught(fx, case, variant):
    worst, bits, structure = _compare(fx, case, variant)
    return not structure or (worst > R.bound(case) if R.BOUND_LOG2[case] is not None else not bits)


@pytest.mark.parametrize("variant,cases", [
    ("biased_z", ["toy_mosei_znorm", "wide_mosei_znorm"]),
    ("unbiased_vision", ["toy_sarcasm_vnorm", "wide_sarcasm_vnorm"]),
    ("untrimmed_stats", ["toy_mosei_znorm", "wide_mosei_znorm"]),
    ("vision_with_dropped", ["toy_sarcasm_vnorm", "wide_sarcasm_vnorm"]),
    ("own_first_row", list(R.BOUND_LOG2)),
    ("lmax_T", list(R.BOUND_LOG2)),
])
def test_wrong_statements_are_caught(fx, variant, cases):
    assert variant in R.VARIANTS
    for case in cases:
        assert _caught(fx, case, variant), (variant, case)
    for case in R.BOUND_LOG2:                                   # and the right statement passes the same check everywhere
        assert not _caught(fx, case, None), case


# ---- C ABI ----
NEW_NAMES = ["umlh_seq_first_nonzero", "umlh_seq_column_standardize_scratch", "umlh_seq_column_standardize", "umlh_seq_standardize",
             "umlh_seq_gather_pad"]


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_entry_points_are_exported_and_declared(lib):
    from test_abi_cpu import prototype_mismatches
    from umlh import _lib
    assert lib.umlh_version() == 11                              # additive: callers detect the feature by its symbols
    assert list(_lib.PROTOTYPES)[-len(NEW_NAMES):] == NEW_NAMES  # the header's order: the section is its last
    for name in NEW_NAMES:
        fn = getattr(lib, name)
        assert fn.restype is _lib.PROTOTYPES[name][0] and list(fn.argtypes) == list(_lib.PROTOTYPES[name][1]), name
    assert prototype_mismatches(_lib.PROTOTYPES) == []
    assert "umlh_kernels_seqload.hip" in _lib.SOURCES


def test_column_standardize_scratch_is_a_layout_of_256_byte_regions(lib):
    q = lib.umlh_seq_column_standardize_scratch
    assert q(1100, 130) == 256 * 130 * 8 and q(3, 5) == 256 and q(813250, 35) == 256 * 35 * 8
    assert all(q(r, d) % 256 == 0 and q(r, d) >= 8 * min(r, 256) * d for r in (1, 2, 255, 256, 257, 10 ** 6) for d in (1, 5, 371))
    assert q(0, 5) == 0 and q(5, 0) == 0 and q(1 << 40, 5) == 0 and q(5, (1 << 20) + 1) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: replayed only where no GPU is visible")
def test_refusals_come_before_any_hip_call(lib):
    E_INVALID = -1
    p = 4096                                                     # a fake address: every call below is refused before it is used

    def refused(entry, args, *words):
        assert getattr(lib, entry)(*args) == E_INVALID, (entry, args)
        msg = lib.umlh_last_error().decode()
        assert msg.startswith(entry + ":") and all(w in msg for w in words), (entry, args, msg)

    def each(entry, base, changes):
        for i, value, words in changes:
            args = list(base)
            args[i] = value
            refused(entry, args, *words)

    each("umlh_seq_first_nonzero", [p, 22, 12, 7, p, None],
         [(0, None, ["null"]), (4, None, ["null"]), (1, 0, ["n=0"]), (1, 1 << 31, ["n="]), (2, 0, ["t_len=0"]), (3, 0, ["d=0"]),
          (3, (1 << 20) + 1, ["d="]), (2, 1 << 29, ["t_len * d"])])
    each("umlh_seq_standardize", [p, 22, 12, 7, p, None],
         [(0, None, ["null"]), (4, None, ["null"]), (1, 0, ["n=0"]), (2, -1, ["t_len=-1"]), (3, 0, ["d=0"])])
    need = lib.umlh_seq_column_standardize_scratch(264, 5)
    each("umlh_seq_column_standardize", [p, 264, 5, 5, p, 5, p, p, need, None],
         [(0, None, ["null"]), (4, None, ["null"]), (6, None, ["null"]), (7, None, ["null"]), (1, 0, ["rows=0"]), (2, 0, ["d=0"]),
          (3, 4, ["ldx=4"]), (5, 4, ["ldo=4"]), (5, 6, ["in place", "ldo=6"]), (8, need - 1, ["scratch", str(need)]),
          (7, p + 4, ["8-byte aligned"])])
    srcs, outs = (C.c_void_p * 3)(p, 2 * p, 3 * p), (C.c_void_p * 3)(4 * p, 5 * p, 6 * p)
    dims = (C.c_int32 * 3)(5, 4, 7)
    base = [srcs, dims, 3, 22, 12, p, p, 4, 12, outs, p, None]
    each("umlh_seq_gather_pad", base,
         [(0, None, ["null"]), (1, None, ["null"]), (9, None, ["null"]), (5, None, ["null"]), (6, None, ["null"]), (10, None, ["null"]),
          (2, 0, ["n_src=0"]), (2, 4, ["n_src=4"]), (3, 0, ["n=0"]), (4, 0, ["t_len=0"]), (7, 0, ["b=0"]), (7, 65536, ["b=65536"]),
          (8, 0, ["t_out=0"]), (1, (C.c_int32 * 3)(5, 0, 7), ["d=0"]), (8, 1 << 29, ["t_out * d"]),
          (0, (C.c_void_p * 3)(None, None, None), ["every source is NULL"]),
          (9, (C.c_void_p * 3)(4 * p, None, 6 * p), ["source 1 has no destination"])])
    # a NULL middle source is legal and its dims / outs entries are not read: what remains is refused for its own reasons only
    args = list(base)
    args[0], args[1], args[7] = (C.c_void_p * 3)(p, None, 3 * p), (C.c_int32 * 3)(5, -9, 7), 0
    refused("umlh_seq_gather_pad", args, "b=0")


# ---- host side ----
@pytest.mark.parametrize("option,value", [("aligned", False), ("flatten_time_series", True), ("max_pad", True),
                                          ("task", "classification"), ("robust_test", True)])
def test_unsupported_options_raise_with_their_name(option, value):
    from multibench import data
    for fn in (lambda: data.get_dataloader({}, **{option: value}), lambda: data.AffectTable({}, **{option: value})):
        with pytest.raises(NotImplementedError, match=option):
            fn()
    with pytest.raises(TypeError, match="shuffle_text"):
        data.get_dataloader({}, shuffle_text=True)


def test_dataset_table_is_the_reference_main():
    from multibench.data import DATASETS
    assert {k: (v["batch_size"], v["indims"], v["data_type"], v["vision_norm"]) for k, v in DATASETS.items()} == {
        "mosi": (32, [20, 300], "mosi", False), "sarcasm": (128, [371, 300], "sarcasm", True),
        "humor": (128, [371, 300], "humor", False), "mosei": (32, [35, 300], "mosei", False)}
