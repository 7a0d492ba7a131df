"""CPU: the linear-probe entry points of ABI revision 6 exist and reject bad arguments without a GPU; the float64
restatement (tests/_probe_ref.py) reproduces what the reference's evaluate_raw_data / evaluate recorded with sklearn
(tests/golden/probe_*.npz, scripts/make_golden_probe.py)."""
import ctypes as C

import numpy as np
import pytest

import _probe_ref as R
from conftest import load_golden

PROBE_CASES = ["mosi_a", "mosi_b", "mosei_a", "mosei_b", "humor_c"]
E2E_CASES = ["mosi", "humor"]
E_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_symbols_and_version(lib):
    from umlh._lib import EXPORTS
    for name in ("umlh_masked_mean", "umlh_probe_scratch_bytes", "umlh_probe_column_stats", "umlh_probe_fit", "umlh_probe_score"):
        assert name in EXPORTS and hasattr(lib, name), name
    assert lib.umlh_version() >= 6
    import umlh
    assert callable(umlh.masked_mean) and callable(umlh.LogisticProbe) and umlh.probe.KINDS == {"lbfgs": 0, "liblinear": 1}


def test_scratch_bytes(lib):
    sb = lib.umlh_probe_scratch_bytes
    for bad in ((1, 8, 40), (1 << 31, 8, 40), (100, 0, 40), (100, 1025, 40), (100, 8, -1), (100, 8, 1001), (-5, 8, 40)):
        assert sb(*bad) == 0, bad
    assert sb(2, 1, 1) > 0 and sb((1 << 31) - 1, 1024, 1000) > 0
    assert sb(1000, 40, 0) > 0                                      # max_iter = 0: the column statistics alone
    for d in (1, 40, 600, 1024):
        b = [sb(n, d, 40) for n in (1 << 12, 1 << 16, 1 << 20, 1 << 24)]
        assert b[0] <= b[1] < b[2] < b[3]
        # at most linear in N with a slope that does not know d: O(N) vectors only, no N x N and no N x d term
        slope = (b[3] - b[2]) / ((1 << 24) - (1 << 20))
        assert slope <= 21.0, (d, b)
    assert sb(1 << 24, 1024, 40) - sb(1 << 20, 1024, 40) == sb(1 << 24, 1, 40) - sb(1 << 20, 1, 40)


def test_invalid_arguments_need_no_gpu(lib):
    fake = C.c_void_p(4096)                                         # never dereferenced: the checks come first
    f64 = C.c_double

    def expect(rc, fn):
        assert rc == E_INVALID, fn
        assert fn.encode() in lib.umlh_last_error(), lib.umlh_last_error()

    mm = lib.umlh_masked_mean
    expect(mm(None, 2, 3, 4, 12, 4, None, fake, 4, None), "umlh_masked_mean")
    expect(mm(fake, 2, 3, 4, 12, 4, None, None, 4, None), "umlh_masked_mean")
    expect(mm(fake, 0, 3, 4, 12, 4, None, fake, 4, None), "umlh_masked_mean")
    expect(mm(fake, 2, 0, 4, 12, 4, None, fake, 4, None), "umlh_masked_mean")
    expect(mm(fake, 2, 3, 0, 12, 4, None, fake, 4, None), "umlh_masked_mean")
    expect(mm(fake, 2, 3, 4, 3, 4, None, fake, 4, None), "umlh_masked_mean")      # ldb < zdim
    expect(mm(fake, 2, 3, 4, 12, 3, None, fake, 4, None), "umlh_masked_mean")     # ldt < zdim
    expect(mm(fake, 2, 3, 4, 12, 4, None, fake, 3, None), "umlh_masked_mean")     # ldo < zdim

    cs = lib.umlh_probe_column_stats
    big = 1 << 30
    expect(cs(None, 10, 4, 4, fake, fake, big, None), "umlh_probe_column_stats")
    expect(cs(fake, 10, 4, 4, None, fake, big, None), "umlh_probe_column_stats")
    expect(cs(fake, 10, 4, 4, fake, None, big, None), "umlh_probe_column_stats")
    expect(cs(fake, 1, 4, 4, fake, fake, big, None), "umlh_probe_column_stats")
    expect(cs(fake, 10, 0, 4, fake, fake, big, None), "umlh_probe_column_stats")
    expect(cs(fake, 10, 1025, 1025, fake, fake, big, None), "umlh_probe_column_stats")
    expect(cs(fake, 10, 4, 3, fake, fake, big, None), "umlh_probe_column_stats")
    expect(cs(fake, 10, 4, 4, fake, fake, 8, None), "umlh_probe_column_stats")    # scratch too small

    fit = lib.umlh_probe_fit
    ok = dict(x=fake, n=100, d=8, ldx=8, y=fake, stats=None, kind=0, c=f64(1.0), max_iter=20, gtol=f64(0.0), coef=fake, rec=fake,
              obj=None, scratch=fake, nbytes=big, stream=None)
    for change in (dict(x=None), dict(y=None), dict(coef=None), dict(rec=None), dict(scratch=None), dict(n=1), dict(n=1 << 31),
                   dict(d=0), dict(d=1025, ldx=1025), dict(ldx=7), dict(kind=2), dict(kind=-1), dict(c=f64(0.0)), dict(c=f64(-1.0)),
                   dict(c=f64(float("nan"))), dict(c=f64(float("inf"))), dict(max_iter=0), dict(max_iter=1001),
                   dict(gtol=f64(-1.0)), dict(gtol=f64(float("nan"))), dict(nbytes=1024), dict(scratch=C.c_void_p(4100))):
        a = {**ok, **change}
        expect(fit(*a.values()), "umlh_probe_fit")

    sc = lib.umlh_probe_score
    expect(sc(None, 10, 4, 4, None, fake, fake, fake, None, None), "umlh_probe_score")
    expect(sc(fake, 10, 4, 4, None, None, fake, fake, None, None), "umlh_probe_score")
    expect(sc(fake, 10, 4, 4, None, fake, fake, None, None, None), "umlh_probe_score")    # nothing to compute
    expect(sc(fake, 10, 4, 4, None, fake, None, fake, None, None), "umlh_probe_score")    # a count without labels
    expect(sc(fake, 0, 4, 4, None, fake, fake, fake, None, None), "umlh_probe_score")
    expect(sc(fake, 10, 0, 4, None, fake, fake, fake, None, None), "umlh_probe_score")
    expect(sc(fake, 10, 4, 3, None, fake, fake, fake, None, None), "umlh_probe_score")


def test_python_wrappers_validate_before_the_gpu():
    import torch
    import umlh
    with pytest.raises(ValueError):
        umlh.LogisticProbe("newton")
    with pytest.raises(ValueError):
        umlh.LogisticProbe("lbfgs", C=0.0)
    with pytest.raises(ValueError):
        umlh.LogisticProbe("lbfgs", max_iter=0)
    with pytest.raises(ValueError):
        umlh.masked_mean(torch.zeros(3, 4))
    with pytest.raises(ValueError):
        umlh.masked_mean(torch.zeros(3, 4, 5, dtype=torch.int64))
    with pytest.raises(umlh.UmlhError):
        umlh.LogisticProbe().coef_


@pytest.mark.parametrize("tag", PROBE_CASES)
def test_restatement_reproduces_sklearn(tag):
    g = load_golden("probe_" + tag)
    kind, stats = int(g["kind"]), None
    if kind == R.LIBLINEAR:
        stats = R.column_stats(g["x_train"])
        np.testing.assert_allclose(stats[0], g["mean"], rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(stats[1], g["scale"], rtol=1e-13)
    w, it, mg = R.fit(g["x_train"], g["y_train"], kind, stats=stats)
    assert mg <= 1e-10 and it <= 40, (it, mg)
    np.testing.assert_allclose(w, g["w_star"], rtol=0, atol=1e-9)
    assert abs(np.abs(g["w_ref"] - w).max() - float(g["delta_ref"])) <= 1e-9
    # the recorded optimum is one: sklearn's own iterate sits above it
    xa = R._aug(R.standardise(g["x_train"], stats))
    y = g["y_train"].astype(np.float64)
    assert R.objective(w, xa, y, kind) <= R.objective(g["w_ref"], xa, y, kind)
    for split in ("val", "test"):
        xh, yh, n = g["x_" + split], g["y_" + split], len(g["y_" + split])
        flips = int(g["ref_flips_" + split])
        assert flips <= 0.01 * n
        assert int(((R.decision(w, xh, stats) > 0) != (R.decision(g["w_ref"], xh, stats) > 0)).sum()) == flips
        assert abs(R.score(w, xh, yh, stats) - float(g["score_ref_" + split])) <= flips / n + 1e-12
        assert R.decidable(w, xh, stats).all()                       # with the reference's arithmetic alone every sample is decidable
    if tag == "mosi_a":
        assert g["scale"][3] == 1.0 and np.ptp(g["x_train"][:, 3]) == 0 and np.abs(g["mean"]).max() > 5      # constant column, far means
    if tag == "mosi_b":
        assert g["x_train"].shape[1] > g["x_train"].shape[0] / 4
    raw = g["labels_raw_train"]
    lab = R.mosi_label(raw) if str(g["ds_name"]) in ("mosi", "mosei") else R.sarcasm_label(raw)
    assert np.array_equal(np.asarray(lab).reshape(-1).astype(int), g["y_train"])


@pytest.mark.parametrize("tag", E2E_CASES)
def test_end_to_end_fixture_raw_baselines(tag):
    """The recorded end-to-end fixtures are self-consistent (key sets, label maps), and evaluate_raw_data, which needs no
    model (a mean over time and three probes), is reproduced by the restatement up to the samples sklearn's own stopping
    tolerance can move: those whose float64 decision value is within the change its coefficient error causes."""
    g = load_golden("probe_e2e_" + tag)
    ds = str(g["ds_name"])
    kind = R.LIBLINEAR if ds == "mosi" else R.LBFGS
    label = R.mosi_label if ds in ("mosi", "mosei") else R.sarcasm_label
    for t in ("train", "val", "test"):
        assert np.array_equal(np.asarray(label(g["labels_" + t])).reshape(-1).astype(int), g["y01_" + t])
        assert g["emb_x_" + t].shape == (len(g["y01_" + t]), 20) and g["emb_y_" + t].shape == g["emb_x_" + t].shape
    assert set(g["keys_raw"]) == {f"{t}/score_{k}_raw" for t in ("val", "test") for k in ("x", "y", "xy")}
    assert len(g["keys_eval"]) == 21 and sum(np.isnan(float(g["res::" + k])) for k in g["keys_eval"]) == 10
    feats = {t: (R.masked_mean(g["x_" + t]).astype(np.float32), R.masked_mean(g["y_" + t]).astype(np.float32))
             for t in ("train", "val", "test")}
    for name, pick in (("x", lambda a: a[0]), ("y", lambda a: a[1]), ("xy", lambda a: np.concatenate(a, axis=1))):
        xt = pick(feats["train"])
        stats = R.column_stats(xt) if kind == R.LIBLINEAR else None
        w, _, mg = R.fit(xt, g["y01_train"], kind, stats=stats)
        assert mg <= 1e-10
        for t in ("val", "test"):
            xh, n = pick(feats[t]), len(g["y01_" + t])
            # sklearn stops within about 1e-2 of the optimum at these sizes (the probe fixtures record up to 5e-2)
            near = int((np.abs(R.decision(w, xh, stats)) <= 5e-2 * np.linalg.norm(R._aug(R.standardise(xh, stats)), axis=1)).sum())
            assert abs(R.score(w, xh, g["y01_" + t], stats) - float(g[f"res::{t}/score_{name}_raw"])) <= near / n + 1e-12


def test_masked_mean_restatement_against_the_reference_formula():
    import torch
    rng = np.random.default_rng(0)
    z = rng.standard_normal((6, 9, 5)).astype(np.float32)
    lens = np.array([9, 1, 4, 7, 20, 2])
    zt, lt = torch.from_numpy(z), torch.from_numpy(lens)
    mask = (torch.arange(9).unsqueeze(0) < lt.unsqueeze(1)).unsqueeze(-1).expand_as(zt).float()      # train.py:120-122
    want = ((zt * mask).sum(dim=1) / mask.sum(dim=1)).numpy()
    got = R.masked_mean(z, lens)
    assert (np.abs(got - want) <= R.masked_mean_bound(z, lens) + 1e-12).all()
    assert np.isnan(R.masked_mean(z, np.array([0, 1, 1, 1, 1, 1]))[0]).all()
    np.testing.assert_allclose(R.masked_mean(z), z.astype(np.float64).mean(1), rtol=1e-14, atol=1e-16)


@pytest.mark.parametrize("tag", E2E_CASES)
def test_restated_pooling_matches_the_reference_embeddings(tag):
    """The reference's pooled embeddings against the restated masked mean of the token embeddings it pooled."""
    g = load_golden("probe_e2e_" + tag)
    for t in ("train", "val", "test"):
        for m in ("x", "y"):
            z, lens, want = g[f"z{m}_{t}"], g[f"l{m}_{t}"], g[f"emb_{m}_{t}"]
            assert want.dtype == np.float32 and np.isfinite(want).all() and lens.min() == 1 and lens.max() == z.shape[1]
            got = R.masked_mean(z, lens)
            assert (np.abs(got - want) <= R.masked_mean_bound(z, lens) + 1e-12).all(), (t, m, np.abs(got - want).max())


def test_label_maps_on_edge_values():
    import torch
    from multibench.train import mosi_label, sarcasm_label
    y = np.array([0.0, -0.0, -1.0, 1.0, -1e-30, 3.5], dtype=np.float32)
    assert mosi_label(y).tolist() == [1, 1, 0, 1, 0, 1]
    assert mosi_label(torch.from_numpy(y)).tolist() == [1, 1, 0, 1, 0, 1]
    assert y.tolist() == pytest.approx([0.0, -0.0, -1.0, 1.0, -1e-30, 3.5])          # the input is not written
    assert np.array_equal(R.mosi_label(y), mosi_label(y).astype(np.int64))
    s = np.array([-1, 1, 0, -1])
    assert sarcasm_label(s).tolist() == [0, 1, 0, 0] and s.tolist() == [-1, 1, 0, -1]
    assert sarcasm_label(torch.tensor([-1.0, 1.0, -0.0])).tolist() == [0.0, 1.0, -0.0]
    assert np.array_equal(R.sarcasm_label(s), sarcasm_label(s))


def test_evaluate_rejects_the_datasets_the_reference_rejects():
    from multibench.train import evaluate, evaluate_raw_data
    for name in ("mimic", "avmnist", ""):
        with pytest.raises(NotImplementedError, match="Dataset not implemented yet"):
            evaluate_raw_data({"train": [], "val": [], "test": []}, name)
        with pytest.raises(NotImplementedError, match="Dataset not implemented yet"):
            evaluate(None, {"train": [], "val": [], "test": []}, name)
