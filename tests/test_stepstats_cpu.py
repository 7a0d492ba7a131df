"""CPU-side checks of the per-step logged statistics: the float64 statement of tests/_stepstats_ref.py against what the
reference's own train() logged (tests/golden/step_stats.npz, written by scripts/make_golden_stepstats.py), three deliberately
wrong statements that the same bound must tell apart, and the ABI v11 entry points: exported, and rejecting bad arguments
before any HIP call."""
import ctypes as C
import inspect

import numpy as np
import pytest

import _stepstats_ref as R
from conftest import load_golden

E_INVALID = -1
RUNS = ("mse", "nce")


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


@pytest.fixture(scope="module")
def golden():
    return load_golden("step_stats")


def _steps(g):
    """(run, step, x, lx, y, ly, y_recon, {key: logged value}) of every recorded training step."""
    for run in RUNS:
        for s in range(g[f"{run}::x"].shape[0]):
            logged = dict(zip(R.LOGGED_KEYS, g[f"{run}::logged"][s]))
            yield (run, s) + tuple(g[f"{run}::{k}"][s] for k in ("x", "lx", "y", "ly", "y_recon")) + (logged,)


def _rel(got, want):
    return abs(got - want) / abs(want)


def test_fixture_is_what_the_script_describes(golden):
    assert float(golden["bound"]) == R.BOUND
    assert set(golden) == {"bound"} | {f"{r}::{k}" for r in RUNS for k in ("x", "y", "lx", "ly", "y_recon", "logged")}
    for run in RUNS:
        assert golden[f"{run}::x"].shape == (3, 4, 6, 5) and golden[f"{run}::y"].shape == golden[f"{run}::y_recon"].shape == (3, 4, 6, 7)
        assert golden[f"{run}::logged"].shape == (3, len(R.LOGGED_KEYS))
        lens = np.concatenate([golden[f"{run}::lx"], golden[f"{run}::ly"]]).reshape(-1)
        assert {1, 6} <= set(lens.tolist()) and any(2 <= v <= 5 for v in lens)
        for k, l in (("x", "lx"), ("y", "ly")):                                      # rows past each length are zero
            for a, n in zip(golden[f"{run}::{k}"].reshape(-1, 6, golden[f"{run}::{k}"].shape[-1]), golden[f"{run}::{l}"].reshape(-1)):
                assert not a[n:].any() and a[:n].all()


def test_float64_statement_reproduces_every_logged_value(golden):
    n = 0
    for run, s, x, lx, y, ly, yr, logged in _steps(golden):
        sx, sy = R.step_stats(x, lx), R.step_stats(y, ly, yr)
        for key, got in (("train/trivial_loss_x", sx[0]), ("train/trivial_loss_y", sy[0]), ("train/recon_y_loss", sy[2])):
            rel = _rel(got, logged[key])
            print(f"{run} step {s} {key}: logged {logged[key]:.9g} float64 {got:.12g} rel {rel:.2e} (bound {R.BOUND:.2e})")
            assert rel <= R.BOUND, (run, s, key)
            n += 1
        assert sx[1] == 5 * np.minimum(lx, 5).sum() and sy[1] == 7 * np.minimum(ly, 5).sum() and sy[3] == 7 * (ly - 1).sum()
        assert sx[2] == 0.0 and sx[3] == 0.0
        t32, _ = R.reference_fp32(x, lx)                                             # the fp32 restatement of the reference's order
        assert _rel(float(t32), logged["train/trivial_loss_x"]) <= R.BOUND
        t32, r32 = R.reference_fp32(y, ly, yr)
        assert _rel(float(t32), logged["train/trivial_loss_y"]) <= R.BOUND and _rel(float(r32), logged["train/recon_y_loss"]) <= R.BOUND
    assert n == 18


@pytest.mark.parametrize("wrong", ["trivial_masked_by_next", "recon_masked_by_this", "denominator_without_d"])
def test_wrong_statements_miss_the_bound(golden, wrong):
    kw = {"trivial_masked_by_next": dict(trivial_mask="next"), "recon_masked_by_this": dict(recon_mask="this"),
          "denominator_without_d": dict(count_columns=False)}[wrong]
    for run, s, x, lx, y, ly, yr, logged in _steps(golden):
        sx, sy = R.step_stats(x, lx, **kw), R.step_stats(y, ly, yr, **kw)
        rels = {"train/trivial_loss_x": _rel(sx[0], logged["train/trivial_loss_x"]),
                "train/trivial_loss_y": _rel(sy[0], logged["train/trivial_loss_y"]),
                "train/recon_y_loss": _rel(sy[2], logged["train/recon_y_loss"])}
        hit = {"trivial_masked_by_next": ("train/trivial_loss_x", "train/trivial_loss_y"), "recon_masked_by_this": ("train/recon_y_loss",),
               "denominator_without_d": tuple(rels)}[wrong]
        for key in hit:
            print(f"{wrong} {run} step {s} {key}: rel {rels[key]:.2e}")
            assert rels[key] >= 8 * R.BOUND, (run, s, key)
        for key in set(rels) - set(hit):                                             # the other statistic is untouched
            assert rels[key] <= R.BOUND


def test_recon_y_loss_is_loss_y_under_the_mse_critic(golden):
    for run, s, *_, logged in _steps(golden):
        rel = _rel(logged["train/recon_y_loss"], logged["train/loss_y"])
        if run == "mse":
            assert rel <= R.BOUND, (s, rel)
        else:
            assert rel > 0.5                                                         # InfoNCE is another quantity altogether
        assert logged["train/loss_x_norm"] == abs(logged["train/loss_x"]) and logged["train/loss_y_norm"] == abs(logged["train/loss_y"])


def test_statement_edge_cases():
    g = np.random.default_rng(3)
    x, r = g.standard_normal((3, 1, 4)), g.standard_normal((3, 1, 4))
    assert R.step_stats(x, [1, 0, 5], r).tolist() == [0.0, 0.0, 0.0, 0.0]          # T = 1: no pair
    x, r = g.standard_normal((2, 4, 3)), g.standard_normal((2, 4, 3))
    got = R.step_stats(x, [-1, 9], r)                                                # clamped to 0 and T
    want = R.step_stats(x[1:], None, r[1:])
    assert np.array_equal(got, want) and got[1] == 9 and got[3] == 9
    x[0, 3] = np.inf                                                                 # row 3 > len 2 of sequence 0: excluded
    r[0, 1:] = np.inf                                                                # recon rows >= len - 1: excluded
    got = R.step_stats(x, [2, 4], r)
    assert np.isfinite(got).all() and got[1] == 3 * (2 + 3) and got[3] == 3 * (1 + 3)


def test_exports_and_version(lib):
    for name in ("umlh_seq_step_stats_scratch_bytes", "umlh_seq_step_stats"):
        assert hasattr(lib, name), name
    assert lib.umlh_version() == 11
    import umlh
    assert umlh.seq_step_stats is umlh.stepstats.seq_step_stats
    assert "umlh_kernels_stepstats.hip" in umlh._lib.SOURCES and "umlh_seq_step_stats" in umlh._lib.PROTOTYPES


def test_scratch_query(lib):
    q = lib.umlh_seq_step_stats_scratch_bytes
    for bad in ((0, 50, 35), (65536, 50, 35), (32, 0, 35), (32, 50, 0), (-1, 50, 35), (32, -2, 35), (32, 50, -7),
                (65535, 1 << 20, 35)):                                               # the last: more partial sums than the final takes
        assert q(*bad) == 0, bad
    for ok in ((1, 1, 1), (32, 50, 35), (128, 50, 371), (65535, 2, 1), (1, 1 << 20, 5000)):
        assert q(*ok) > 0 and q(*ok) % 256 == 0, ok
    assert q(32, 50, 35) == q(32, 65, 1024) < q(32, 66, 1024) == q(32, 65, 1025)     # 64 pair rows x 1024 columns per partial


def test_rejects_bad_arguments_before_touching_the_gpu(lib):
    fake = C.c_void_p(64)                                   # never dereferenced: the checks come first
    need = lib.umlh_seq_step_stats_scratch_bytes(4, 6, 7)
    ok = dict(x=fake, ldb=42, ldt=7, recon=fake, ldb_r=42, ldt_r=7, b=4, t_len=6, d=7, lengths=None, out4=fake, scratch=fake,
              scratch_bytes=need)
    for change, what in ((dict(x=None), b"null"), (dict(out4=None), b"null"), (dict(scratch=None), b"null"), (dict(b=0), b"b=0"),
                         (dict(b=65536), b"b=65536"), (dict(t_len=0), b"t_len=0"), (dict(d=0), b"d=0"), (dict(ldt=6), b"ldt=6"),
                         (dict(ldb=6), b"ldb=6"), (dict(ldb=41), b"overlap"), (dict(ldt_r=6), b"ldt_r=6"), (dict(ldb_r=6), b"ldb_r=6"),
                         (dict(ldb_r=30), b"ldb_r=30 ldt_r=7 overlap"), (dict(scratch_bytes=need - 1), b"scratch"),
                         (dict(b=65535, t_len=1 << 20, ldb=7 << 20), b"too large")):
        args = {**ok, **change}
        assert lib.umlh_seq_step_stats(*args.values(), None) == E_INVALID, change
        msg = lib.umlh_last_error()
        assert b"umlh_seq_step_stats" in msg and what in msg, (change, msg)
    args = {**ok, "recon": None, "ldb_r": 0, "ldt_r": 0, "x": None}                  # the recon strides are not looked at without recon
    assert lib.umlh_seq_step_stats(*args.values(), None) == E_INVALID and b"null" in lib.umlh_last_error()


def test_python_entry_point_checks_its_arguments():
    import torch
    import umlh
    with pytest.raises(ValueError, match="3-D"):
        umlh.seq_step_stats(torch.zeros(4, 5))
    with pytest.raises(ValueError, match="floating-point"):
        umlh.seq_step_stats(torch.zeros(2, 3, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="empty"):
        umlh.seq_step_stats(torch.zeros(0, 3, 4))
    with pytest.raises(ValueError, match="recon must be"):
        umlh.seq_step_stats(torch.zeros(2, 3, 4), recon=torch.zeros(2, 3, 5))
    with pytest.raises(ValueError, match="3 lengths for 2 sequences"):
        umlh.seq_step_stats(torch.zeros(2, 3, 4), lengths=[1, 2, 3])


def test_train_takes_step_diagnostics():
    from multibench.train import train
    p = inspect.signature(train).parameters
    assert "step_diagnostics" in p and p["step_diagnostics"].default is False
