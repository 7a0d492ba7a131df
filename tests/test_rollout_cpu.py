"""CPU-side checks of the rollout and spectrum feature (no GPU): the float64 closed form of tests/_rollout_ref.py against what
the reference's own rollout() and analyze_spectral_bias() gave (tests/golden/rollout*.npz), the criterion table of
_rollout_ref re-measured, the conditions that keep a comparison from passing vacuously, deliberately wrong variants, and the
C ABI of the three new entry points: exported, prototyped, checking their arguments before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import _rollout_ref as R
from conftest import load_golden


@pytest.fixture(scope="module")
def golden():
    return load_golden("rollout")


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def golden_params(g, x_side, with_pos):
    sd = {k[3:]: g[k] for k in g.files if k.startswith("w::")}
    return R.params_from_state(sd, x_side, with_pos, int(g["n_layers"]), float(g["eps"]))


GOLDEN_CASES = [("case1", False, 4, 1, 5), ("case2", True, 3, 3, 8)]


@pytest.mark.parametrize("tag,with_pos,B,T0,steps", GOLDEN_CASES)
def test_closed_form_equals_the_reference_rollout(golden, tag, with_pos, B, T0, steps):
    assert int(golden[f"{tag}::steps"]) == steps
    for side, name in ((True, "x"), (False, "y")):
        seq, pred = golden[f"{tag}::{name}"], golden[f"{tag}::pred_{name}"]
        assert seq.shape[:2] == (B, T0) and pred.shape == (B, T0 + steps, seq.shape[2])
        assert np.array_equal(pred[:, :T0], seq)                       # the reference's cat: the input, then the generated frames
        ref = R.rollout(golden_params(golden, side, with_pos), seq[:, -1], steps)
        err = np.abs(pred[:, T0 - 1:] - ref).max() / np.abs(ref).max()
        print(f"{tag} {name}: closed form against the reference {err:.3e} (bound {float(golden['bound']):.3e})")
        assert err <= float(golden["bound"])


def test_spectrum_ref_equals_the_reference_spectra(golden):
    for name in ("x", "y"):
        for key, blk in ((f"spec::{name}_gt", golden[f"spec::{name}_block"]), (f"spec::{name}_pred", golden[f"case2::pred_{name}"])):
            want = golden[key]
            got = R.spectrum(blk)
            assert got.shape == want.shape == (blk.shape[1] // 2 + 1,)
            assert np.abs(got - want).max() / np.abs(got).max() <= float(golden["bound_spec"])


def test_golden_bounds_are_powers_of_two_at_fp32_level(golden):
    for k in ("bound", "bound_spec"):
        b = float(golden[k])
        assert np.log2(b) == int(np.log2(b)) and 2.0 ** -24 <= b <= 2.0 ** -14


def _wrong_golden(golden, what):
    """Error of a deliberately wrong restatement against the reference's case 2 (learnable positions, T0 = 3), x side."""
    seq, pred = golden["case2::x"], golden["case2::pred_x"]
    p = golden_params(golden, True, True)
    seed, variant = seq[:, -1], None
    if what == "first_frame":
        seed = seq[:, 0]
    elif what == "other_decoder":
        py = golden_params(golden, False, True)
        p = dict(p, w_out=py["w_out"][:p["w_out"].shape[0]], b_out=py["b_out"][:p["b_out"].shape[0]])
    else:
        variant = what
    got = R.rollout(p, seed, 8, variant=variant)
    return np.abs(pred[:, 3:] - got[:, 1:]).max() / np.abs(pred[:, 3:]).max()


# the golden model has nn's eps = 1e-5: dropping it moves the values by less than the fixture's fp32 bound, so that variant is
# held to the table's eps = 1e-2 case below
@pytest.mark.parametrize("what", tuple(v for v in R.VARIANTS if v != "no_eps") + ("first_frame", "other_decoder"))
def test_every_wrong_variant_breaks_the_golden_bound_by_8x(golden, what):
    err = _wrong_golden(golden, what)
    print(f"{what}: {err:.3e} = {err / float(golden['bound']):.1f} x bound")
    assert err >= 8 * float(golden["bound"])


def test_criterion_table_is_current():
    """Every row of _rollout_ref's table re-measured: the bound is 8 x the fp32 evaluation's error rounded up to a power of two
    (0.3 bits of slack for another BLAS), and no case is chaotic (worst error <= 64 x the step-1 error)."""
    import re
    rows = {m[1]: (float(m[2]), int(m[3])) for m in re.finditer(r"(\w+) +(\d\.\d\de-\d\d) +\d+\.\d +2\^(-\d+)", R.__doc__)}
    assert set(R.BOUNDS) == set(R.CASES)
    for name in R.CASES:
        if R.CASES[name][7] == 0:
            continue
        worst, growth = R.measure_fp32(name)
        print(f"{name}: fp32 {worst:.2e} growth {growth:.1f} bound 2^{int(np.log2(R.BOUNDS[name]))}")
        assert growth <= 64.0, name
        assert 8 * worst <= R.BOUNDS[name] * 2 ** 0.3 and R.BOUNDS[name] <= 32 * worst, name
        assert rows[name][1] == int(np.log2(R.BOUNDS[name])), name
        assert 0.5 <= rows[name][0] / worst <= 2.0, name


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c[6] > 1 and c[7] >= 1])
def test_rows_of_the_reference_stay_apart(name):
    """A comparison of collapsed rows would only see one trajectory: at generated steps 1-4 the rows differ by >= 1e-2 of
    max|ref|, and the long-horizon case keeps them apart to its last step."""
    p, x0, steps = R.make_case(name)
    ref = R.rollout(p, x0, steps)
    for s in range(1, min(steps, 4) + 1):
        assert R.row_spread(ref, s) >= 1e-2, (name, s)
    if name == R.LONG_CASE:
        assert steps == 49 and R.row_spread(ref, steps) >= 1e-2


@pytest.mark.parametrize("what", R.VARIANTS + ("first_frame", "other_decoder"))
def test_every_wrong_variant_breaks_a_table_bound_by_8x(what):
    name = "z10_d5_eps" if what == "no_eps" else "z10_d5_long"         # conv, learnable positions; eps = 1e-2 where eps is dropped
    p, x0, _ = R.make_case(name)
    steps, variant, seed = 4, None, x0
    rng = np.random.default_rng(5)
    if what == "first_frame":
        seed = rng.standard_normal(x0.shape).astype(np.float32)        # the first frame of a longer input
    elif what == "other_decoder":
        p = dict(p, w_out=(3.0 * rng.uniform(-1, 1, p["w_out"].shape) / np.sqrt(10)).astype(np.float32))
    else:
        variant = what
    e = R.step_errors(R.rollout(p, seed, steps, variant=variant), R.rollout(R.make_case(name)[0], x0, steps))
    assert e.max() >= 8 * R.BOUNDS[name], (what, e.max())


# ---- the C ABI ----
def test_new_symbols_are_exported_with_the_tables_prototypes(lib):
    from umlh import _lib
    for name in ("umlh_rollout", "umlh_seq_spectrum_scratch_bytes", "umlh_seq_spectrum"):
        assert name in _lib.PROTOTYPES, name
        fn = getattr(lib, name)
        assert fn.restype is _lib.PROTOTYPES[name][0] and list(fn.argtypes) == list(_lib.PROTOTYPES[name][1]), name
    assert lib.umlh_seq_spectrum_scratch_bytes.restype is C.c_uint64
    assert lib.umlh_version() == 11                                    # additive: callers detect the feature by its symbols
    assert C.sizeof(_lib.RolloutCfg) == 24


def _rollout_call(lib, cfg=(40, 2048, 35, 1, 4, 1e-5), n=4, ldx=35, ldb=5 * 35, ldt=35, null=None, layers=True):
    from umlh._lib import RolloutCfg
    fake = C.c_void_p(64)                                              # never dereferenced: the checks come first
    c = RolloutCfg(*cfg)
    P = (C.c_void_p * max(12 * cfg[3], 1))(*([64] * max(12 * cfg[3], 1))) if layers else None
    args = {k: fake for k in ("w_in", "b_in", "w_out", "b_out", "x0", "out")}
    if null:
        args[null] = None
    return lib.umlh_rollout(C.byref(c), P, None, None, args["w_in"], args["b_in"], args["w_out"], args["b_out"], args["x0"], ldx, n,
                            args["out"], ldb, ldt, None)


@pytest.mark.parametrize("kw,what", [
    (dict(cfg=(513, 2048, 35, 1, 4, 1e-5)), b"Z=513"), (dict(cfg=(0, 2048, 35, 1, 4, 1e-5)), b"Z=0"),
    (dict(cfg=(40, 2049, 35, 1, 4, 1e-5)), b"d_ff=2049"), (dict(cfg=(40, 2048, 1025, 1, 4, 1e-5), ldx=1025, ldt=1025, ldb=5 * 1025), b"D=1025"),
    (dict(cfg=(40, 2048, 35, 17, 4, 1e-5)), b"n_layers=17"), (dict(cfg=(40, 2048, 35, 1, 4097, 1e-5), ldb=4098 * 35), b"steps=4097"),
    (dict(cfg=(40, 2048, 35, 1, -1, 1e-5)), b"steps=-1"), (dict(cfg=(40, 2048, 35, 1, 4, -1.0)), b"eps"),
    (dict(n=0), b"n=0"), (dict(n=(1 << 20) + 1), b"n=1048577"), (dict(ldx=34), b"ldx=34"), (dict(ldt=34), b"ldt=34"),
    (dict(ldb=5 * 35 - 1), b"ldb=174"), (dict(null="x0"), b"null pointer"), (dict(null="w_out"), b"null pointer"),
    (dict(layers=False), b"P is NULL"),
])
def test_rollout_rejects_bad_arguments_before_touching_the_gpu(lib, kw, what):
    assert _rollout_call(lib, **kw) == -1
    msg = lib.umlh_last_error()
    assert b"umlh_rollout" in msg and what in msg, msg


def test_rollout_rejects_null_cfg_and_null_layer_tensor(lib):
    fake = C.c_void_p(64)
    assert lib.umlh_rollout(None, None, None, None, fake, fake, fake, fake, fake, 35, 4, fake, 175, 35, None) == -1
    assert b"cfg is NULL" in lib.umlh_last_error()
    from umlh._lib import RolloutCfg
    P = (C.c_void_p * 12)(*([64] * 11 + [None]))
    c = RolloutCfg(40, 2048, 35, 1, 4, 1e-5)
    assert lib.umlh_rollout(C.byref(c), P, None, None, fake, fake, fake, fake, fake, 35, 4, fake, 175, 35, None) == -1
    assert b"P[11] is NULL" in lib.umlh_last_error()


def test_spectrum_rejects_bad_arguments_before_touching_the_gpu(lib):
    fake = C.c_void_p(64)
    call = lambda x=fake, ldb=50 * 300, ldt=300, b=32, T=50, d=300, out=fake, scratch=fake, nbytes=1 << 30: \
        lib.umlh_seq_spectrum(x, ldb, ldt, b, T, d, out, scratch, nbytes, None)
    for kw, what in ((dict(x=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(scratch=None), b"null pointer"),
                     (dict(T=0), b"t_len=0"), (dict(T=1025, ldb=1025 * 300), b"t_len=1025"), (dict(d=0), b"d=0"), (dict(b=0), b"b=0"),
                     (dict(b=(1 << 20) + 1), b"b=1048577"), (dict(ldt=299), b"ldt=299"), (dict(ldb=299), b"ldb=299"),
                     (dict(ldb=49 * 300), b"overlap"), (dict(nbytes=8), b"scratch of 8 bytes"),
                     (dict(b=1 << 20, d=1024, ldt=1024, ldb=50 * 1024, T=50), b"too large")):
        assert call(**kw) == -1, kw
        msg = lib.umlh_last_error()
        assert b"umlh_seq_spectrum" in msg and what in msg, (kw, msg)


def test_spectrum_scratch_query(lib):
    q = lib.umlh_seq_spectrum_scratch_bytes
    assert q(0, 50, 300) == 0 and q(32, 0, 300) == 0 and q(32, 1025, 300) == 0 and q(32, 50, 0) == 0 and q((1 << 20) + 1, 50, 1) == 0
    assert q(32, 50, 300) >= 2 * 19 * 26 * 8                           # ceil(32 / 16) * ceil(300 / 16) partial vectors of 26 doubles
    assert q(1, 1, 1) >= 8
    # the largest call of the envelope: 2^20 partial vectors of 513 doubles do not fit 32 bits
    assert q(1 << 20, 1024, 16) >= (1 << 16) * 513 * 8
    assert q(1 << 20, 1024, 256) >= (1 << 20) * 513 * 8 > 1 << 32
    assert q(1 << 20, 1024, 257) == 0                                  # one column chunk too many


def test_python_wrappers_validate_before_any_gpu_work():
    import torch
    import umlh
    with pytest.raises(ValueError):
        umlh.seq_spectrum(torch.zeros(3, 4))
    with pytest.raises(ValueError):
        umlh.seq_spectrum(torch.zeros(3, 4, 5, dtype=torch.int64))
    with pytest.raises(ValueError):
        umlh.rollout_rows(torch.zeros(3), None, None, None, None, [], 1e-5, None, None, 2)
    with pytest.raises(ValueError):
        umlh.rollout_rows(torch.zeros(3, 5), torch.zeros(10, 5), torch.zeros(10), None, None, [torch.zeros(1)] * 11, 1e-5,
                          torch.zeros(5, 10), torch.zeros(5), 2)
    with pytest.raises(ValueError):
        umlh.rollout_rows(torch.zeros(3, 5), torch.zeros(10, 5), torch.zeros(10), None, None, [], 1e-5, torch.zeros(5, 10),
                          torch.zeros(5), -1)


def test_train_rollout_spectra_needs_the_capture():
    from multibench import train as T
    with pytest.raises(ValueError, match="capture_embeddings_during_training"):
        T.train(None, "xy", [], [], None, rollout_spectra=True)
