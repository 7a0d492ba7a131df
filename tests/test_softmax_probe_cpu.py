"""CPU: the reference module of the multinomial logistic probe (tests/_softmax_probe_ref.py) and its fixtures
(tests/golden/softmax_probe*.npz, written by scripts/make_golden_softmax_probe.py) are sound before the GPU tests lean on them;
the argument errors of the Python layer that need no device.

Every measured figure is printed before it is asserted (run with -s)."""
import numpy as np
import pytest

import _softmax_probe_ref as R
from conftest import load_golden

CASES = list(R.CASES)


@pytest.fixture(scope="module")
def golden():
    return load_golden("softmax_probe")


@pytest.fixture(scope="module")
def problems(golden):
    """case -> (x, y, stats, x~, optimum, sklearn's [coef | intercept]); built once."""
    out = {}
    for name, c in R.CASES.items():
        x, y = R.make_case(name)
        assert bytes(golden[f"{name}.x_sum"]).decode() == R.checksum(x), f"{name}: the regenerated features differ from the fixture's"
        assert bytes(golden[f"{name}.y_sum"]).decode() == R.checksum(y)
        stats = R.column_stats(x) if c["standardize"] else None
        sk = np.concatenate([golden[f"{name}.sk_coef"], golden[f"{name}.sk_intercept"][:, None]], axis=1)
        out[name] = (x, y, stats, R.x_tilde(x, stats), golden[f"{name}.opt"], sk)
    return out


@pytest.fixture(scope="module")
def fits(problems):
    """case -> the fp32 restatement's fit at gtol = 1e-6 n; run once."""
    return {name: R.fit_fp32(x, y, C=R.C_REG, stats=stats, gtol=1e-6 * len(y)) for name, (x, y, stats, _, _, _) in problems.items()}


@pytest.mark.parametrize("name", CASES)
def test_float64_statement_reproduces_the_stored_optimum(problems, name):
    x, y, stats, xt, opt, sk = problems[name]
    f, g = R.objective_grad(opt, xt, y, R.C_REG)
    f_sk, _ = R.objective_grad(sk, xt, y, R.C_REG)
    print(f"{name}: f*={f:.12g} max|g*|={np.abs(g).max():.2e} f_sklearn - f* = {f_sk - f:.3e}")
    assert np.abs(g).max() <= 1e-6
    assert f_sk >= f
    # finite differences see the same gradient (central, in double: h^2 truncation error)
    rng = np.random.default_rng(1)
    W = opt + 0.1 * rng.standard_normal(opt.shape)
    _, gw = R.objective_grad(W, xt, y, R.C_REG)
    for _ in range(3):
        c, j = rng.integers(opt.shape[0]), rng.integers(opt.shape[1])
        E = np.zeros_like(W)
        E[c, j] = 1e-5
        fd = (R.objective_grad(W + E, xt, y, R.C_REG, False)[0] - R.objective_grad(W - E, xt, y, R.C_REG, False)[0]) / 2e-5
        assert abs(fd - gw[c, j]) <= 1e-6 * max(1.0, abs(gw[c, j]))


@pytest.mark.parametrize("name", CASES)
def test_fp32_restatement_converges(problems, fits, golden, name):
    x, y, stats, xt, opt, sk = problems[name]
    fit = fits[name]
    f, g = R.objective_grad(fit["W"], xt, y, R.C_REG)
    f_opt = R.objective_grad(opt, xt, y, R.C_REG, False)[0]
    f_sk = R.objective_grad(sk, xt, y, R.C_REG, False)[0]
    obj = fit["objectives"][: fit["n_iter"] + 1]
    print(f"{name}: converged={fit['converged']} n_iter={fit['n_iter']} gap={(f - f_opt) / f_opt:.2e} sklearn's gap={(f_sk - f_opt) / f_opt:.2e} "
          f"max|g|={np.abs(g).max():.2e}")
    assert fit["converged"] == 1
    assert f <= f_sk
    assert np.abs(g).max() <= 1e-6 * len(y) + R.grad_allowance(fit["W"], xt, y)
    assert (np.diff(obj) <= 0).all() and np.isnan(fit["objectives"][fit["n_iter"] + 1:]).all()


@pytest.mark.parametrize("name", CASES)
def test_tau_and_the_share_of_undecidable_rows(problems, fits, golden, name):
    """TAU = 8 x the largest logit error of the fp32 restatement, rounded up to a power of two.  The re-measured value may
    differ from the stored one by what another BLAS's summation order does to the fp32 products: one binade is allowed."""
    x, y, stats, xt, opt, sk = problems[name]
    tau = float(golden[f"{name}.tau"])
    zerr = np.abs(xt.astype(np.float64) @ (fits[name]["W"].astype(np.float64) - opt).T).max()
    _, marg = R.margins(opt, xt)
    share = float(np.mean(marg <= tau))
    print(f"{name}: stored tau={tau:.3g} re-measured 8 x zerr={8 * zerr:.3g} undecidable share={share:.4f}")
    assert R.pow2_ceil(8 * zerr) <= 2 * tau
    assert share <= 0.05


def test_wrong_variants_break_a_bound_by_8x(problems):
    """Each wrong variant of the reference misses the optimum's gradient bound (1e-6) by at least 8x."""
    x, y, stats, xt, opt, sk = problems["n600_d33_k7_ld40"]
    for kw in (dict(penalise_intercept=True), dict(mean=True), dict(label_shift=1)):
        _, g = R.objective_grad(opt, xt, y, R.C_REG, **kw)
        print(f"{kw}: max|g| at the optimum = {np.abs(g).max():.3e}")
        assert np.abs(g).max() >= 8e-6
    x, y, stats, xt, opt, sk = problems["n900_d20_k5_std"]
    _, g = R.objective_grad(opt, R.x_tilde(x, None), y, R.C_REG)
    print(f"standardisation dropped: max|g| at the optimum = {np.abs(g).max():.3e}")
    assert np.abs(g).max() >= 8e-6
    # softmax without the max shift at logits of +-90, in the device's fp32: exp(90) is not an fp32 number
    z = np.array([[90.0, -90.0, 0.0]], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        naive = np.log(np.exp(z).sum(dtype=np.float32))
    shifted = 90.0 + np.log(np.exp(z.astype(np.float64) - 90.0).sum())
    print(f"no max shift: logsumexp = {naive} against {shifted}")
    assert not np.isfinite(naive) and abs(shifted - 90.0) < 1e-30 + 1e-12
    W = np.zeros((3, 2))
    W[:, 1] = [90.0, -90.0, 0.0]
    f, g = R.objective_grad(W, np.ones((4, 2)), np.array([0, 1, 2, 0]), 1.0)
    assert np.isfinite(f) and np.isfinite(g).all() and abs(f - (0 + 180 + 90 + 0)) < 1e-9
    with np.errstate(over="ignore", invalid="ignore"):
        f_naive, _ = R.objective_grad(W * 8, np.ones((4, 2)), np.array([0, 1, 2, 0]), 1.0, max_shift=False)
    assert not np.isfinite(f_naive)


def test_rows_with_labels_out_of_range_contribute_nothing(problems):
    x, y, stats, xt, opt, sk = problems["n257_d5_k3"]
    y2 = y.copy()
    y2[::7] = -1
    y2[3::11] = 3
    keep = (y2 >= 0) & (y2 < 3)
    f1, g1 = R.objective_grad(opt, xt, y2, R.C_REG)
    f2, g2 = R.objective_grad(opt, xt[keep], y2[keep], R.C_REG)
    assert abs(f1 - f2) <= 1e-12 * abs(f2) and np.abs(g1 - g2).max() <= 1e-12


def test_python_argument_errors():
    from umlh.probe import LogisticProbe, SoftmaxProbe, logistic_probe
    for kw in (dict(C=0.0), dict(C=-1.0), dict(max_iter=0), dict(max_iter=1001), dict(gtol=-1.0), dict(history=0), dict(history=33)):
        with pytest.raises(ValueError):
            SoftmaxProbe(**kw)
    pr = SoftmaxProbe(C=0.5, max_iter=7, gtol=None, history=3, standardize=True, keep_objectives=True)
    assert (pr.C, pr.max_iter, pr.gtol, pr.history, pr.standardize, pr.keep_objectives) == (0.5, 7, None, 3, True, True)
    assert isinstance(logistic_probe("lbfgs", 2), LogisticProbe) and logistic_probe("liblinear", 2).kind == "liblinear"
    assert isinstance(logistic_probe("lbfgs", 3), SoftmaxProbe)
    with pytest.raises(ValueError, match="liblinear"):
        logistic_probe("liblinear", 3)
    with pytest.raises(ValueError):
        logistic_probe("newton", 3)
    with pytest.raises(ValueError):
        logistic_probe("lbfgs", 1)
