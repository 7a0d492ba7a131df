"""GPU: umlh.align.svcca and umlh.spectral.principal_subspace (fp64 centred Grams, Householder tridiagonalisation with the
reflectors kept, bisection, inverse iteration) against float64 numpy.

Value: per golden case |svcca - closed64| and every |rho_k - rho64_k| are no larger than the reference's own largest error on
the fp32 inputs over five seeds (stored in the golden).  Eigenpairs: residual and orthogonality ratios within 8 x those of
numpy.linalg.eigh on the same float64 Gram (floored at 1), the projector within the first-order perturbation bound.  Every
measured figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import _svcca_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("mosei", "mid", "offset", "wide", "q1", "full", "same")
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def gold():
    return load_golden("svcca")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _svcca(a, b, q):
    import umlh
    return float(umlh.svcca(_dev(a), _dev(b), q))


@pytest.mark.parametrize("case", CASES)
def test_value_against_the_closed_form(gold, case):
    import umlh
    a, b, q = gold[f"{case}/a"], gold[f"{case}/b"], int(gold[f"{case}/q"])
    closed, rho64 = float(gold[f"{case}/closed64"]), gold[f"{case}/rho64"]
    bound = float(np.abs(gold[f"{case}/ref32"] - closed).max())
    val, rho, evals = umlh.svcca_terms(_dev(a), _dev(b), q)
    assert val.shape == () and val.dtype == torch.float64 and rho.shape == (q,) and evals.shape == (2, q)
    assert val.device.type == "cuda" and rho.dtype == torch.float64 and evals.dtype == torch.float64
    assert torch.equal(val, umlh.svcca(_dev(a), _dev(b), q))
    rho, evals = rho.cpu().numpy(), evals.cpu().numpy()
    err, rerr = abs(float(val) - closed), float(np.abs(rho - rho64).max())
    print(f"{case}: svcca {float(val):.15f} closed64 {closed:.15f} error {err:.3e}, max rho error {rerr:.3e} "
          f"(reference fp32, five seeds: {bound:.3e})")
    assert err <= bound and rerr <= bound
    assert (np.diff(rho) <= 0).all() and rho.min() >= 0.0 and rho.max() <= 1.0
    assert abs(float(val) - rho.mean()) <= 4 * EPS
    for k, x in enumerate((a, b)):
        lam64 = R.top_eigh(R.gram64(x, True), q)[0]
        np.testing.assert_allclose(evals[k], lam64, rtol=0, atol=64 * x.shape[1] * EPS * lam64[0])


def test_value_with_two_by_three_cross_tiles(gold):
    """Every recorded case has d_a <= 64: one row of 64-column tiles in the rectangular cross-Gram.  A planted case of the
    recorded kind (R.gen_case) with d_a = 65, d_b = 130 has 2 x 3 of them.  Its gap sigma_(q+1) / sigma_q stays below the 0.2
    that R.planted is built to keep clear of, like the recorded cases'; the bound is the smallest of theirs."""
    import umlh
    q = 4
    a, b = R.gen_case("tiles", 150, 65, 130, q, 2)
    gaps = [np.linalg.svd(R.standardise64(x), compute_uv=False) for x in (a, b)]
    ratio = max(s[q] / s[q - 1] for s in gaps)
    bound = min(float(np.abs(gold[f"{c}/ref32"] - float(gold[f"{c}/closed64"])).max()) for c in CASES)
    rho64 = R.rho64(a, b, q)
    val, rho, evals = umlh.svcca_terms(_dev(a), _dev(b), q)
    rho, evals = rho.cpu().numpy(), evals.cpu().numpy()
    err, rerr = abs(float(val) - float(rho64.mean())), float(np.abs(rho - rho64).max())
    print(f"tiles: sigma_(q+1)/sigma_q {ratio:.3f} svcca {float(val):.15f} closed64 {rho64.mean():.15f} error {err:.3e}, "
          f"max rho error {rerr:.3e} (bound {bound:.3e})")
    assert ratio < 0.2
    assert err <= bound and rerr <= bound
    assert (np.diff(rho) <= 0).all() and rho.min() >= 0.0 and rho.max() <= 1.0
    assert abs(float(val) - rho.mean()) <= 4 * EPS
    for k, x in enumerate((a, b)):
        lam64 = R.top_eigh(R.gram64(x, True), q)[0]
        np.testing.assert_allclose(evals[k], lam64, rtol=0, atol=64 * x.shape[1] * EPS * lam64[0])


def _eig_input(gold, name):
    if name == "gen512":
        return R.matrix_512(), 10
    case, view = name.split("-")
    return gold[f"{case}/{view}"], int(gold[f"{case}/q"])


@pytest.mark.parametrize("standardize", [0, 1])
@pytest.mark.parametrize("name", ["mosei-b", "offset-a", "wide-a", "gen512"])
def test_eigenpairs(gold, name, standardize):
    import umlh
    a, q = _eig_input(gold, name)
    n, d = a.shape
    x = _dev(a)
    evals, evecs = umlh.principal_subspace(x, q, standardize=bool(standardize))
    assert evals.shape == (q,) and evecs.shape == (d, q) and evals.dtype == torch.float64 and evecs.dtype == torch.float64
    assert evecs.is_contiguous() and evals.device.type == "cuda"
    lam, v = evals.cpu().numpy(), evecs.cpu().numpy()
    G = R.gram64(a, bool(standardize))
    lam64, v64, all64 = R.top_eigh(G, q)
    res, orth = R.eig_ratios(G, lam, v)
    res_np, orth_np = R.eig_ratios(G, lam64, v64)
    gap = (all64[q - 1] - all64[q]) / all64[0]
    proj = float(np.linalg.norm(v @ v.T - v64 @ v64.T, 2))
    proj_bound = 1e3 * d * EPS / gap
    print(f"{name} standardize={standardize} d={d} q={q}: residual ratio {res:.3f} (eigh {res_np:.3f}), orthogonality ratio "
          f"{orth:.3f} (eigh {orth_np:.3f}), projector distance {proj:.3e} (bound {proj_bound:.3e}, relative gap {gap:.3e})")
    assert res <= 8 * max(res_np, 1.0)
    assert orth <= 8 * max(orth_np, 1.0)
    assert proj <= proj_bound
    assert (np.diff(lam) <= 0).all()
    # sign convention: the largest-magnitude component of each vector is positive (the first one on ties)
    for k in range(q):
        assert v[np.argmax(np.abs(v[:, k])), k] > 0, k
    if not standardize:
        sv = umlh.svdvals(x)[:q].cpu().numpy()
        ulps = np.abs(np.sqrt(lam) - sv) / np.spacing(sv)
        print(f"  sqrt(evals) against svdvals: {ulps.max():.1f} ulps")
        assert ulps.max() <= 8


def test_invariances():
    a, b = R.quantised_pair()
    q = 6
    base = _svcca(a, b, q)
    assert 0.05 < base < 0.95
    perm, a2, b2 = R.invariance_maps(a, b)
    d_perm = abs(_svcca(a[perm], b[perm], q) - base)
    assert (a2.astype(np.float32) == a2).all() and (b2.astype(np.float32) == b2).all()
    d_aff_a = abs(_svcca(a2.astype(np.float32), b, q) - base)
    d_aff_b = abs(_svcca(a, b2.astype(np.float32), q) - base)
    d_sym = abs(_svcca(b, a, q) - base)
    print(f"svcca {base:.15f}: row permutation {d_perm:.3e}, affine map of a {d_aff_a:.3e}, of b {d_aff_b:.3e}, "
          f"swapped views {d_sym:.3e}")
    assert d_perm <= 1e-12 and d_aff_a <= 1e-9 and d_aff_b <= 1e-9 and d_sym <= 1e-13


def test_plumbing_is_bit_equal(gold):
    import umlh
    a, b, q = gold["mid/a"], gold["mid/b"], 10
    xa, xb = _dev(a), _dev(b)
    ref = umlh.svcca_terms(xa, xb, q)
    ref_ev = umlh.principal_subspace(xb, q, standardize=True)
    torch.cuda.synchronize()

    def same(got, want=ref):
        return all(torch.equal(x, y) for x, y in zip(got, want))
    # a strided view: ld > d
    wide_a = torch.full((a.shape[0], a.shape[1] + 7), 9.0, device=DEV)
    wide_a[:, :a.shape[1]] = xa
    wide_b = torch.full((b.shape[0], b.shape[1] + 16), -3.0, device=DEV)
    wide_b[:, 16:] = xb
    va, vb = wide_a[:, :a.shape[1]], wide_b[:, 16:]
    assert va.stride(0) > va.shape[1] and not vb.is_contiguous()
    assert same(umlh.svcca_terms(va, vb, q))
    assert same(umlh.principal_subspace(vb, q, standardize=True), ref_ev)
    # CPU and float64 inputs
    assert same(umlh.svcca_terms(torch.from_numpy(a), torch.from_numpy(b), q))
    assert same(umlh.svcca_terms(xa.double(), torch.from_numpy(b).double(), q))
    assert same(umlh.principal_subspace(torch.from_numpy(b).double(), q, standardize=True), ref_ev)
    # a side stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = umlh.svcca_terms(xa, xb, q)
        side_ev = umlh.principal_subspace(xb, q, standardize=True)
    s.synchronize()
    assert same(side) and same(side_ev, ref_ev)
    # two back-to-back calls
    first, second = umlh.svcca_terms(xa, xb, q), umlh.svcca_terms(xa, xb, q)
    assert same(first) and same(second)


def test_edges(gold):
    import umlh
    g = np.random.default_rng(11)
    a, b = gold["mid/a"], gold["mid/b"]
    # exact rank 3: three columns and copies of them (identical columns stay identical after standardising)
    base = g.standard_normal((200, 3)).astype(np.float32)
    rank3 = base[:, [0, 1, 2, 0, 1, 2, 2, 1, 0, 0, 1, 2]]
    val, rho, evals = umlh.svcca_terms(_dev(rank3), _dev(a[:200]), 5)
    print(f"rank 3, q = 5: svcca {float(val)}, eigenvalues {evals[0].cpu().numpy()}")
    assert torch.isnan(val) and torch.isnan(rho).all()
    assert torch.isnan(umlh.svcca(_dev(a[:200]), _dev(rank3), 5))
    assert float(umlh.svcca(_dev(rank3), _dev(a[:200]), 3)) > 0.0
    # an all-constant view
    assert torch.isnan(umlh.svcca(torch.full((50, 4), 2.0, device=DEV), _dev(a[:50]), 2))
    # a NaN entry
    bad = a.copy()
    bad[17, 5] = np.nan
    assert torch.isnan(umlh.svcca(_dev(bad), _dev(b), 10)) and torch.isnan(umlh.svcca(_dev(b), _dev(bad), 10))
    ev, vec = umlh.principal_subspace(_dev(bad), 4, standardize=True)
    assert torch.isnan(ev).all() and torch.isnan(vec).all()
    bad[17, 5] = np.inf
    assert torch.isnan(umlh.svcca(_dev(bad), _dev(b), 10))
    # a constant column next to informative ones changes nothing
    plain = _svcca(a, b, 10)
    with_const = np.concatenate([a[:, :9], np.full((a.shape[0], 1), 7.5, np.float32), a[:, 9:]], axis=1)
    d_const = abs(_svcca(with_const, b, 10) - plain)
    print(f"constant column: difference {d_const:.3e}")
    assert d_const <= 1e-12
    ev, vec = umlh.principal_subspace(_dev(with_const), 10, standardize=True)
    assert float(vec[9].abs().max()) <= 1e-15
    # the limits raise before the GPU is used
    with pytest.raises(ValueError, match="q=33"):
        umlh.svcca(_dev(a), _dev(b), 33)                       # above d_a = 32
    with pytest.raises(ValueError, match="q=65"):
        umlh.svcca(torch.zeros(100, 80, device=DEV), torch.zeros(100, 80, device=DEV), 65)
    with pytest.raises(ValueError, match="q=4"):
        umlh.svcca(_dev(a[:3]), _dev(b[:3]), 4)                # above n
    with pytest.raises(ValueError, match="d=513"):
        umlh.svcca(torch.zeros(b.shape[0], 513, device=DEV), _dev(b), 10)
    with pytest.raises(ValueError, match="n=1 "):
        umlh.svcca(_dev(a[:1]), _dev(b[:1]), 1)
    with pytest.raises(ValueError, match="d=513"):
        umlh.principal_subspace(torch.zeros(600, 513, device=DEV), 4)
