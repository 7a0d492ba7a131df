"""CPU: the float64 references of the MultiBench critics (tests/_critic_ref.py) are themselves pinned -- against
oracle/multibench_oracle.py, the reference's golden vectors and torch autograd in float64 -- the restated plan of the decoder
backward reproduces the library's size query and reaches every path the case table claims, and the criterion is shown to be
calibrated (the levels of the module docstring re-measured) and to discriminate (every deliberately wrong variant breaks a bound by
8x or more).  No GPU."""
import re

import numpy as np
import pytest
import torch

import _critic_ref as R
from conftest import load_golden
from oracle import multibench_oracle as MO

F64 = np.float64


def _t(a):
    return torch.from_numpy(np.asarray(a, F64))


def _close(got, ref, tol=1e-12):
    ref = np.asarray(ref, F64)
    assert np.abs(np.asarray(got, F64) - ref).max(initial=0.0) <= tol * max(1.0, np.abs(ref).max(initial=0.0))


# ---- the decoder reference ----
@pytest.mark.parametrize("c", [c for c in R.DECODER_CASES if c["T"] > 1], ids=lambda c: c["id"])
def test_seq_mse_ref_equals_the_oracle(c):
    """oracle.multibench_oracle.decoder_next_step_loss states T > 1 with lengths None or in 1 .. T."""
    z, w, b, x = R.build_decoder(c)
    for pat in ("none", "random"):
        ln = R.build_lengths(c, pat)
        r = R.seq_mse_ref(z, w, b, x, ln, 1.0)
        loss, recon, dz, dw, db = MO.decoder_next_step_loss(z.astype(F64), w.astype(F64), b.astype(F64), x.astype(F64), ln)
        if ln is None:                                        # (the oracle masks with ones: its unmasked mean has the epsilon too)
            loss, dz, dw, db = (g * (1 + 1e-8 / float(r["denominator"])) for g in (loss, dz, dw, db))
        _close(r["loss"], loss)
        _close(r["recon"], recon)
        for got, ref in ((r["dz"], dz), (r["dw"], dw), (r["db"], db)):
            _close(got, ref, 1e-11)


@pytest.mark.parametrize("tag", ["z20_sin", "z40_learn", "z20_nopos"])
def test_seq_mse_ref_equals_the_reference_golden(tag):
    g = load_golden("mb_" + tag)
    for mod, dec in (("x", 0), ("y", 1)):
        w, b = g[f"sd::decoders.{dec}.fc.weight"], g[f"sd::decoders.{dec}.fc.bias"]
        r = R.seq_mse_ref(g["z" + mod], w, b, g[mod], g["l" + mod], 1.0)
        assert abs(float(r["loss"]) - float(g["loss_" + mod])) < 1e-5
        np.testing.assert_allclose(r["recon"], g[mod + "_recon"], atol=2e-5)


@pytest.mark.parametrize("c", R.DECODER_CASES, ids=lambda c: c["id"])
def test_seq_mse_ref_equals_torch_autograd(c):
    """MultiBench/models.py:129-143, 209-213 written with torch in float64, every lengths pattern (0, 1, T, > T, negative)."""
    B, T = c["B"], c["T"]
    zn, wn, bn, xn = R.build_decoder(c)
    for pat in R.decoder_runs(c):
        ln = R.build_lengths(c, pat)
        z, w, b = (_t(a).requires_grad_(True) for a in (zn, wn, bn))
        x = _t(xn)
        recon = z @ w.T + b
        if T == 1:
            loss = (recon[:, 0] - x[:, 0]).pow(2).mean()
        elif ln is None:
            loss = (recon[:, :-1] - x[:, 1:]).pow(2).mean()
        else:
            mask = (torch.arange(T)[None, :] < torch.as_tensor(ln)[:, None])[:, 1:]
            me = mask[..., None].expand_as(x[:, 1:]).double()
            loss = ((recon[:, :-1] - x[:, 1:]) ** 2 * me).sum() / (me.sum() + 1e-8)
        (R.GRAD_OUT * loss).backward()
        r = R.seq_mse_ref(zn, wn, bn, xn, ln, R.GRAD_OUT)
        _close(r["loss"], loss.item())
        for got, t in ((r["dz"], z), (r["dw"], w), (r["db"], b)):
            _close(got, t.grad.numpy(), 1e-11)
        if pat == "dead":
            assert float(r["loss"]) == 0 and not r["dz"].any() and not r["dw"].any() and not r["db"].any()
            assert float(r["denominator"]) == 1e-8
        back = R.seq_mse_backward_ref(zn, wn, r["dres"], r["denominator"], R.GRAD_OUT)
        for k in ("dz", "dw", "db"):
            _close(back[k][0].reshape(r[k].shape), r[k])


def test_live_mask_rule():
    T = 6
    live = R.live_mask(7, T, [0, 1, 2, T, T + 3, -2, T - 1])
    assert live.sum(1).tolist() == [0, 0, 1, T - 1, T - 1, 0, T - 2]
    assert not live[:, -1].any()
    assert R.live_mask(3, 1, [0, 5, -1]).all() and R.live_mask(3, 1, None).all()
    assert R.live_mask(2, T, None).sum() == 2 * (T - 1)


# ---- the plan ----
@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_plan_reproduces_the_size_query_and_the_table_reaches_its_paths(lib):
    seen_sp, short, big_chunk = set(), False, False
    for c in R.DECODER_CASES:
        B, T, Z, D = c["B"], c["T"], c["Z"], c["D"]
        sp, ns, chunk, nr = R.plan(B, T, Z, D)
        assert (sp, ns, chunk, nr) == c["plan"], c["id"]
        assert int(lib.umlh_seq_mse_backward_scratch_floats(B, T, Z, D)) == sp * D * Z + nr * D + 64 == R.scratch_floats(B, T, Z, D)
        assert 1 <= ns <= sp and (nr - 1) * chunk < B * T <= nr * chunk
        seen_sp.add(sp)
        short |= ns < sp
        big_chunk |= chunk > 64
    assert {1, 2, 3, 25, 32} <= seen_sp and short and big_chunk
    e = next(c for c in R.DECODER_CASES if c["id"] == "e_sp2")
    assert e["B"] * e["T"] - 2 * 64 == 2                      # the last db chunk of case e has 2 rows
    # every shape of a few hundred random ones, the 128-row threshold included
    rng = np.random.default_rng(0)
    for _ in range(300):
        B, T, Z, D = (int(v) for v in (rng.integers(1, 70), rng.integers(1, 70), rng.integers(1, 310), rng.integers(1, 310)))
        assert int(lib.umlh_seq_mse_backward_scratch_floats(B, T, Z, D)) == R.scratch_floats(B, T, Z, D), (B, T, Z, D)
    for R_ in (127, 128, 129):
        assert int(lib.umlh_seq_mse_backward_scratch_floats(1, R_, 40, 35)) == R.scratch_floats(1, R_, 40, 35)
    assert R.plan(1, 127, 40, 35)[0] == 1 and R.plan(1, 128, 40, 35)[0] == 2


# ---- the InfoNCE reference ----
def test_infonce_ref_equals_the_oracle_and_the_reference_golden():
    g = load_golden("infonce")
    for tag in ("small", "masked", "wide", "one_row_seqs"):
        pred, tgt, temp = g[f"{tag}::pred"], g[f"{tag}::tgt"], float(g[f"{tag}::temperature"])
        sel = g[f"{tag}::mask"].astype(bool) if int(g[f"{tag}::masked"]) else np.ones(pred.shape[:2], bool)
        r = R.infonce_ref(pred[sel], tgt[sel], temp, 1.0)
        loss, dp = MO.infonce_loss(pred, tgt, sel, float(np.float32(temp)))
        _close(r["loss"], loss)
        _close(r["dpred"], dp[sel], 1e-11)
        assert abs(float(r["loss"]) - float(g[f"{tag}::loss"])) < 2e-5, tag
        np.testing.assert_allclose(r["dpred"], g[f"{tag}::dpred"][sel], atol=2e-6, rtol=2e-4, err_msg=tag)


@pytest.mark.parametrize("c", R.INFONCE_CASES, ids=R.infonce_id)
def test_infonce_ref_equals_torch_autograd(c):
    """SequenceInfoNCELoss with torch in float64.  torch's gradient is dpred_torch: on a row of norm below 1e-12 clamp_min's
    backward drops the projection term that the kernels' documented form (dpred) keeps."""
    n, D, temp, kind = c
    pn, tn = R.build_infonce(c)
    r = R.infonce_ref(pn, tn, temp, R.GRAD_OUT)
    p = _t(pn).requires_grad_(True)
    ph, th = torch.nn.functional.normalize(p, dim=-1), torch.nn.functional.normalize(_t(tn), dim=-1)
    logits = ph @ th.T / float(np.float32(temp))
    loss = torch.nn.functional.cross_entropy(logits, torch.arange(n))
    (R.GRAD_OUT * loss).backward()
    _close(r["loss"], loss.item(), 1e-11)
    _close(r["probs"], (torch.softmax(logits, -1) - torch.eye(n)).detach().numpy(), 1e-11)
    _close(r["dpred_torch"], p.grad.numpy(), 1e-10)
    leaves = R.infonce_backward_ref(r["pred_hat"], r["target_hat"], r["pred_norm"], r["probs"], R.GRAD_OUT, temp)
    _close(leaves["dpred"], r["dpred"])
    row = R.special_row(c)
    if kind == "tiny_row":
        # the declared difference: |y|^2 = (|x| / 1e-12)^2 of the row's gradient, and only on that row
        diff = np.abs(r["dpred"] - r["dpred_torch"])
        y2 = float((r["pred_hat"][row] ** 2).sum())
        assert abs(y2 - (R.TINY_NORM / R.NORM_EPS) ** 2) < 1e-3 * y2
        assert not np.delete(diff, row, 0).any()
        if D > 1:
            assert 0 < diff[row].max() <= 1.001 * y2 * np.abs(r["dpred_torch"][row]).max()
    else:
        assert np.array_equal(r["dpred"], r["dpred_torch"])   # a zero row has y = 0: both forms agree
    if kind == "zero_row":
        assert not r["pred_hat"][row].any() and float(r["pred_norm"][row]) == 1e-12
        _close(r["row_loss"][row], np.log(n))
    if n == 1:
        assert float(r["loss"]) == 0 and not r["probs"].any() and not r["dpred"].any()


def test_the_infonce_table_covers_every_listed_value():
    ns, Ds, temps, kinds = (set(c[i] for c in R.INFONCE_CASES) for i in range(4))
    assert ns == {1, 2, 3, 4, 5, 63, 64, 65, 257} and Ds == {1, 8, 63, 64, 65, 300}
    assert temps == {0.07, 1.0, 0.01} and kinds == {"random", "sharp", "zero_row", "tiny_row", "duplicate_targets"}
    assert all((c[2] == 0.01) == (c[3] == "sharp") for c in R.INFONCE_CASES) and len(R.INFONCE_CASES) <= 24
    for c in R.INFONCE_CASES:
        if c[3] == "sharp" and c[1] > 1:                      # the diagonal dominates: row_loss = lse - diag cancels
            r = R.infonce_ref(*R.build_infonce(c), c[2], 1.0)
            assert np.median(r["row_loss"]) < 0.05 and np.abs(np.diagonal(r["pred_hat"] @ r["target_hat"].T)).min() > 0.99


# ---- the criterion ----
def test_levels_of_the_docstring_are_remeasured_and_under_their_bounds():
    lv = R.measure_levels()
    assert {f: set(d) for f, d in lv.items()} == {f: set(d) for f, d in R.LEVELS_LOG2.items()}
    rows = {(m[1], m[2]): (float(m[3]), int(m[4])) for m in re.finditer(r"(\w+) +(\w+) +(-\d+\.\d) +(-\d+)(?= |\n)", R.__doc__)}
    for fam, d in lv.items():
        for k, v in d.items():
            rec = R.LEVELS_LOG2[fam][k]
            assert np.log2(v) <= rec + 0.3, (fam, k, np.log2(v), rec)
            assert 8 * v <= R.BOUNDS[fam][k] * 2 ** 0.3 and R.BOUNDS[fam][k] <= 16 * 2.0 ** rec
            assert rows[fam, k] == (rec, int(np.log2(R.BOUNDS[fam][k]))), (fam, k, rows.get((fam, k)))


@pytest.mark.parametrize("name", R.WRONG_VARIANTS)
def test_every_wrong_variant_breaks_a_bound_by_8x(name):
    assert R.variant_excess(name) >= 8.0, name


def test_sequential_fp32_sums_meet_the_gemm_criterion_on_every_decoder_case():
    """The single-sum outputs in the worst fp32 order (one rounding per product, then the rounded scale s = 2 g / denominator):
    the criterion the GPU test applies to recon and to the backward given its leaves holds for an honest kernel at every shape of
    the table, the one- and two-term sums of the smallest case included."""
    from _gemm_ref import emulate
    F32 = np.float32
    for c in R.DECODER_CASES:
        z, w, b, x = R.build_decoder(c)
        B, T, Z, D = c["B"], c["T"], c["Z"], c["D"]
        if B * T * Z * D > 200000:
            continue                                          # (the emulation walks k in Python)
        ref = R.seq_mse_ref(z, w, b, x, None, 1.0)
        recon = (emulate("fp32", z.reshape(B * T, Z), w).astype(F64) + b).astype(F32)
        assert R.meets_criterion(R.gemm_err(recon, ref["recon"].reshape(B * T, D), ref["S_recon"].reshape(B * T, D))), c["id"]
        dres, den = R.build_isolated(c)
        for g in R.ISOLATED_GRADS:
            s = F32(F32(2) * F32(g) / den)
            back = R.seq_mse_backward_ref(z, w, dres, den, g)
            got = dict(dz=(emulate("fp32", dres.reshape(B * T, D), w.T.copy()) * s).astype(F32).reshape(B, T, Z),
                       dw=(emulate("fp32", dres.reshape(B * T, D).T.copy(), z.reshape(B * T, Z).T.copy()) * s).astype(F32))
            for k, v in got.items():
                assert R.meets_criterion(R.gemm_err(v, back[k][0].reshape(v.shape), back[k][1].reshape(v.shape))), (c["id"], g, k)


def _mfma_chain(A, B, rows=None):
    """A [M,K] . B [N,K]^T as the fp32 MFMA accumulates it (k in pairs, one rounding per pair), optionally in chunks of `rows`
    reduction rows whose sums are added in order."""
    from _gemm_ref import _chain
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    K = A.shape[1]
    acc = np.zeros((A.shape[0], B.shape[0]), np.float32)
    for k0 in range(0, K, rows or K):
        part = _chain([A[:, k0:k0 + (rows or K)]], [B[:, k0:k0 + (rows or K)]], ((0, 0),), 2)
        acc = (part.astype(F64) + acc).astype(np.float32)
    return acc


@pytest.mark.parametrize("cid", ["h_cap32", "i_chunk65"])
def test_one_chain_over_thousands_of_forward_rows_misses_the_criterion_and_the_chunked_sum_meets_it(cid):
    """Why umlh_seq_mse_backward without scratch sums dW in the plan's row chunks.  On leaves a forward produced, dres = recon - x
    correlates with z: the terms of dW share a sign, the partial sums drift, and one k-ordered chain over 2112 / 4160 rows rounds
    every add at the running sum's magnitude.  (On arbitrary leaves the same chain meets the criterion: the test above.)"""
    from _gemm_ref import slab_count
    c = next(c for c in R.DECODER_CASES if c["id"] == cid)
    B, T, Z, D = c["B"], c["T"], c["Z"], c["D"]
    z, w, b, x = R.build_decoder(c)
    r = R.seq_mse_ref(z, w, b, x, None, R.GRAD_OUT, np.float32)
    dres, den = r["dres"].astype(np.float32), np.float32(r["denominator"])
    back = R.seq_mse_backward_ref(z, w, dres, den, R.GRAD_OUT)
    s = np.float32(np.float32(2 * R.GRAD_OUT) / den)
    A, Bm = dres.reshape(B * T, D).T.copy(), z.reshape(B * T, Z).T.copy()
    one = R.gemm_err((_mfma_chain(A, Bm) * s).astype(np.float32), back["dw"][0], back["dw"][1])
    chunk = slab_count(B * T, c["plan"][0])[1]
    chunked = R.gemm_err((_mfma_chain(A, Bm, chunk) * s).astype(np.float32), back["dw"][0], back["dw"][1])
    assert not R.meets_criterion(one) and one[1] > 2 * chunked[1], (cid, np.log2(one), np.log2(chunked))
    assert R.meets_criterion(chunked) and chunked[1] < R.CRIT_RMS / 2, (cid, np.log2(chunked))


def test_dhat_criterion_holds_on_arbitrary_leaves_and_not_on_a_forwards_leaves():
    """The GEMM criterion on dhat = probs . target_hat is stated on arbitrary leaves.  On a forward's own leaves a row of
    softmax - I is one term near -1 followed by hundreds of small positive ones (at D = 1 of two values only): every add of the
    k-ordered chain rounds at magnitude 1 and, the addends repeating, in the same direction."""
    big = (257, 1, 1.0, "random")
    assert big in R.INFONCE_CASES
    for c in R.INFONCE_CASES:
        ph, th, pn, pr = R.build_leaves(c)
        ref = R.infonce_backward_ref(ph, th, pn, pr, R.GRAD_OUT, c[2])
        assert R.meets_criterion(R.gemm_err(_mfma_chain(pr, th.T.copy()), ref["dhat"], ref["S_dhat"])), c
    r = R.infonce_ref(*R.build_infonce(big), big[2], R.GRAD_OUT)
    ph, th, pn, pr = (r[k].astype(np.float32) for k in ("pred_hat", "target_hat", "pred_norm", "probs"))
    ref = R.infonce_backward_ref(ph, th, pn, pr, R.GRAD_OUT, big[2])
    e = R.gemm_err(_mfma_chain(pr, th.T.copy()), ref["dhat"], ref["S_dhat"])
    assert not R.meets_criterion(e) and e[1] > 4 * R.CRIT_RMS, np.log2(e)
