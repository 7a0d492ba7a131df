"""CPU checks of the yardstick the fp32 GEMM tests use (tests/_gemm_ref.py): the float64 restatement of umlh_gemm_f32's contract,
the accuracy criterion (it accepts the fp32 fma chain and the x3 six-piece products, and rejects the x3 form without its lo
pieces and plain bf16 products), and the dispatch rules restated in Python."""
import numpy as np
import pytest

from _gemm_ref import (CASES, CRIT_MAX, CRIT_RMS, ENVS, X3_KERNELS, build_case, emulate, gemm_err, gemm_ref, meets_criterion,
                       operands, predict_kernel, spread_rows)


@pytest.mark.parametrize("K", [64, 1024, 4096])
def test_criterion_accepts_the_fp32_chain_and_x3_and_rejects_truncated_products(K):
    rng = np.random.default_rng(K)
    A, B = spread_rows(rng, 48, K), spread_rows(rng, 40, K)
    ref, S = gemm_ref(A, B, 0, 0, None, None, 1.0, 48, 40, K, K, K)
    err = {f: gemm_err(emulate(f, A, B), ref, S) for f in ("fp32", "x3", "x3_drop_lo", "bf16")}
    for f in ("fp32", "x3"):                 # measured: max <= 2^-22, rms <= 2^-25 (4x under the rms bound)
        assert meets_criterion(err[f]), (f, np.log2(err[f]))
        assert err[f][1] <= CRIT_RMS / 4, (f, np.log2(err[f]))
    for f in ("x3_drop_lo", "bf16"):         # measured: rms >= 2^-21.2 (3.5x over the bound at K = 4096)
        assert not meets_criterion(err[f]), (f, np.log2(err[f]))
        assert err[f][1] >= CRIT_RMS * 3, (f, np.log2(err[f]))
    assert err["bf16"][0] > CRIT_MAX         # (and the max bound alone catches bf16 products)


def test_reference_reads_strides_transposes_and_gathers_as_the_header_describes():
    rng = np.random.default_rng(5)
    M, N, K = 7, 5, 9
    X, W = rng.standard_normal((M, K)), rng.standard_normal((N, K))
    rows = rng.integers(0, M, 11)
    krows = rng.integers(0, 12, K)
    for ta, tb in ((0, 0), (0, 1), (1, 1)):
        lda, ldb = (K + 3 if ta == 0 else 11 + 2), (K + 1 if tb == 0 else N + 4)
        if ta == 0:                          # A[r*lda + k], rows gathered: 11 output rows read table rows `rows`
            A = np.zeros((M, lda)); A[:, :K] = X; want_a, mm, ar = X[rows], 11, rows
        else:                                # A[k*lda + m]
            Xt = rng.standard_normal((11, K)); A = np.zeros((K, lda)); A[:, :11] = Xt.T; want_a, mm, ar = Xt, 11, None
        if tb == 0:                          # B[n*ldb + k]
            B = np.zeros((N, ldb)); B[:, :K] = W; want_b, kr = W, None
        else:                                # B[krow*ldb + n], reduction rows gathered
            T = rng.standard_normal((12, N)); B = np.zeros((12, ldb)); B[:, :N] = T; want_b, kr = T[krows].T, krows
        Am, Bm = operands(A.astype(np.float32), B.astype(np.float32), ta, tb, ar, kr, mm, N, K, lda, ldb)
        np.testing.assert_array_equal(Am, want_a.astype(np.float32).astype(np.float64))
        np.testing.assert_array_equal(Bm, want_b.astype(np.float32).astype(np.float64))
        ref, S = gemm_ref(A.astype(np.float32), B.astype(np.float32), ta, tb, ar, kr, -0.5, mm, N, K, lda, ldb)
        np.testing.assert_allclose(ref, -0.5 * Am @ Bm.T, rtol=1e-14)
        np.testing.assert_allclose(S, 0.5 * np.abs(Am) @ np.abs(Bm).T, rtol=1e-14)


def test_reference_follows_ieee_for_inf_nan_and_zero_products():
    rng = np.random.default_rng(6)
    A = rng.standard_normal((9, 6)).astype(np.float32)
    B = rng.standard_normal((8, 6)).astype(np.float32)
    A[0, 1] = np.inf; A[1, 2] = -np.inf; A[2, 3] = np.nan; A[3, 4] = np.uint32(0x7F800001).view(np.float32); A[4, :] = 0
    B[0, 1] = 0.0; B[1, 5] = np.inf; B[2, 0] = -np.inf; A[5, 5] = 0.0; B[3, 1] = np.inf     # inf*0, 0*inf, +inf + inf ...
    ref, _ = gemm_ref(A, B, 0, 0, None, None, 2.0, 9, 8, 6, 6, 6)
    with np.errstate(invalid="ignore", over="ignore"):
        brute = 2.0 * (A.astype(np.float64)[:, None, :] * B.astype(np.float64)[None, :, :]).sum(-1)
    np.testing.assert_array_equal(np.isnan(ref), np.isnan(brute))
    np.testing.assert_array_equal(ref[~np.isnan(ref)] == np.inf, brute[~np.isnan(brute)] == np.inf)
    np.testing.assert_array_equal(ref[~np.isnan(ref)] == -np.inf, brute[~np.isnan(brute)] == -np.inf)
    fin = np.isfinite(brute)
    np.testing.assert_allclose(ref[fin], brute[fin], rtol=1e-12)
    assert np.isnan(ref).any() and np.isposinf(ref).any() and np.isneginf(ref).any()


def test_error_measure_counts_a_nonfinite_result_of_a_finite_reference_as_a_failure():
    ref, S = np.array([[1.0, 0.0, np.inf]]), np.array([[2.0, 0.0, 1.0]])
    assert gemm_err(np.array([[1.0, 0.0, np.nan]]), ref, S) == (0.0, 0.0)
    assert gemm_err(np.array([[1.0 + 2.0 ** -22, 0.0, 0.0]]), ref, S)[0] == 2.0 ** -23
    assert gemm_err(np.array([[1.0, 1e-30, 0.0]]), ref, S)[0] == np.inf          # S = 0: the output must be exact
    assert gemm_err(np.array([[np.nan, 0.0, 0.0]]), ref, S)[0] == np.inf


def _c(ta, tb, M, N, K, splits=1, a_rows=False, k_rows=False, **kw):
    c = dict(ta=ta, tb=tb, M=M, N=N, K=K, splits=splits, a_rows=a_rows, k_rows=k_rows,
             lda=M if ta else K, ldb=N if tb else K, ldo=N)
    c.update(kw)
    return c


def test_predicted_kernels_of_the_gpu_case_table():
    for c in CASES:
        assert predict_kernel(c) == c["expect"], c["id"]
        assert predict_kernel(c, ENVS["x3_off"]) == (c["expect"][:-3] if c["expect"] in X3_KERNELS else c["expect"]), c["id"]
    by_id = {c["id"]: c for c in CASES}
    assert predict_kernel(by_id["15_tm2_by_slabs_ldo"], {"UMLH_F32_TM": "1"}) == "tm1"
    assert predict_kernel(by_id["09_dw"], {"UMLH_F32_DW": "0"}) == "tm1"
    assert predict_kernel(by_id["09_dw"], {"UMLH_F32_TM": "2"}) == "dw_x3"        # (the tile override does not reach dw)


def test_dispatch_rules():
    # the 768-workgroup switch of the 128x128 grid: 95 vs 96 row tiles of 64 at N = 1000 (8 column tiles of 128)
    assert predict_kernel(_c(0, 0, 95 * 128, 1000, 600, a_rows=True)) == "tm1"          # 8 x 95 = 760
    assert predict_kernel(_c(0, 0, 95 * 128 + 1, 1000, 600, a_rows=True)) == "tm2_x3"   # 8 x 96 = 768
    assert predict_kernel(_c(0, 0, 12160, 1000, 512, a_rows=True)) == "tm1"             # logits: 760 workgroups
    assert predict_kernel(_c(0, 0, 12290, 1000, 512, a_rows=True)) == "tm2_x3"          # 776
    assert predict_kernel(_c(0, 0, 12290, 1000, 512, a_rows=True), {"UMLH_F32_X3": "0"}) == "tm2"
    assert predict_kernel(_c(0, 0, 12290, 1000, 512, a_rows=True), {"UMLH_F32_TM": "1"}) == "tm1"
    assert predict_kernel(_c(0, 0, 100, 100, 600, a_rows=True), {"UMLH_F32_TM": "2"}) == "tm2_x3"
    # slabs count toward the switch: 8 x 8 tiles x 12 slabs = 768; 11 slabs stay on the 64x64 tile
    assert predict_kernel(_c(0, 0, 1000, 1000, 20000, splits=12)) == "tm2_x3"
    assert predict_kernel(_c(0, 0, 1000, 1000, 20000, splits=11)) == "tm1"
    # dense: no gathers, (ta,tb) != (1,0) and at most 512 reduction rows per split
    assert predict_kernel(_c(0, 0, 100, 100, 512)) == "gemm_enc"
    assert predict_kernel(_c(0, 0, 100, 100, 513)) == "tm1"
    assert predict_kernel(_c(0, 0, 100, 100, 1024, splits=2)) == "gemm_enc"
    assert predict_kernel(_c(0, 0, 100, 100, 200, a_rows=True)) == "tm1"
    assert predict_kernel(_c(1, 1, 4000, 4000, 300)) == "gemm_enc"
    # dw_f32: (0,1), no a_rows, M*N >= 8 128x128 tiles, N % 4 == 0, 16-byte strides and bases, <= 4096 rows per split
    assert predict_kernel(_c(0, 1, 512, 256, 1000, k_rows=True)) == "dw_x3"
    assert predict_kernel(_c(0, 1, 512, 255, 1000, k_rows=True)) == "tm1"
    assert predict_kernel(_c(0, 1, 511, 256, 1000, k_rows=True)) == "tm1"
    assert predict_kernel(_c(0, 1, 512, 256, 1001, k_rows=True)) == "tm1"                # lda = 1001
    assert predict_kernel(_c(0, 1, 512, 256, 1001, k_rows=True, lda=1004)) == "dw_x3"
    assert predict_kernel(_c(0, 1, 512, 256, 5000, k_rows=True)) == "tm1"                # 5000 rows in one split
    assert predict_kernel(_c(0, 1, 512, 256, 5000, splits=2, k_rows=True)) == "dw_x3"
    assert predict_kernel(_c(0, 1, 512, 256, 1000, k_rows=True, ldo=258)) == "tm1"
    assert predict_kernel(_c(0, 1, 512, 256, 1000, k_rows=True, a_off=2)) == "tm1"
    assert predict_kernel(_c(0, 1, 512, 256, 1000, k_rows=True, out_off=1)) == "tm1"
    assert predict_kernel(_c(0, 1, 512, 256, 1000, k_rows=True), {"UMLH_F32_X3": "0"}) == "dw"
    assert predict_kernel(_c(0, 1, 512, 256, 1000, k_rows=True), {"UMLH_F32_DW": "0"}) == "tm1"
    assert predict_kernel(_c(0, 0, 0, 10, 10)) is None and predict_kernel(_c(0, 0, 10, 0, 10)) is None


def test_case_operands_are_deterministic_and_place_the_nonfinite_values():
    c = next(c for c in CASES if c["id"] == "19b_nonfinite_tm1")
    A1, B1, r1, _ = build_case(c)
    A2, B2, r2, _ = build_case(c)
    assert A1.tobytes() == A2.tobytes() and B1.tobytes() == B2.tobytes() and (r1 == r2).all()
    Am, Bm = operands(A1, B1, 0, 0, r1, None, c["M"], c["N"], c["K"], c["lda"], c["ldb"])
    assert np.isposinf(Am).any() and np.isneginf(Am).any() and np.isnan(Am).any() and (Am == 0).all(axis=1).any()
    assert (A1.view(np.uint32) == 0x7F800001).any() and (B1.view(np.uint32) == 0x7F800001).any()
    assert np.isposinf(Bm).any() and np.isneginf(Bm).any()
