"""Shared helpers for the tests of the fp32 GEMM entry point umlh_gemm_f32 (include/umlh.h) and of the engine calls built on the
same dispatcher (umlh_logits, umlh_project): a float64 restatement of the contract, the accuracy criterion every fp32 kernel path
must meet, numpy emulations of the product forms the criterion is calibrated on, and the dispatch rules restated in Python.

Criterion.  The error of an output is measured against the float64 result and normalised by the sum of the magnitudes of its
products, S = sum_k |alpha a_mk b_nk| (the scale at which an fp32 sum rounds).  A kernel path passes when
max <= 2^-20 and rms <= 2^-23 over the outputs.  Levels measured on the CPU with the emulations below (K in {64, 1024, 4096},
row magnitudes spread over 10^+-3, four seeds; tests/test_gemm_ref_cpu.py re-measures them):

    product form                                          max               rms
    sequential fp32 fma chain (one rounding per product)  2^-22.0 .. -22.8  2^-25.0 .. -25.2
    x3: six bf16 piece products, fp32 accumulation        2^-22.7 .. -23.5  2^-25.6 .. -25.8
    x3 with the lo pieces dropped                         2^-19.4 .. -16.2  2^-21.2 .. -18.2
    plain bf16 products                                   2^-12.3 .. -9.2   2^-14.1 .. -11.1

The rms bound is the discriminator, with a margin of 3.5x or more on each side; the max bound catches gross
errors on single outputs.
"""
import numpy as np

from test_x3_split_cpu import _rne_bf16, split3     # the numpy restatement of csrc/umlh_common.h: split3_pair

CRIT_MAX = 2.0 ** -20
CRIT_RMS = 2.0 ** -23

KT = 16              # K chunk of the tile kernels (csrc/umlh_common.h)
DWKIDS = 4096        # reduction rows per split whose row ids fit dw_f32's LDS table (csrc/umlh_kernels_f32.hip: KIDS)


# ---------------------------------------------------------------------------------------------------------------------------- #
# the contract in float64
# ---------------------------------------------------------------------------------------------------------------------------- #
def operands(A, B, ta, tb, a_rows, k_rows, M, N, K, lda, ldb):
    """The logical operands of out[m][n] = alpha * sum_k A(m,k) B(n,k) as float64 [M,K] and [N,K] arrays, read from the flat
    fp32 buffers A and B exactly as include/umlh.h describes (strides, transposes, gathers)."""
    A = np.asarray(A, dtype=np.float32).ravel()
    B = np.asarray(B, dtype=np.float32).ravel()
    if ta == 0:
        rows = np.arange(M) if a_rows is None else np.asarray(a_rows, dtype=np.int64)
        Am = A[(rows[:, None] * lda + np.arange(K)[None, :])] if M else np.zeros((0, K), np.float32)
    else:
        Am = A[(np.arange(K)[None, :] * lda + np.arange(M)[:, None])] if M else np.zeros((0, K), np.float32)
    if tb == 0:
        Bm = B[(np.arange(N)[:, None] * ldb + np.arange(K)[None, :])] if N else np.zeros((0, K), np.float32)
    else:
        krows = np.arange(K) if k_rows is None else np.asarray(k_rows, dtype=np.int64)
        Bm = B[(krows[None, :] * ldb + np.arange(N)[:, None])] if N else np.zeros((0, K), np.float32)
    with np.errstate(invalid="ignore"):              # (a signalling NaN payload such as 0x7f800001 converts quietly)
        return Am.astype(np.float64), Bm.astype(np.float64)


def _matmul_nonfinite(Am, Bm):
    """Am @ Bm.T in float64 with IEEE semantics for inf and NaN, whatever the BLAS does with them: the finite products come
    from a BLAS product of the operands with their non-finite entries zeroed, and the non-finite pattern of every output from
    exact counts (0/1 matrix products) of its NaN, +inf and -inf products."""
    fa, fb = np.isfinite(Am), np.isfinite(Bm)
    out = np.where(fa, Am, 0.0) @ np.where(fb, Bm, 0.0).T
    if fa.all() and fb.all():
        return out
    f = lambda x: x.astype(np.float64)
    ia, ib = np.isinf(Am), np.isinf(Bm)
    na, nb = np.isnan(Am), np.isnan(Bm)
    za, zb = Am == 0, Bm == 0
    pa, pb = Am > 0, Bm > 0                       # (NaN compares false: neither positive nor negative)
    ma, mb = Am < 0, Bm < 0
    nan = f(na).sum(1)[:, None] + f(nb).sum(1)[None, :] + f(ia) @ f(zb).T + f(za) @ f(ib).T
    pinf = f(ia & pa) @ f(pb).T + f(ia & ma) @ f(mb).T + f(~ia & pa) @ f(ib & pb).T + f(~ia & ma) @ f(ib & mb).T
    minf = f(ia & pa) @ f(mb).T + f(ia & ma) @ f(pb).T + f(~ia & pa) @ f(ib & mb).T + f(~ia & ma) @ f(ib & pb).T
    out = np.where(pinf > 0, np.inf, out)
    out = np.where(minf > 0, -np.inf, out)
    return np.where((nan > 0) | ((pinf > 0) & (minf > 0)), np.nan, out)


def gemm_ref(A, B, ta, tb, a_rows, k_rows, alpha, M, N, K, lda, ldb):
    """(ref, S): the float64 result [M,N] of umlh_gemm_f32's contract and the sum of its product magnitudes S = sum_k
    |alpha a_mk b_nk| (the criterion's scale; computed over the finite products)."""
    Am, Bm = operands(A, B, ta, tb, a_rows, k_rows, M, N, K, lda, ldb)
    ref = float(alpha) * _matmul_nonfinite(Am, Bm)
    S = abs(float(alpha)) * (np.abs(np.where(np.isfinite(Am), Am, 0.0)) @ np.abs(np.where(np.isfinite(Bm), Bm, 0.0)).T)
    return ref, S


def gemm_err(got, ref, Sabs):
    """(max, rms) of |got - ref| / S over the outputs whose reference is finite.  An output with S = 0 (all products zero) must
    be exactly ref; a non-finite got where ref is finite counts as an infinite error."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    Sabs = np.asarray(Sabs, dtype=np.float64)
    keep = np.isfinite(ref)
    if not keep.any():
        return 0.0, 0.0
    d = np.abs(got[keep] - ref[keep])
    s = Sabs[keep]
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(s > 0, d / np.where(s > 0, s, 1.0), np.where(d == 0, 0.0, np.inf))
    e = np.where(np.isfinite(got[keep]), e, np.inf)
    return float(e.max()), float(np.sqrt(np.mean(e * e)))


def meets_criterion(err):
    mx, rms = err
    return mx <= CRIT_MAX and rms <= CRIT_RMS


def spread_rows(rng, rows, cols, decades=3):
    """Standard normal [rows, cols] fp32 with row magnitudes spread log-uniformly over 10^-decades .. 10^+decades."""
    x = rng.standard_normal((rows, cols)).astype(np.float64)
    x *= 10.0 ** rng.uniform(-decades, decades, (rows, 1))
    return x.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------- #
# product forms, emulated in numpy (the criterion's calibration)
# ---------------------------------------------------------------------------------------------------------------------------- #
def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _chain(pieces_a, pieces_b, pairs, group):
    """out[m][n] = sum_k sum_(i,j) a_i[m,k] b_j[n,k] accumulated sequentially in fp32: k is walked in groups of `group`, and for
    every group each piece pair's partial dot product (exact in float64) is added to the running fp32 sum with one rounding --
    the MFMA's accumulation step (group 16 for v_mfma_f32_32x32x16_bf16; group 1 is a plain fma chain)."""
    M, K = pieces_a[0].shape
    N = pieces_b[0].shape[0]
    acc = np.zeros((M, N), dtype=np.float32)
    a64 = [p.astype(np.float64) for p in pieces_a]
    b64 = [p.astype(np.float64) for p in pieces_b]
    for k0 in range(0, K, group):
        for i, j in pairs:
            acc = _f32(acc.astype(np.float64) + a64[i][:, k0:k0 + group] @ b64[j][:, k0:k0 + group].T)
    return acc


X3_PAIRS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))     # lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi (kernel order)
DROP_LO_PAIRS = ((1, 1), (1, 0), (0, 1), (0, 0))


def emulate(form, Am, Bm):
    """Am [M,K] @ Bm [N,K]^T in one of the product forms: 'fp32' (sequential fma chain, one rounding per product: the worst order
    of an fp32 sum), 'x3' (six piece products on the bf16 MFMA), 'x3_drop_lo' (hi/mid pieces only), 'bf16' (operands rounded to
    bf16, one product each)."""
    Am, Bm = np.asarray(Am, np.float32), np.asarray(Bm, np.float32)
    if form == "fp32":
        return _chain([Am], [Bm], ((0, 0),), 1)
    if form == "bf16":
        return _chain([_rne_bf16(Am)], [_rne_bf16(Bm)], ((0, 0),), 16)
    sa, sb = split3(Am), split3(Bm)
    return _chain(sa, sb, X3_PAIRS if form == "x3" else DROP_LO_PAIRS, 16)


# ---------------------------------------------------------------------------------------------------------------------------- #
# dispatch (csrc/umlh_ops.cpp: umlh_gemm_f32; csrc/umlh_kernels_f32.hip: dw_f32_applies, umlh_f32_launch_gemm)
# ---------------------------------------------------------------------------------------------------------------------------- #
def _cdiv(a, b):
    return -(-a // b)


def slab_count(K, splits):
    """Slabs of a split-K launch: K is cut into chunks of ceil(K / splits) rounded up to the K chunk KT."""
    if splits == 1:
        return 1, K
    chunk = _cdiv(_cdiv(K, splits), KT) * KT
    return _cdiv(K, chunk), chunk


def predict_kernel(case, env=None):
    """The kernel umlh_gemm_f32 runs for `case` under the environment switches `env`:
    'gemm_enc', 'tm1' (gemm_f32 64x64), 'tm2' (gemm_f32 128x128, fp32 MFMA), 'tm2_x3' (128x128, x3 products), 'dw' (dw_f32) or
    'dw_x3' (dw_f32x3); None when M or N is 0 (nothing is launched).

    `case` keys: ta, tb, M, N, K, lda, ldb, ldo, splits, a_rows (bool), k_rows (bool), and optionally a_off / b_off / out_off,
    the operands' base offsets in floats from a 16-byte boundary (default 0).  `env`: UMLH_F32_X3 / UMLH_F32_TM / UMLH_F32_DW."""
    env = env or {}
    x3 = not str(env.get("UMLH_F32_X3", "1")).startswith("0")
    tm_env = int(env.get("UMLH_F32_TM", "0") or 0)
    dw_off = str(env.get("UMLH_F32_DW", "")) != "" and int(env["UMLH_F32_DW"]) == 0
    ta, tb, M, N, K = case["ta"], case["tb"], case["M"], case["N"], case["K"]
    splits = case.get("splits", 1)
    a_rows, k_rows = bool(case.get("a_rows")), bool(case.get("k_rows"))
    if M <= 0 or N <= 0:
        return None
    if not a_rows and not k_rows and not (ta == 1 and tb == 0) and _cdiv(K, splits) <= 512:
        return "gemm_enc"
    ns, chunk = slab_count(K, splits)
    lda, ldb, ldo = case["lda"], case["ldb"], case["ldo"]
    slab_stride = 0 if splits == 1 else M * ldo
    out_off = 0 if splits > 1 else case.get("out_off", 0)          # (split-K: the kernel writes the slabs, 16-B aligned here)
    dw = (not dw_off and ta == 0 and tb == 1 and not a_rows and M * N >= 8 * 128 * 128 and N >= 4 and N % 4 == 0 and lda >= 4
          and chunk <= DWKIDS and lda % 4 == 0 and ldb % 4 == 0 and case.get("a_off", 0) % 4 == 0 and case.get("b_off", 0) % 4 == 0
          and ldo % 4 == 0 and slab_stride % 4 == 0 and out_off % 4 == 0)
    if dw:
        return "dw_x3" if x3 else "dw"
    wg128 = _cdiv(N, 128) * _cdiv(M, 128) * ns
    tm = tm_env if tm_env in (1, 2) else (1 if wg128 < 768 else 2)
    if tm == 1:
        return "tm1"
    return "tm2_x3" if x3 else "tm2"


X3_KERNELS = ("tm2_x3", "dw_x3")


# ---------------------------------------------------------------------------------------------------------------------------- #
# the case table of tests/test_gemm_f32_gpu.py: every kernel path of umlh_gemm_f32 at its ragged edges
# ---------------------------------------------------------------------------------------------------------------------------- #
# Switch settings the GPU test runs the table under (each in a fresh process: the switches are read once per process).
ENVS = {"default": {}, "x3_off": {"UMLH_F32_X3": "0"}, "tm1": {"UMLH_F32_TM": "1"}, "dw_off": {"UMLH_F32_DW": "0"}}


def _case(cid, ta, tb, M, N, K, *, splits=1, lda=None, ldb=None, ldo=None, alpha=1.0, a_table=None, k_table=None, a_off=0,
          b_off=0, nonfinite=False, expect):
    """a_table / k_table: rows of the gathered table (a_rows / k_rows are drawn from it with repeats); a_off / b_off: the operand
    base sits that many floats past a 16-byte boundary; expect: the kernel predicted under the default switches."""
    return dict(id=cid, ta=ta, tb=tb, M=M, N=N, K=K, splits=splits, alpha=alpha,
                lda=lda if lda is not None else (M if ta else K), ldb=ldb if ldb is not None else (N if tb else K),
                ldo=ldo if ldo is not None else N, a_rows=a_table is not None, k_rows=k_table is not None, a_table=a_table,
                k_table=k_table, a_off=a_off, b_off=b_off, nonfinite=nonfinite, expect=expect)


CASES = [
    _case("01_enc_strided", 0, 0, 77, 45, 300, lda=303, ldo=50, alpha=0.37, expect="gemm_enc"),
    _case("02_enc_nt", 0, 1, 130, 66, 512, expect="gemm_enc"),
    _case("03_enc_tt", 1, 1, 65, 129, 200, expect="gemm_enc"),
    _case("04_enc_splitk_ldo", 0, 0, 96, 64, 2000, splits=4, ldo=71, expect="gemm_enc"),
    _case("05_tm1_arows", 0, 0, 200, 100, 333, a_table=300, expect="tm1"),
    _case("06_tm1_krows_n_odd", 0, 1, 100, 130, 700, k_table=900, expect="tm1"),
    _case("07_tm1_tt_long_k", 1, 1, 130, 70, 1500, expect="tm1"),
    _case("08_tm1_krows_no_lds_ids", 0, 1, 64, 96, 5000, k_table=5200, expect="tm1"),
    _case("09_dw", 0, 1, 512, 512, 1000, k_table=1200, alpha=1.0 / 1000, expect="dw_x3"),
    _case("10_dw_ragged", 0, 1, 333, 516, 777, lda=780, k_table=800, expect="dw_x3"),
    _case("11_dw_splitk", 0, 1, 512, 512, 8192, splits=2, k_table=8300, expect="dw_x3"),
    _case("12_tm2_arows_k_odd", 0, 0, 4099, 3203, 1031, a_table=4200, expect="tm2_x3"),
    _case("13_tm2_tt", 1, 1, 3201, 4093, 1031, expect="tm2_x3"),
    _case("14_tm2_krows_n_odd", 0, 1, 4096, 3203, 600, k_table=700, expect="tm2_x3"),
    _case("15_tm2_by_slabs_ldo", 0, 0, 1000, 1000, 20000, splits=12, ldo=1003, expect="tm2_x3"),
    _case("16_tm2_a_unaligned", 0, 0, 4099, 3203, 1031, a_table=4200, a_off=1, expect="tm2_x3"),
    _case("17_dw_b_unaligned", 0, 1, 512, 512, 1000, k_table=1200, alpha=1.0 / 1000, b_off=1, expect="tm1"),
    _case("18a_m0", 0, 0, 0, 5, 3, splits=2, expect=None),
    _case("18b_n0", 0, 0, 5, 0, 3, ldo=2, expect=None),
    _case("18c_1x1x1", 0, 0, 1, 1, 1, expect="gemm_enc"),
    _case("19a_nonfinite_enc", 0, 0, 70, 50, 100, nonfinite=True, expect="gemm_enc"),
    _case("19b_nonfinite_tm1", 0, 0, 100, 70, 200, a_table=150, nonfinite=True, expect="tm1"),
    _case("19c_nonfinite_tm2", 0, 0, 3100, 4100, 64, a_table=3200, nonfinite=True, expect="tm2_x3"),
    _case("19d_nonfinite_dw", 0, 1, 512, 512, 256, k_table=300, nonfinite=True, expect="dw_x3"),
]

SENTINEL_BITS = 0x7FBADBAD        # a NaN payload no kernel produces: the out buffer's fill outside the [M, N] window


def a_index(c, m, k, rows):
    return c["a_off"] + (rows[m] * c["lda"] + k if c["ta"] == 0 else k * c["lda"] + m)


def b_index(c, n, k, krows):
    return c["b_off"] + (n * c["ldb"] + k if c["tb"] == 0 else krows[k] * c["ldb"] + n)


def build_case(c):
    """Operands of a case as flat fp32 buffers (the base offset included) plus the gathers: (A, B, a_rows, k_rows).  Deterministic
    in the case id, so the GPU child and the parent that forms the float64 reference build the same data."""
    rng = np.random.default_rng(sum(ord(ch) for ch in c["id"]) * 7919 + len(c["id"]))
    M, N, K, lda, ldb = c["M"], c["N"], c["K"], c["lda"], c["ldb"]
    a_rows = rng.integers(0, c["a_table"], M).astype(np.int64) if c["a_rows"] else None
    k_rows = rng.integers(0, c["k_table"], K).astype(np.int64) if c["k_rows"] else None
    ra = c["a_table"] if c["a_rows"] else (K if c["ta"] else M)          # stored rows of A ([rows][lda])
    rb = c["k_table"] if c["k_rows"] else (K if c["tb"] else N)
    ra, rb = max(ra, 1), max(rb, 1)                                       # (M = 0 / N = 0: the operands still exist)
    # row magnitudes over 10^+-3 along the output dimension (each stored row of a k-contiguous operand is one m / n; a k-major
    # operand gets its spread along the columns)
    if c["ta"] == 0:
        A = spread_rows(rng, ra, lda)
    else:
        A = spread_rows(rng, lda, ra).T.copy()
    if c["tb"] == 0:
        B = spread_rows(rng, rb, ldb)
    else:
        B = spread_rows(rng, ldb, rb).T.copy()
    A = np.concatenate([np.full(c["a_off"], np.nan, np.float32), A.ravel()])
    B = np.concatenate([np.full(c["b_off"], np.nan, np.float32), B.ravel()])
    if c["nonfinite"]:
        rows = a_rows if a_rows is not None else np.arange(M)
        krows = k_rows if k_rows is not None else np.arange(K)
        nan_lo = np.uint32(0x7F800001).view(np.float32)        # its truncated hi piece is +inf
        ms, ns, ks = rng.choice(M, 6, replace=False), rng.choice(N, 5, replace=False), rng.choice(K, 8, replace=False)
        A[a_index(c, ms[0], ks[0], rows)] = np.inf
        A[a_index(c, ms[1], ks[1], rows)] = -np.inf
        A[a_index(c, ms[2], ks[2], rows)] = np.nan
        A[a_index(c, ms[3], ks[3], rows)] = nan_lo
        for k in range(K):                                       # a zero row of A: its outputs have S = 0
            A[a_index(c, ms[4], k, rows)] = 0.0
        B[b_index(c, ns[0], ks[4], krows)] = np.inf
        B[b_index(c, ns[1], ks[5], krows)] = -np.inf
        B[b_index(c, ns[2], ks[6], krows)] = np.nan
        B[b_index(c, ns[3], ks[7], krows)] = nan_lo
        B[b_index(c, ns[4], ks[0], krows)] = 0.0                  # inf * 0 in A's +inf row
        A[a_index(c, ms[5], ks[4], rows)] = 0.0                  # 0 * inf in B's +inf column
    return A, B, a_rows, k_rows


def case_ref(c):
    """(ref, S) of a case in float64."""
    A, B, a_rows, k_rows = build_case(c)
    A = A[c["a_off"]:]
    B = B[c["b_off"]:]
    return gemm_ref(A, B, c["ta"], c["tb"], a_rows, k_rows, c["alpha"], c["M"], c["N"], c["K"], c["lda"], c["ldb"])
