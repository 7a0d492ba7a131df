"""GPU: the MIMIC loader.  The three kernels of umlh_kernels_tabular.hip through ctypes into NaN-sentinel buffers with a guard
row, ``multibench.mimic`` against what the reference's own loader recorded in tests/golden/mimic*.npz, and a run of
``build_run`` + ``train`` + ``evaluate`` + ``evaluate_robustness`` on the fixture's N = 203 datafile.

Bounds.
  ``umlh_tab_standardize``, stats: the column mean against ``math.fsum`` of the cleaned column / rows, within
      chain(rows) * 2^-53 * mean|term|, chain(rows) the roundings of the kernel's longest fp64 chain by its plan -- c = min(rows,
      256) row chunks of at most ceil(rows / c) rows, four row groups per chunk summed in a chain each (ceil(ceil(rows / c) / 4) - 1
      roundings after the exact first add to 0.0), min(rows per chunk, 4) - 1 to join the groups, c - 1 to join the chunks, 1 for the division --
      which is at most rows for every row count (asserted).  The std: its terms fl((v - mean)^2) are taken from the kernel's own
      mean, all positive, so mean|term| is the variance: relative error of the variance at most (chain + 2) * 2^-53 (one more
      rounding in a term that the compiler may or may not fuse into the add, one for the comparison's own term), of its square
      root half of that plus 2^-53.
  out: within 1 fp32 ulp of float32((clean(x) - np.average) / np.std), numpy's float64 expression, on EVERY element; NaN and
      +-Inf exactly where numpy has them.  The inputs keep |mean| <= 8 std: a relative fp64 perturbation of the statistics of
      rows * 2^-53 then moves the quotient by far less than half an fp32 ulp and can only flip a rounding.
  ``umlh_tab_perturb`` and ``umlh_rows_gather``: equal as uint32 words, no tolerance.  The counter stream: the kept fraction at
      p = 0.3 over 10^5 elements within 5 binomial sigma.
  The loader: tables within 1 ulp of the recorded float64 arrays rounded to fp32 and bit-equal where the recorded value is an
      fp32 number; batches equal to table rows bit for bit; noise levels equal to the numpy statement on the level's own fp32
      rows, the recorded zero pattern exactly.  The run: losses bit-equal to the same run fed host lists.
Every measured figure is printed before it is asserted."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _mimic_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


@pytest.fixture(scope="module")
def lib():
    import umlh
    return umlh.load_library()


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _stream_arg(stream):
    st = torch.cuda.current_stream(DEV) if stream is None else stream
    return st, C.c_void_p(st.cuda_stream)


# ---- umlh_tab_standardize ----
def chain(rows):
    c = min(rows, 256)
    per = -(-rows // c)
    return max(-(-per // 4) - 1, 0) + (min(per, 4) - 1) + (c - 1) + 1


def _standardize(lib, x, ldx=None, ldo=None, in_place=False, stream=None):
    """umlh_tab_standardize on x [rows, d] laid out with row stride ldx in a NaN buffer one row longer; the output in a NaN
    buffer of stride ldo one row longer (the source's own buffer when in_place): (out [rows, d], stats [2, d])."""
    rows, d = x.shape
    ldx, ldo = ldx or d, ldo or d
    src = torch.full((rows + 1, ldx), float("nan"), dtype=torch.float64 if x.dtype == np.float64 else torch.float32, device=DEV)
    src[:rows, :d] = _dev(x)
    before = src.clone()
    if in_place:
        dst, ldo = src, ldx
    else:
        dst = torch.full((rows + 1, ldo), float("nan"), dtype=torch.float32, device=DEV)
    stats = torch.full((2 * d + 1,), float("nan"), dtype=torch.float64, device=DEV)
    need = lib.umlh_tab_standardize_scratch(rows, d)
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    st, sarg = _stream_arg(stream)
    st.wait_stream(torch.cuda.current_stream(DEV))
    rc = lib.umlh_tab_standardize(src.data_ptr(), int(x.dtype == np.float64), rows, d, ldx, dst.data_ptr(), ldo, stats.data_ptr(),
                                  scratch.data_ptr(), need, sarg)
    assert rc == 0, lib.umlh_last_error()
    st.synchronize()
    out, s = dst.cpu().numpy(), stats.cpu().numpy()
    assert np.isnan(out[rows]).all() and np.isnan(out[:, d:]).all() and np.isnan(s[2 * d]), "written outside the output"
    if not in_place:
        assert torch.equal(src.view(torch.uint8), before.view(torch.uint8)), "the source was written"
    return out[:rows, :d].copy(), s[:2 * d].reshape(2, d)


def _columns(rng, rows, d, dtype):
    x = (rng.standard_normal((rows, d)) + rng.uniform(-7.0, 7.0, d)) * rng.uniform(0.1, 30.0, d)       # |mean| <= 8 std
    return x.astype(dtype)


def _plant(rng, x):
    x = x.copy()
    k = max(1, x.size // 50)
    for v in (np.nan, np.inf, -np.inf):
        x.flat[rng.choice(x.size, k, replace=False)] = v
    return x


def _check_standardize(x, out, stats, what, worst):
    rows, d = x.shape
    v = R.clean(x).astype(np.float64)
    with np.errstate(all="ignore"):
        want = ((v - np.average(v, axis=0)) / np.std(v, axis=0)).astype(np.float32)
    dist = R.ulp_distance(out, want)
    assert np.array_equal(np.isnan(out), np.isnan(want)) and np.array_equal(np.isinf(out), np.isinf(want)), what
    worst["ulp"] = max(worst["ulp"], int(dist.max()))
    assert dist.max() <= 1, (what, int(dist.max()))
    k = chain(rows)
    assert k <= rows
    for c in range(d):
        col = v[:, c].tolist()
        mag = math.fsum(abs(t) for t in col) / rows
        err = abs(stats[0, c] - math.fsum(col) / rows)
        if mag > 0:
            worst["mean"] = max(worst["mean"], err / (k * U * mag))
        assert err <= k * U * mag, (what, c, err, k * U * mag)
        terms = ((v[:, c] - stats[0, c]) ** 2).tolist()
        var = math.fsum(terms) / rows
        rel = abs(stats[1, c] - math.sqrt(var)) / math.sqrt(var) if var > 0 else abs(stats[1, c])
        bound = ((k + 2) / 2 + 1) * U
        worst["std"] = max(worst["std"], rel / bound)
        assert rel <= bound, (what, c, rel, bound)


@pytest.mark.parametrize("d", [1, 5, 12, 33])
def test_standardize_against_float64(lib, d):
    rng = np.random.default_rng(300 + d)
    worst = {"ulp": 0, "mean": 0.0, "std": 0.0}
    for rows in (1, 2, 255, 256, 257, 4097):
        for dtype in (np.float32, np.float64):
            x = _columns(rng, rows, d, dtype)
            for xx, how in ((x, {}), (_plant(rng, x), {}), (_plant(rng, x), {"ldx": d + 3, "ldo": d + 2})):
                out, stats = _standardize(lib, xx, **how)
                _check_standardize(xx, out, stats, (rows, d, dtype.__name__, how), worst)
            if dtype == np.float32:
                xx = _plant(rng, x)
                out, stats = _standardize(lib, xx, ldx=d + 1, in_place=True)
                _check_standardize(xx, out, stats, (rows, d, "in place"), worst)
    print(f"d={d}: worst out {worst['ulp']} ulp; worst mean error {worst['mean']:.3f} of its bound, worst std error {worst['std']:.3f} of its bound")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_standardize_constant_column_is_numpy(lib, dtype):
    """A column with std == 0 is not special-cased.  The constants are values whose sums are exact in any order, so the mean is
    the constant itself for numpy and for the kernel alike: 0 / 0 = NaN.  v / 0 = +-Inf needs v != mean at std == 0, which only
    an underflow of (v - mean)^2 gives: +-1e-200 in a double source."""
    rng = np.random.default_rng(7)
    for rows in (2, 257, 4096):
        x = _columns(rng, rows, 5, dtype)
        x[:, 1], x[:, 3] = 2.5, 0.0
        x[0, 3] = np.nan                                           # cleaned to the column's own constant
        if dtype == np.float64:
            x[:, 4] = np.where(np.arange(rows) % 2, -1e-200, 1e-200)
        out, stats = _standardize(lib, x)
        v = R.clean(x).astype(np.float64)
        with np.errstate(all="ignore"):
            want = ((v - np.average(v, axis=0)) / np.std(v, axis=0)).astype(np.float32)
        assert stats[0, 1] == 2.5 and stats[1, 1] == 0.0 and stats[0, 3] == 0.0 and stats[1, 3] == 0.0
        assert np.isnan(out[:, [1, 3]]).all() and np.isnan(want[:, [1, 3]]).all() and np.isfinite(out[:, [0, 2]]).all()
        if dtype == np.float64:
            assert abs(stats[0, 4]) <= 1e-200 and stats[1, 4] == 0.0 and np.array_equal(out[:, 4], want[:, 4])
            assert np.isposinf(out[0::2, 4]).all() and np.isneginf(out[1::2, 4]).all()
        assert R.ulp_distance(out, want).max() <= 1


@pytest.mark.parametrize("rows,d", [(1, 5), (257, 5), (4097, 12), (1000, 33)])
def test_standardize_equals_column_standardize_on_finite_fp32(lib, rows, d):
    from umlh import seqload
    x = _columns(np.random.default_rng(rows + d), rows, d, np.float32)
    out, stats = _standardize(lib, x)
    want, want_stats = seqload.column_standardize(_dev(x).view(rows, 1, d))
    assert np.array_equal(stats.view(np.uint64), want_stats.cpu().numpy().view(np.uint64))
    assert np.array_equal(_bits(out), _bits(want.view(rows, d).cpu().numpy()))


def test_standardize_is_reproducible_across_calls_and_streams(lib):
    rng = np.random.default_rng(5)
    side = torch.cuda.Stream(DEV)
    for dtype in (np.float32, np.float64):
        x = _plant(rng, _columns(rng, 4097, 12, dtype))
        a, b, c = _standardize(lib, x), _standardize(lib, x), _standardize(lib, x, stream=side)
        for other in (b, c):
            assert np.array_equal(_bits(a[0]), _bits(other[0])) and np.array_equal(a[1].view(np.uint64), other[1].view(np.uint64))


def test_wrapper_standardizes_views_and_float64():
    from umlh import seqload
    rng = np.random.default_rng(9)
    x = _plant(rng, _columns(rng, 300, 12, np.float64))
    wide = torch.full((300, 16), float("nan"), dtype=torch.float64, device=DEV)
    wide[:, :12] = _dev(x)
    out, stats = seqload.tab_standardize(wide[:, :12])
    ref, ref_stats = seqload.tab_standardize(_dev(x))
    assert out.dtype == torch.float32 and torch.equal(out.view(torch.int32), ref.view(torch.int32)) and torch.equal(stats, ref_stats)
    x32 = _dev(x, np.float32)
    keep = x32.clone()
    same, _ = seqload.tab_standardize(x32, out=x32)
    other, _ = seqload.tab_standardize(keep)
    assert same.data_ptr() == x32.data_ptr() and torch.equal(same.view(torch.int32), other.view(torch.int32))
    with pytest.raises(Exception, match="aliases"):
        d64 = _dev(x)
        seqload.tab_standardize(d64, out=d64.view(torch.float32)[:, :12])


# ---- umlh_tab_perturb ----
def _special(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    kind = rng.integers(0, 14, x.shape)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40)):
        x[kind == k] = v
    w = x.view(np.uint32)
    w[kind == 6] = 0x7FC12345                                      # a NaN with a payload: moved, not computed on
    return x


def _perturb(lib, x, drop, carry, in_place=False, lds=None, ldd=None, p_drop=0.0, p_carry=0.0, seed=0, stream=None):
    n, d = x.shape
    lds, ldd = lds or d, ldd or d
    src = torch.full((n + 1, lds), float("nan"), dtype=torch.float32, device=DEV)
    src[:n, :d] = _dev(x)
    before = src.clone()
    if in_place:
        dst, ldd = src, lds
    else:
        dst = torch.full((n + 1, ldd), float("nan"), dtype=torch.float32, device=DEV)
    dm = None if drop is None else _dev(drop, np.uint8)
    cm = None if carry is None else _dev(carry, np.uint8)
    st, sarg = _stream_arg(stream)
    st.wait_stream(torch.cuda.current_stream(DEV))
    rc = lib.umlh_tab_perturb(src.data_ptr(), n, d, lds, None if dm is None else dm.data_ptr(), None if cm is None else cm.data_ptr(),
                              C.c_float(p_drop), C.c_float(p_carry), seed, dst.data_ptr(), ldd, sarg)
    assert rc == 0, lib.umlh_last_error()
    st.synchronize()
    out = dst.cpu().numpy()
    assert np.isnan(out[n]).all() and np.isnan(out[:, d:]).all(), "written outside the rows"
    if not in_place:
        assert torch.equal(src.view(torch.int32), before.view(torch.int32)), "the source was written"
    return out[:n, :d].copy()


def _masks(rng, n, d, kind):
    if kind == "zeros":
        return np.zeros((n, d), np.uint8), np.zeros((n, max(d - 1, 0)), np.uint8)
    if kind == "ones":
        return np.ones((n, d), np.uint8), np.ones((n, max(d - 1, 0)), np.uint8)
    if kind == "runs":                                             # few drops, long carry runs: they cross every 64-column edge
        return (rng.random((n, d)) < 0.05).astype(np.uint8), (rng.random((n, max(d - 1, 0))) < 0.97).astype(np.uint8)
    return (rng.random((n, d)) < 0.3).astype(np.uint8), (rng.random((n, max(d - 1, 0))) < 0.3).astype(np.uint8)


@pytest.mark.parametrize("d", [1, 2, 5, 64, 65, 200])
def test_perturb_is_the_statement_word_for_word(lib, d):
    rng = np.random.default_rng(400 + d)
    for n in (1, 2, 63, 64, 65, 1000):
        x = _special(rng, n, d)
        for kind in ("zeros", "ones", "random", "runs"):
            drop, carry = _masks(rng, n, d, kind)
            hows = [{}] if n not in (65, 1000) else [{}, {"in_place": True}, {"lds": d + 3, "ldd": d + 1}, {"in_place": True, "lds": d + 2}]
            for how in hows:
                for dm, cm in ((drop, carry), (drop, None), (None, carry)):
                    got = _perturb(lib, x, dm, cm if d > 1 else None, **how)
                    want = R.tabular(x, dm, cm if d > 1 else None)
                    assert np.array_equal(_bits(got), _bits(want)), (n, d, kind, how, dm is None, cm is None)
    x = _special(rng, 65, d)
    assert np.array_equal(_bits(_perturb(lib, x, None, None)), _bits(x))                       # nothing asked: the identity on the bits


def test_perturb_carry_runs_cross_every_chunk_edge(lib):
    rng = np.random.default_rng(11)
    n, d = 9, 200
    x = _special(rng, n, d)
    x[:, [0, 63, 64, 127, 128, 191, 192]] = np.arange(1, 8, dtype=np.float32)                  # known values at the edges
    carry = np.zeros((n, d - 1), np.uint8)
    carry[0, :] = 1                                                # one run over the whole row
    carry[1, 60:70] = 1                                            # columns 61..70 take column 60: across 64
    carry[2, 63] = 1                                               # column 64 alone takes 63: the first lane of a chunk
    carry[3, 62:192] = 1                                           # across 64, 128 and 192, two whole chunks inside
    carry[4, 127:129], carry[4, 191:193] = 1, 1
    carry[5, 64:128] = 1                                           # a whole chunk and the next one's first lane (65..128)
    carry[6, 0:63] = 1                                             # all of chunk 0, ends at the edge
    carry[7, 191:] = 1                                             # into the partial last chunk
    drop = np.zeros((n, d), np.uint8)
    drop[3, 62], drop[8, :] = 1, 1
    carry[8, ::2] = 1
    for how in ({}, {"in_place": True}, {"lds": d + 5, "ldd": d + 1}):
        got = _perturb(lib, x, drop, carry, **how)
        assert np.array_equal(_bits(got), _bits(R.tabular(x, drop, carry))), how
    assert (got[0] == got[0, 0]).all() or np.isnan(got[0, 0])
    assert _bits(got[3, 63:193]).tolist() == [0] * 130             # the dropped column 62 carried over three edges as +0.0


def test_perturb_counter_stream(lib):
    n, d, seed, p = 1000, 100, 12345, 0.3
    ones = np.ones((n, d), np.float32)

    def dropout(sd, shape=(n, d)):
        """the elements umlh_dropout zeroes in a table of ones of this shape on stream ``sd``"""
        words = shape[0] * shape[1]
        t = torch.ones(words, dtype=torch.float32, device=DEV)
        assert lib.umlh_dropout(t.data_ptr(), words, C.c_float(p), sd, _stream_arg(None)[1]) == 0
        torch.cuda.synchronize()
        return (t.cpu().numpy() == 0).reshape(shape)
    got = _perturb(lib, ones, None, None, p_drop=p, seed=seed)
    assert np.array_equal(got == 0, dropout(seed))                                             # umlh_dropout's own decisions
    kept = float((got != 0).mean())
    sigma = math.sqrt(p * (1 - p) / (n * d))
    print(f"kept fraction {kept:.5f} at p = {p} over {n * d} elements: {(kept - (1 - p)) / sigma:+.2f} sigma")
    assert abs(kept - (1 - p)) <= 5 * sigma
    rng = np.random.default_rng(3)
    x = _special(rng, n, d)
    both = _perturb(lib, x, None, None, p_drop=p, p_carry=p, seed=seed)
    want = R.tabular(x, dropout(seed), dropout(seed + 1)[:, 1:])                               # carry: the stream seed + 1 at i * d + j
    assert np.array_equal(_bits(both), _bits(want))
    side = torch.cuda.Stream(DEV)
    assert np.array_equal(_bits(both), _bits(_perturb(lib, x, None, None, p_drop=p, p_carry=p, seed=seed)))
    assert np.array_equal(_bits(both), _bits(_perturb(lib, x, None, None, p_drop=p, p_carry=p, seed=seed, stream=side)))
    assert np.array_equal(_bits(both), _bits(_perturb(lib, x, None, None, p_drop=p, p_carry=p, seed=seed, in_place=True)))
    assert not np.array_equal(_bits(both), _bits(_perturb(lib, x, None, None, p_drop=p, p_carry=p, seed=seed + 7)))
    assert np.array_equal(_bits(_perturb(lib, x, None, None, p_drop=0.0, p_carry=0.0, seed=seed)), _bits(x))      # p = 0: the identity
    assert (_bits(_perturb(lib, x, None, None, p_drop=1.0, seed=seed)) == 0).all()             # p = 1 drops everything
    all_carry = _perturb(lib, x, None, None, p_carry=1.0, seed=seed)
    assert np.array_equal(_bits(all_carry), np.repeat(_bits(x[:, :1]), d, axis=1))
    mask = (rng.random((n, d)) < 0.5).astype(np.uint8)                                         # a given mask wins over its p
    assert np.array_equal(_bits(_perturb(lib, x, mask, None, p_drop=1.0, seed=seed)), _bits(R.tabular(x, mask, None)))
    wide = _special(rng, 70, 200)                                                              # the wave-per-row path draws the same stream
    assert np.array_equal(_bits(_perturb(lib, wide, None, None, p_drop=p, p_carry=p, seed=seed)),
                          _bits(R.tabular(wide, dropout(seed, wide.shape), dropout(seed + 1, wide.shape)[:, 1:])))


# ---- umlh_rows_gather ----
def _gather(lib, tables, ids, stream=None):
    """tables: list of [n, w] float32 arrays or None; -> blocks ([b, w] or None), each written into a NaN buffer with a guard row."""
    n = next(t for t in tables if t is not None).shape[0]
    b, k = len(ids), len(tables)
    dev = [None if t is None else _dev(t) for t in tables]
    bufs = [None if t is None else torch.full((b + 2, t.shape[1]), float("nan"), dtype=torch.float32, device=DEV) for t in tables]
    srcs = (C.c_void_p * k)(*[None if t is None else t.data_ptr() for t in dev])
    outs = (C.c_void_p * k)(*[None if t is None else t[1:].data_ptr() for t in bufs])
    widths = (C.c_int32 * k)(*[-5 if t is None else t.shape[1] for t in tables])               # a skipped source's width is not read
    idv = _dev(np.asarray(ids, dtype=np.int64))
    st, sarg = _stream_arg(stream)
    st.wait_stream(torch.cuda.current_stream(DEV))
    rc = lib.umlh_rows_gather(srcs, widths, k, n, idv.data_ptr(), b, outs, sarg)
    assert rc == 0, lib.umlh_last_error()
    st.synchronize()
    res = []
    for t in bufs:
        if t is None:
            res.append(None)
            continue
        a = t.cpu().numpy()
        assert np.isnan(a[0]).all() and np.isnan(a[b + 1]).all(), "a guard row was written"
        res.append(a[1:b + 1].copy())
    return res


@pytest.mark.parametrize("widths", [(5, 288), (1,), (3, 7, 300), (5, None, 288), (None, 1300)])
def test_rows_gather_is_exact(lib, widths):
    rng = np.random.default_rng(sum(w or 0 for w in widths))
    n = 57
    tables = [None if w is None else _special(rng, n, w) for w in widths]
    side = torch.cuda.Stream(DEV)
    for b in (1, 40, 129):
        ids = rng.integers(0, n, b)
        if b > 1:
            ids[[0, b // 2, b - 1]] = (-1, n, ids[1])                                          # out of range twice, one repeated
        for stream in (None, side):
            got = _gather(lib, tables, ids, stream)
            for t, g in zip(tables, got):
                if t is None:
                    assert g is None
                    continue
                live = (ids >= 0) & (ids < n)
                want = np.where(live[:, None], _bits(t)[np.clip(ids, 0, n - 1)], 0)
                assert np.array_equal(_bits(g), want), (widths, b)


def test_rows_gather_wrapper_takes_tables_with_trailing_dimensions():
    from umlh import seqload
    rng = np.random.default_rng(2)
    st, se = _dev(_special(rng, 31, 5)), _dev(_special(rng, 31, 288)).view(31, 24, 12)
    ids = torch.tensor([3, 3, 30, 0, -1, 31], dtype=torch.int64, device=DEV)
    a, b = seqload.rows_gather([st, se], ids)
    assert a.shape == (6, 5) and b.shape == (6, 24, 12)
    assert torch.equal(a[:4].view(torch.int32), st[ids[:4]].view(torch.int32)) and torch.equal(b[:4].view(torch.int32), se[ids[:4]].view(torch.int32))
    assert (a[4:].view(torch.int32) == 0).all() and (b[4:].view(torch.int32) == 0).all()
    only, skipped = seqload.rows_gather([se, None], ids)
    assert skipped is None and torch.equal(only.view(torch.int32), b.view(torch.int32))


# ---- the loader against the fixture ----
@pytest.fixture(scope="module")
def tables(fx):
    from multibench.mimic import MimicTable
    out = {}
    for case in R.CASES:
        df = R.datafile(fx, case)
        before = {k: v.copy() for k, v in df.items()}
        out[case] = MimicTable(df, 7, DEV)
        assert all(R.same_bits(df[k], before[k]) for k in df), "the caller's arrays were modified"
    return out


@pytest.mark.parametrize("case", R.CASES)
def test_tables_are_the_recorded_arrays_rounded_once(fx, tables, case):
    tb = tables[case]
    n = R.config(fx, case)[0]
    assert tb.static.shape == (n, 5) and tb.series.shape == (n, 24, 12) and tb.static.dtype == tb.series.dtype == torch.float32
    for got, name in ((tb.static, "static"), (tb.series, "series")):
        want64 = fx[f"{case}/std/{name}"]
        got, want = got.cpu().numpy(), want64.astype(np.float32)
        dist = R.ulp_distance(got, want)
        exact = (want.astype(np.float64) == want64) | np.isnan(want64)
        print(f"{case} {name}: worst {int(dist.max())} ulp, {int((dist > 0).sum())} of {dist.size} elements differ, {int(exact.sum())} exactly representable")
        assert dist.max() <= 1 and (dist[exact] == 0).all()
    assert (tb.valid, tb.test, tb.train) == tuple(fx[f"{case}/split/{s}"].tolist() for s in ("valid", "test", "train"))
    for s, idx in (("valid", tb.valid), ("test", tb.test), ("train", tb.train)):
        assert np.array_equal(tb.labels[idx], fx[f"{case}/labels/7/{s}"])


@pytest.mark.parametrize("case", R.CASES)
def test_batches_in_the_recorded_order(fx, tables, case):
    from multibench.mimic import get_dataloader
    tb = tables[case]
    _, bs, _, tseed = R.config(fx, case)
    static, series = tb.static.cpu().numpy(), tb.series.cpu().numpy()
    for name in ("plain", "shuffled"):
        trains, valids, _ = get_dataloader(7, bs, train_shuffle=name == "shuffled", table=tb, reference_layout=True,
                                           tabular_robust=False, timeseries_robust=False)
        torch.manual_seed(tseed)                                   # the reference's loader draws from torch's global generator
        got = list(trains)
        index = fx[f"{case}/epoch/{name}/index"]
        assert [b[0].shape[0] for b in got] == fx[f"{case}/epoch/{name}/sizes"].tolist() and len(got) == len(trains)
        off = 0
        for st, se, y in got:
            idx = index[off:off + st.shape[0]]
            off += st.shape[0]
            assert st.is_cuda and se.is_cuda and not y.is_cuda and se.shape[1:] == (24, 12) and y.shape == (st.shape[0],)
            assert np.array_equal(_bits(st.cpu().numpy()), _bits(static[idx])) and np.array_equal(_bits(se.cpu().numpy()), _bits(series[idx]))
            assert np.array_equal(y.numpy(), tb.labels[idx])
        for which, b in (("first", got[0]), ("last", got[-1])):
            assert R.ulp_distance(b[0].cpu().numpy(), fx[f"{case}/epoch/{name}/{which}/static"].astype(np.float32)).max() <= 1
            assert R.ulp_distance(b[1].cpu().numpy(), fx[f"{case}/epoch/{name}/{which}/series"].astype(np.float32)).max() <= 1
            assert np.array_equal(b[2].numpy(), fx[f"{case}/epoch/{name}/{which}/labels"])
    v = list(valids)
    assert np.array_equal(np.concatenate([b[2].numpy() for b in v]), fx[f"{case}/labels/7/valid"])


def _whole(loader):
    batches = list(loader)
    return [np.concatenate([b[k].cpu().numpy() for b in batches]) for k in range(3)]


@pytest.mark.parametrize("case", R.CASES)
def test_noise_levels_against_the_recording_and_the_statement(fx, tables, case):
    from multibench.mimic import get_dataloader
    tb = tables[case]
    _, bs, seed, _ = R.config(fx, case)
    _, _, tests = get_dataloader(7, bs, table=tb, rng=seed, reference_layout=True)
    levels = tests["timeseries"]
    assert len(levels) == 11
    static, series = tb.static.cpu().numpy()[tb.test], tb.series.cpu().numpy()[tb.test]
    drawn = R.draws(len(tb.test), seed)
    for k in R.RECORDED:
        st, se, y = _whole(levels[k])
        assert np.array_equal(st == 0, fx[f"{case}/level/{k}/static"] == 0) and np.array_equal(se == 0, fx[f"{case}/level/{k}/series"] == 0)
        assert np.array_equal(y, fx[f"{case}/level/{k}/labels"])
        lv = drawn[k]
        assert np.array_equal(_bits(st), _bits(R.tabular(static, lv["drop"], lv["carry"])))
        assert R.same_values(se, R.series_noise(series, lv["eps"], lv["elem"], lv["keep"], np.float32))
    assert levels._last[0] == R.RECORDED[-1]                       # one level's tables at a time


def test_a_disabled_family_consumes_no_draws_on_the_device(fx, tables):
    from multibench.mimic import get_dataloader
    tb = tables["n57"]
    _, bs, seed, _ = R.config(fx, "n57")
    static, series = tb.static.cpu().numpy()[tb.test], tb.series.cpu().numpy()[tb.test]
    _, _, tests = get_dataloader(7, bs, table=tb, rng=seed, reference_layout=True, tabular_robust=False)
    st, se, _ = _whole(tests["timeseries"][3])
    lv = R.draws(len(tb.test), seed, tabular_robust=False)[3]
    assert np.array_equal(_bits(st), _bits(static)) and R.same_values(se, R.series_noise(series, lv["eps"], lv["elem"], lv["keep"], np.float32))
    assert np.array_equal(se == 0, fx["n57/notab/series"] == 0)
    _, _, tests = get_dataloader(7, bs, table=tb, rng=seed, reference_layout=True, timeseries_robust=False)
    st, se, _ = _whole(tests["timeseries"][3])
    lv = R.draws(len(tb.test), seed, timeseries_robust=False)[3]
    assert np.array_equal(_bits(se), _bits(series)) and np.array_equal(_bits(st), _bits(R.tabular(static, lv["drop"], lv["carry"])))
    assert np.array_equal(st == 0, fx["n57/nots/static"] == 0)


def test_layouts_flatten_and_deep_copy(fx, tables):
    from multibench.mimic import get_dataloader
    tb = tables["n57"]
    trains, valids, tests = get_dataloader(7, 8, table=tb, generator=torch.Generator().manual_seed(5), rng=1)
    c = copy.deepcopy(trains)
    state = trains.generator.get_state().clone()
    replay = list(c)
    assert torch.equal(trains.generator.get_state(), state)        # the copy has its own generator
    epoch = list(trains)
    assert len(epoch) == len(replay) == len(trains) == 6
    static, series = tb.static, tb.series
    for (xs, ls, inds, y), (xs2, ls2, inds2, y2) in zip(epoch, replay):
        b = inds.shape[0]
        assert torch.equal(inds, inds2) and torch.equal(y, y2) and torch.equal(xs[0], xs2[0]) and torch.equal(xs[2], xs2[2])
        assert xs[1] is None and ls[1] is None and xs[0].shape == (b, 1, 5) and xs[2].shape == (b, 24, 12)
        assert inds.shape == (b, 1) and y.shape == (b, 1) and not inds.is_cuda and not y.is_cuda
        assert ls[0].tolist() == [1] * b and ls[2].tolist() == [24] * b and ls[0].dtype == torch.int64 and ls[0].is_cuda
        rows = torch.tensor(tb.train)[inds.view(-1)].to(DEV)
        assert torch.equal(xs[0][:, 0].view(torch.int32), static[rows].view(torch.int32))
        assert torch.equal(xs[2].view(torch.int32), series[rows].view(torch.int32))
        assert np.array_equal(y.view(-1).numpy(), tb.labels[np.asarray(tb.train)[inds.view(-1).numpy()]])
    assert [b[2].view(-1).tolist() for b in trains] != [b[2].view(-1).tolist() for b in epoch]      # the next epoch is another order
    flat_tr, _, flat_te = get_dataloader(7, 8, table=tb, train_shuffle=False, flatten_time_series=True, rng=1)
    plain_tr, _, _ = get_dataloader(7, 8, table=tb, train_shuffle=False, tabular_robust=False, timeseries_robust=False)
    for a, b in zip(flat_tr, plain_tr):
        assert a[0][2].shape == (a[2].shape[0], 288) and torch.equal(a[0][2].view(-1, 24, 12).view(torch.int32), b[0][2].view(torch.int32))
    lv = list(flat_te["timeseries"][3])
    assert lv[0][0][2].shape[1] == 288 and sum(b[2].shape[0] for b in lv) == len(tb.test)
    assert len(tests["timeseries"][-1]) == len(tests["timeseries"][0]) and len(tests["timeseries"][2:5]) == 3
    with pytest.raises(ValueError, match="task"):                  # a table carries the labels of the task it was built for
        get_dataloader(3, 8, table=tb)


# ---- end to end on the N = 203 datafile ----
class _ListLoader(list):
    batch_size = 128


def _host(batch):
    cpu = lambda t: None if t is None else t.cpu()
    return [cpu(x) for x in batch[0]], [cpu(l) for l in batch[1]], batch[2], batch[3]


RESULT_KEYS = {"val/modality_separate", "test/score_x", "test/score_y", "test/score_xy", "val/score_x", "val/score_y", "val/score_xy",
               "val/loss_x", "test/loss_x", "val/loss_y", "test/loss_y"}
RAW_KEYS = {"val/score_x_raw", "val/score_y_raw", "test/score_x_raw", "test/score_y_raw", "test/score_xy_raw", "val/score_xy_raw"}


def _run(fx, task, seed=3):
    from multibench.mimic import build_run
    torch.manual_seed(seed)                                        # the model's initial weights
    return build_run(R.datafile(fx, "n203"), 20, task=task, generator=torch.Generator().manual_seed(1),
                     generator_2=torch.Generator().manual_seed(2), rng=4321, device=DEV)


@pytest.fixture(scope="module")
def trained(fx):
    from multibench.train import train
    run = _run(fx, 7)
    assert run["ds_name"] == "mimic_icd9" and run["ds_name"] != "mimic" and run["indims"] == [5, 12] and run["batch_size"] == 128
    cfg = run["eval_config"]
    assert cfg["test"] is cfg["val"] and cfg["ds_name"] == run["ds_name"] and cfg["freq"] == 100        # 'test' IS the valid loader
    assert sum(b[2].shape[0] for b in cfg["train"]) == 163 and cfg["train"][0][2].shape[0] == 40 and len(run["train_loader"]) == 2
    torch.manual_seed(11)                                          # the seed of the encoder's dropout masks
    res = train(run["model"], "xy", run["train_loader"], run["train_loader_2"], run["optimizer"], num_epoch=1, step_k=-1,
                ds_name=run["ds_name"], eval_config=cfg, device=DEV)
    return run, res


def test_build_run_and_train_equal_the_same_run_fed_host_lists(fx, trained):
    from multibench.train import train
    run, res = trained
    print("loss", res["loss"])
    assert len(res["loss"]) == 2 and all(np.isfinite(v) for v in res["loss"])
    assert [e[:2] for e in res["eval"]] == [(0, 0), (0, None)]
    for _, _, scores in res["eval"]:
        assert set(scores) == RESULT_KEYS | RAW_KEYS and all(0.0 <= scores[k] <= 1.0 for k in scores if "score" in k)
    assert set(res["raw"]) == RAW_KEYS
    other = _run(fx, 7)
    host_1, host_2 = (_ListLoader(_host(b) for b in other[k]) for k in ("train_loader", "train_loader_2"))
    torch.manual_seed(11)
    host = train(other["model"], "xy", host_1, host_2, other["optimizer"], num_epoch=1, step_k=-1, ds_name=other["ds_name"],
                 eval_config=other["eval_config"], device=DEV)
    for k in ("loss_x", "loss_y", "loss"):
        assert res[k] == host[k], k
    assert res["eval"][-1][2] == host["eval"][-1][2]


def test_evaluate_robustness_over_the_eleven_levels(fx, trained):
    from multibench.train import evaluate, evaluate_raw_data, evaluate_robustness
    run, _ = trained
    cfg, name = run["eval_config"], run["ds_name"]
    assert set(evaluate_raw_data(cfg, ds_name=name, device=DEV, label_fn=cfg["label_fn"])) == RAW_KEYS
    # level 0 (eps = 0.0, nothing dropped) against evaluate on the CLEAN test split: a loader of its own over the table's
    # test rows, which no noise kernel has touched
    from multibench.mimic import MimicLoader
    tb = run["table"]
    levels = run["robust"]["timeseries"]
    clean_loader = MimicLoader(tb.static, tb.series, tb.test, tb.labels[np.asarray(tb.test)], 40)
    clean_batches = list(clean_loader)
    level0 = list(levels[0])
    assert len(clean_batches) == len(level0) == 1 and clean_batches[0][0][0].data_ptr() != level0[0][0][0].data_ptr()
    for a, b in zip(clean_batches, level0):                       # level 0 is the clean rows (x + 0.0 == x), in the same order
        assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[0][2], b[0][2]) and torch.equal(a[3], b[3])
    base = evaluate(run["model"], dict(cfg, test=clean_batches), name, device=DEV, label_fn=cfg["label_fn"])
    assert set(k for k in base if not ("private" in k or "complete" in k)) == RESULT_KEYS
    rob = evaluate_robustness(run["model"], cfg, {"timeseries": levels}, name, device=DEV, label_fn=cfg["label_fn"])
    for k in ("x", "y", "xy"):
        curve = rob[f"robust/timeseries/score_{k}"]
        print(k, curve)
        assert len(curve) == 11 and curve[0] == base[f"test/score_{k}"]
    for k in ("loss_x", "loss_y"):
        print(k, rob[f"robust/timeseries/{k}"][0], base[f"test/{k}"])
        assert len(rob[f"robust/timeseries/{k}"]) == 11 and rob[f"robust/timeseries/{k}"][0] == base[f"test/{k}"]
    assert rob["robust/timeseries/loss_x"][3] != base["test/loss_x"] and rob["robust/timeseries/loss_y"][3] != base["test/loss_y"]
    assert rob["robust/timeseries/n"] == [20] * 11
    with pytest.raises(NotImplementedError):                      # the name 'mimic' behaves as before
        evaluate(run["model"], cfg, "mimic", device=DEV)


def test_mortality_task_takes_the_softmax_probes(fx):
    from multibench.train import evaluate
    from umlh.probe import SoftmaxProbe
    run = _run(fx, -1)
    assert run["ds_name"] == "mimic_mortality"
    cfg = run["eval_config"]
    lab = np.concatenate([np.asarray(cfg["label_fn"](b[3].numpy())).reshape(-1) for b in cfg["train"]])
    assert lab.dtype == np.int64 and len(np.unique(lab)) == 6
    res, _, clfs = evaluate(run["model"], cfg, run["ds_name"], device=DEV, return_embeddings=True, label_fn=cfg["label_fn"])
    assert set(k for k in res if not ("private" in k or "complete" in k)) == RESULT_KEYS
    assert all(isinstance(c, SoftmaxProbe) for c in clfs[3:]) and not any(isinstance(c, SoftmaxProbe) for c in clfs[:3])
