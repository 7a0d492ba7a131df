"""GPU checks of the outlier-clamp kernels (csrc/umlh_kernels_outlier.hip) through umlh.align and the C ABI: the selections are
bit-equal to np.sort, the clamp to the float64 statement of tests/_outlier_ref.py and to the reference's recorded results, the
normalisation within the measured fp32 bound; every kernel path (a wave per row, a row in LDS, a streamed row; dense, strided,
vector and tail accesses) and every radix pass decides a case."""
import ctypes as C

import numpy as np
import pytest
import torch

import _outlier_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

QS = (0.0, 0.5, 0.95, 0.999)


@pytest.fixture(scope="module")
def A():
    import umlh
    umlh.build_library()
    return umlh.align


@pytest.fixture(scope="module")
def gold():
    return load_golden("outliers")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def data(rng, n, d, ties=True):
    x = rng.standard_normal((n, d)).astype(np.float32)
    if ties and d > 2:
        x[:, ::3] = np.round(x[:, ::3] * 2) / 2          # many equal |x|, both signs, zeros
    return x


def select(A, x_t, q):
    q_val, mean64, quant, lo, hi = A.row_abs_quantile(x_t, q, return_order_stats=True)
    return {"q_val": q_val.cpu().numpy(), "mean64": mean64.cpu().numpy(), "quant": quant.cpu().numpy(), "lo_val": lo.cpu().numpy(),
            "hi_val": hi.cpu().numpy()}


def check_select(A, x_np, x_t, q, what):
    got, ref = select(A, x_t, q), R.row_quantile(x_np, q)
    for k in ("lo_val", "hi_val", "quant"):
        assert np.array_equal(bits(got[k]), bits(ref[k])), (what, q, k)
    fin = ref["quant"].astype(np.float64)
    if np.isnan(fin).any():
        assert np.isnan(got["mean64"]) and np.isnan(got["q_val"]), (what, q)
    else:
        want = fin.sum() / len(fin)
        if np.isfinite(want):
            assert abs(got["mean64"] - want) <= 1e-15 * abs(want), (what, q)
        else:
            assert got["mean64"] == want, (what, q)
        assert bits(got["q_val"]) == bits(np.float32(got["mean64"])), (what, q)
    return got


def widths(A):
    w, l = A.ROW_QUANTILE_WAVE_COLS, A.ROW_QUANTILE_LDS_COLS
    return [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, w - 1, w, w + 1, l - 1, l, l + 1]


@pytest.mark.parametrize("i", range(16))
def test_selection_is_bit_equal_to_sort(A, i):
    d = widths(A)[i]
    rng = np.random.default_rng(100 + d)
    for n in ((2,) if d >= A.ROW_QUANTILE_LDS_COLS - 1 else (1, 2, 7, 300)):
        x = data(rng, n, d)
        x_t = dev(x)
        for q in QS:
            check_select(A, x, x_t, q, (n, d))


def test_selection_strided_rows_and_3d(A):
    rng = np.random.default_rng(7)
    for n, d in ((7, 65), (5, 1000), (3, A.ROW_QUANTILE_WAVE_COLS + 1), (2, A.ROW_QUANTILE_LDS_COLS + 1)):
        x = data(rng, n, d)
        full = torch.full((n, d + 5), float("nan"), device="cuda")
        full[:, :d] = dev(x)
        for q in (0.5, 0.999):
            check_select(A, x, full[:, :d], q, ("strided", n, d))      # a NaN from the gap would make quant NaN
    x3 = rng.standard_normal((6, 5, 7)).astype(np.float32)
    got = check_select(A, x3, dev(x3), 0.95, "3-D")
    assert np.array_equal(bits(got["quant"]), bits(select(A, dev(x3.reshape(6, 35)), 0.95)["quant"]))


def from_bits(k):
    return np.asarray(k, np.uint32).view(np.float32)


def test_every_radix_pass_decides(A):
    rng = np.random.default_rng(11)
    n, d = 5, 300
    sign = lambda: (rng.integers(0, 2, (n, d)).astype(np.uint32) << 31)
    for low_bits in (23, 15, 7):                # keys agree in their top 8, 16, 24 bits: the answer is decided below
        keys = np.uint32(0x3fc00000 & ~((1 << low_bits) - 1)) | rng.integers(0, 1 << low_bits, (n, d)).astype(np.uint32)
        x = from_bits(keys | sign())
        for q in QS:
            check_select(A, x, dev(x), q, ("low bits", low_bits))
    cases = {
        "all equal": np.full((n, d), -1.25, np.float32),
        "integer ties": rng.integers(-3, 4, (n, d)).astype(np.float32),
        "denormals": from_bits(rng.integers(1, 1 << 23, (n, d)).astype(np.uint32) | sign()),
        "zeros": from_bits(sign()),
        "two values": np.where(rng.random((n, d)) < 0.5, 1.0, -2.0).astype(np.float32),
    }
    x = data(rng, n, d); x[1, 17] = np.inf; x[3, 0] = -np.inf
    cases["one inf"] = x
    for what, x in cases.items():
        for q in QS:
            check_select(A, x, dev(x), q, what)
    for d in (300, A.ROW_QUANTILE_WAVE_COLS + 10, A.ROW_QUANTILE_LDS_COLS + 10):      # a NaN row beside clean rows, every kernel
        x = data(rng, 4, d)
        clean = select(A, dev(x), 0.95)
        x[2, d // 2] = np.nan
        got = check_select(A, x, dev(x), 0.95, ("nan row", d))
        keep = [0, 1, 3]
        assert np.array_equal(bits(got["quant"][keep]), bits(clean["quant"][keep])) and np.isnan(got["quant"][2])
        assert np.isnan(got["mean64"]) and np.isnan(got["q_val"])
        assert got["hi_val"][2] >= got["lo_val"][2]                                   # bit order: NaN above Inf, not yet reached


def kth(A, x_t, k):
    return A.abs_kth(x_t, k).cpu().numpy()


def test_global_kth_is_bit_equal_to_sort(A):
    rng = np.random.default_rng(13)
    for shape in ((1, 1), (5, 51), (16, 16), (1, 257), (70001, 1), (1000, 1049), (3, 4, 25)):
        x = data(rng, shape[0], int(np.prod(shape[1:]))).reshape(shape)
        s = np.sort(np.abs(x).ravel())
        x_t = dev(x)
        for k in sorted({0, x.size - 1, *(int(q * x.size) for q in (0.5, 0.95, 0.999))}):
            assert bits(kth(A, x_t, k)) == bits(s[k]), (shape, k)
    x = data(rng, 40, 33)                                                # a strided matrix, NaN in the gap
    full = torch.full((40, 40), float("nan"), device="cuda")
    full[:, :33] = dev(x)
    s = np.sort(np.abs(x).ravel())
    for k in (0, 659, 1319):
        assert bits(kth(A, full[:, :33], k)) == bits(s[k]), ("strided", k)
    flat = torch.empty(40 * 33 + 1, device="cuda")                      # dense rows on a base off 16 bytes: the 4-byte loads
    flat[1:] = dev(x).reshape(-1)
    for k in (0, 659, 1319):
        assert bits(kth(A, flat[1:].view(40, 33), k)) == bits(s[k]), ("unaligned", k)
    keys = np.uint32(0x40490f80) | rng.integers(0, 128, (9, 77)).astype(np.uint32)      # decided in the last pass
    x = from_bits(keys)
    s = np.sort(x.ravel())
    for k in (0, 100, 346, 692):
        assert bits(kth(A, dev(x), k)) == bits(s[k]), ("last pass", k)
    x = data(rng, 10, 30); x[2, 3] = x[7, 7] = x[9, 29] = np.nan          # NaNs order last
    s = np.sort(np.abs(x).ravel())
    assert bits(kth(A, dev(x), 296)) == bits(s[296]) and np.isfinite(s[296])
    for k in (297, 299):
        assert np.isnan(kth(A, dev(x), k)) and np.isnan(s[k])


def clamp_rows(A, x_t, q_val_t, normalize, out_t):
    from umlh import _glue as glue
    from umlh._lib import check, load_library
    n, d = x_t.shape
    check(load_library().umlh_clamp_rows(x_t.data_ptr(), n, d, x_t.stride(0), q_val_t.data_ptr(), int(normalize), out_t.data_ptr(),
                                         out_t.stride(0), glue.stream(x_t.device)), "umlh_clamp_rows")


def test_clamp_is_bit_equal_and_stays_inside_its_output(A):
    rng = np.random.default_rng(17)
    for n, d in ((1, 1), (7, 65), (33, 1027), (3, 4099)):
        x = data(rng, n, d) * 2
        x_t = dev(x)
        q_val = A.row_abs_quantile(x_t, 0.9)[0]
        qv = q_val.cpu().numpy()
        ref = np.clip(x, -qv, qv)
        assert np.array_equal(bits(ref), bits(R.clamp(x, qv))) and (d == 1 or (np.abs(x) > qv).any())
        # dense out of place (16-byte accesses and their tail), one spare NaN row behind the output
        buf = torch.full((n + 1, d), float("nan"), device="cuda")
        clamp_rows(A, x_t, q_val, False, buf[:n])
        got = buf.cpu().numpy()
        assert np.array_equal(bits(got[:n]), bits(ref)) and np.isnan(got[n]).all(), ("dense", n, d)
        # bases off 16 bytes: the 4-byte path
        flat_in, flat_out = torch.empty(n * d + 1, device="cuda"), torch.full((n * d + 1 + d,), float("nan"), device="cuda")
        flat_in[1:] = x_t.reshape(-1)
        clamp_rows(A, flat_in[1:].view(n, d), q_val, False, flat_out[1:1 + n * d].view(n, d))
        got = flat_out.cpu().numpy()
        assert np.array_equal(bits(got[1:1 + n * d]), bits(ref.ravel())) and np.isnan(got[0]) and np.isnan(got[1 + n * d:]).all()
        # own output stride, strided input with NaN in its gap
        full = torch.full((n, d + 3), float("nan"), device="cuda")
        full[:, :d] = x_t
        buf = torch.full((n + 1, d + 7), float("nan"), device="cuda")
        clamp_rows(A, full[:, :d], q_val, False, buf[:n, :d])
        got = buf.cpu().numpy()
        assert np.array_equal(bits(got[:n, :d]), bits(ref)) and np.isnan(got[:n, d:]).all() and np.isnan(got[n]).all(), ("strided", n, d)
        # in place, dense and strided
        y = x_t.clone()
        clamp_rows(A, y, q_val, False, y)
        assert np.array_equal(bits(y.cpu().numpy()), bits(ref))
        clamp_rows(A, full[:, :d], q_val, False, full[:, :d])
        got = full.cpu().numpy()
        assert np.array_equal(bits(got[:, :d]), bits(ref)) and np.isnan(got[:, d:]).all()
        # the wrapper: out= and the default
        assert np.array_equal(bits(A.remove_outliers(x_t, 0.9).cpu().numpy()), bits(ref))
        z = x_t.clone()
        assert A.remove_outliers(z, 0.9, out=z) is z and np.array_equal(bits(z.cpu().numpy()), bits(ref))


def test_clamp_special_values_follow_the_golden_record(A, gold):
    """-0.0, +-Inf and NaN elements, a NaN, an infinite and a zero bound: bit-equal to what the reference returned."""
    for name in gold["cases"]:
        x, out = gold[f"{name}/x"], gold[f"{name}/out"]
        x_t = dev(x.reshape(x.shape[0], -1))
        q_val = dev(np.asarray(gold[f"{name}/q_val"], np.float32).reshape(1))
        full = torch.full((x_t.shape[0], x_t.shape[1] + 3), float("nan"), device="cuda")
        full[:, : x_t.shape[1]] = x_t
        for src in (x_t, full[:, : x_t.shape[1]]):               # the dense and the row-strided kernel path
            got = torch.empty_like(x_t)
            clamp_rows(A, src, q_val, False, got)
            assert np.array_equal(bits(got.cpu().numpy().reshape(x.shape)), bits(out)), name


def test_normalise_against_float64(A):
    rng = np.random.default_rng(19)
    w, l = A.ROW_QUANTILE_WAVE_COLS, A.ROW_QUANTILE_LDS_COLS
    for n, d in ((1, 1), (9, 65), (300, 33), (5, w), (5, w + 1), (2, l), (2, l + 1)):
        x = data(rng, n, d) * 3
        if n > 2:
            x[1] = 0.0                                           # an all-zero row stays zero
        x_t = dev(x)
        q_val = A.row_abs_quantile(x_t, 0.9)[0]
        ref = R.normalize64(R.clamp(x, q_val.cpu().numpy()))
        buf = torch.full((n + 1, d + 4), float("nan"), device="cuda")
        clamp_rows(A, x_t, q_val, True, buf[:n, :d])
        got = buf.cpu().numpy()
        assert R.max_rel(got[:n, :d], ref) <= R.NORM_BOUND, (n, d, R.max_rel(got[:n, :d], ref))
        assert np.isnan(got[:n, d:]).all() and np.isnan(got[n]).all()
        if n > 2:
            assert not got[1, :d].any()
        y = x_t.clone()                                          # in place
        clamp_rows(A, y, q_val, True, y)
        assert np.array_equal(bits(y.cpu().numpy()), bits(got[:n, :d])), (n, d)
    nan_q = dev(np.array([np.nan], np.float32))
    out = torch.zeros(3, 8, device="cuda")
    clamp_rows(A, torch.ones(3, 8, device="cuda"), nan_q, True, out)
    assert torch.isnan(out).all()


def test_end_to_end_against_the_golden_cases(A, gold):
    import metrics
    for name in gold["cases"]:
        x, q, ex = gold[f"{name}/x"], float(gold[f"{name}/q"]), bool(gold[f"{name}/exact"])
        ref, qv = gold[f"{name}/out"], float(gold[f"{name}/q_val"])
        got_t = metrics.remove_outliers(dev(x), q, exact=ex, max_threshold=1.0)
        assert got_t.shape == x.shape and got_t.dtype == torch.float32 and got_t.is_cuda
        got = got_t.cpu().numpy()
        assert np.array_equal(bits(got), bits(R.remove_outliers(x, q, ex))), name          # the statement, bit for bit
        if ex or not np.isfinite(qv):
            assert np.array_equal(bits(got), bits(ref)), name
        else:
            fin = np.isfinite(ref)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), name
            assert np.abs(got[fin].astype(np.float64) - ref[fin]).max(initial=0.0) <= R.QVAL_BOUND * abs(qv), name
            r = A.row_abs_quantile(dev(x), q)
            assert R.rel_diff(gold[f"{name}/rowq"], r[2].cpu().numpy()) <= R.QUANT_BOUND, name
            assert R.rel_diff(gold[f"{name}/q_val"], r[0].cpu().numpy()) <= R.QVAL_BOUND, name
        if np.isfinite(ref).all():
            prep = A.prepare_features(dev(x), q, exact=ex).cpu().numpy()
            assert prep.shape == x.shape
            assert R.max_rel(prep, R.prepare_features(x, q, ex)) <= R.NORM_BOUND, name
            assert np.array_equal(bits(A.prepare_features(dev(x), q, exact=ex, normalize=False).cpu().numpy()), bits(got)), name
    x_t = dev(gold["gauss_64x33_q95_rows/x"])
    assert metrics.remove_outliers(x_t, 1) is x_t and A.remove_outliers(x_t, 1.0) is x_t
    assert R.max_rel(A.prepare_features(x_t, 1.0).cpu().numpy(), R.normalize64(x_t.cpu().numpy())) <= R.NORM_BOUND
    with pytest.raises(ValueError):
        A.remove_outliers(x_t, 0.5, out=torch.empty(3, 3, device="cuda"))


def test_knn_accuracy(A, gold):
    import metrics
    k2, k3 = gold["knn2"], gold["knn3"]
    assert float(A.knn_accuracy(dev(k3))) == R.knn_accuracy(k3)
    assert float(A.knn_accuracy(dev(k3.reshape(30, 16)))) == R.knn_accuracy(k3)
    assert float(A.knn_accuracy(dev(k2))) == R.knn_accuracy(k2)
    got3, got2 = metrics.compute_knn_accuracy(dev(k3)), metrics.compute_knn_accuracy(dev(k2))
    assert got3.ndim == 0 and got3.dtype == torch.float32 and got3.is_cuda
    assert got3.item() == float(gold["acc3"]) and got2.item() == float(gold["acc2"])
    assert float(A.knn_accuracy(torch.zeros(1, 3, dtype=torch.int64))) == 1.0 and float(A.knn_accuracy(torch.ones(1, 3, dtype=torch.int32))) == 0.0
    rng = np.random.default_rng(23)
    big = rng.integers(0, 1200, (1031, 33)).astype(np.int32)              # a ragged last workgroup
    wide = rng.integers(0, 50, (37, 130)).astype(np.int32)               # more than one sweep of the 64 lanes
    for lists in (big, wide):
        assert float(A.knn_accuracy(dev(lists))) == R.knn_accuracy(lists)
        assert float(A.knn_accuracy(dev(lists), whole_table=True)) == R.knn_accuracy_reference(lists)
    a, b = dev(rng.standard_normal((200, 16)).astype(np.float32)), dev(rng.standard_normal((200, 24)).astype(np.float32))
    ka, kb = A.knn(a, 5), A.knn(b, 5)
    assert float(A.knn_accuracy(ka.long()[kb.long()])) == float(A.list_stats(ka, kb)[0]) == float(A.cycle_knn(a, b, 5))


def test_results_are_bitwise_reproducible_across_calls_and_streams(A):
    rng = np.random.default_rng(29)
    x_t = dev(data(rng, 300, 257))
    long_t = dev(data(rng, 3, A.ROW_QUANTILE_WAVE_COLS + 5))
    lists = dev(rng.integers(0, 300, (300, 9)).astype(np.int32))

    def run():
        outs = []
        for t in (x_t, long_t):
            outs += list(A.row_abs_quantile(t, 0.95, return_order_stats=True))
            outs += [A.abs_kth(t, t.numel() // 3), A.remove_outliers(t, 0.95), A.remove_outliers(t, 0.95, exact=True),
                     A.prepare_features(t, 0.95)]
        outs.append(A.knn_accuracy(lists))
        return outs

    first, second = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, third):
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64), b.view(torch.int32 if b.dtype == torch.float32 else torch.int64))
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64), c.view(torch.int32 if c.dtype == torch.float32 else torch.int64))


def test_invalid_arguments_return_before_any_hip_call(A):
    from umlh._lib import load_library
    lib = load_library()
    x = torch.randn(4, 8, device="cuda")
    o = torch.full((4, 8), 7.0, device="cuda")
    s = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p, d = (lambda t: C.c_void_p(t.data_ptr())), C.c_double
    E_INVALID = -1
    bad = [
        lib.umlh_row_abs_quantile(p(x), 4, 8, 7, d(.5), None, None, p(o), None, p(o), p(s), 1 << 16, None),
        lib.umlh_row_abs_quantile(p(x), 4, 8, 8, d(1.0), None, None, p(o), None, p(o), p(s), 1 << 16, None),
        lib.umlh_row_abs_quantile(p(x), 0, 8, 8, d(.5), None, None, p(o), None, p(o), p(s), 1 << 16, None),
        lib.umlh_row_abs_quantile(p(x), 4, 8, 8, d(.5), None, None, p(o), None, p(o), p(s), 0, None),
        lib.umlh_abs_kth(p(x), 4, 8, 8, 32, p(o), p(s), 1 << 16, None),
        lib.umlh_abs_kth(p(x), 4, 8, 8, -1, p(o), p(s), 1 << 16, None),
        lib.umlh_abs_kth(p(x), 4, 8, 8, 0, p(o), p(s), 8, None),
        lib.umlh_clamp_rows(p(x), 4, 8, 8, p(o), 0, p(o), 7, None),
        lib.umlh_clamp_rows(p(x), 4, 8, 8, None, 0, p(o), 8, None),
        lib.umlh_clamp_rows(p(x), 4, 8, 8, p(o), 0, p(x), 16, None),
        lib.umlh_knn_accuracy(p(x), 4, 2, 1, p(o), p(s), 1 << 16, None),
        lib.umlh_knn_accuracy(p(x), 4, 0, 0, p(o), p(s), 1 << 16, None),
    ]
    assert bad == [E_INVALID] * len(bad)
    assert lib.umlh_outlier_scratch_bytes(0, 0, 8) == 0 and lib.umlh_outlier_scratch_bytes(5, 4, 8) == 0
    torch.cuda.synchronize()
    assert (o == 7.0).all() and not s.any()                # nothing was launched
