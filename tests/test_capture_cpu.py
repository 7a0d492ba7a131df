"""CPU-side checks of the embedding capture: the ABI v10 entry points are exported and reject bad arguments before any HIP
call, the float64 references of tests/_capture_ref.py are themselves right, and multibench.capture.take_fixed_samples (host
code) makes the reference's selection."""
import ctypes as C

import numpy as np
import pytest
import torch

import _capture_ref as R

E_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_exports_and_version(lib):
    for name in ("umlh_seq_compact", "umlh_paired_cosine_scratch_bytes", "umlh_paired_cosine"):
        assert hasattr(lib, name), name
    assert lib.umlh_version() >= 10
    import umlh
    assert umlh.seq_compact is umlh.capture.seq_compact and umlh.paired_cosine is umlh.capture.paired_cosine


def test_compaction_rejects_bad_arguments_before_touching_the_gpu(lib):
    fake = C.c_void_p(64)                                   # never dereferenced: the checks come first
    ok = dict(z=fake, b=5, t_len=9, d=12, ldb=108, ldt=12, lengths=None, drop_last=0, out=fake, ldo=12, out_rows=45, rows_total=fake)
    for change, what in ((dict(d=0), b"d=0"), (dict(b=65536), b"b=65536"), (dict(ldt=11), b"ldt=11"), (dict(drop_last=-1), b"drop_last=-1"),
                         (dict(out_rows=-1), b"out_rows=-1"), (dict(rows_total=None), b"rows_total"), (dict(b=0), b"b=0"),
                         (dict(t_len=0), b"t_len=0"), (dict(ldo=11), b"ldo=11"), (dict(ldb=50), b"overlap"), (dict(z=None), b"null")):
        args = {**ok, **change}
        assert lib.umlh_seq_compact(*args.values(), None) == E_INVALID, change
        msg = lib.umlh_last_error()
        assert b"umlh_seq_compact" in msg and what in msg, (change, msg)


def test_cosine_rejects_bad_arguments_before_touching_the_gpu(lib):
    fake = C.c_void_p(64)
    need = lib.umlh_paired_cosine_scratch_bytes(100, 20)
    ok = dict(a=fake, lda=20, b=fake, ldb=20, n=100, d=20, eps=1e-8, out2=fake, rows=None, scratch=fake, scratch_bytes=need)
    for change, what in ((dict(n=0), b"n=0"), (dict(lda=19), b"lda=19"), (dict(ldb=19), b"ldb=19"), (dict(eps=-1e-8), b"eps=-1e-08"),
                         (dict(eps=float("nan")), b"eps="), (dict(scratch_bytes=need - 1), b"scratch"), (dict(d=0), b"d=0"),
                         (dict(out2=None), b"null")):
        args = {**ok, **change}
        assert lib.umlh_paired_cosine(*args.values(), None) == E_INVALID, change
        msg = lib.umlh_last_error()
        assert b"umlh_paired_cosine" in msg and what in msg, (change, msg)


def test_cosine_scratch_query(lib):
    q = lib.umlh_paired_cosine_scratch_bytes
    assert q(0, 20) == 0 and q(-1, 20) == 0 and q(100, 0) == 0 and q(100, -3) == 0
    for n in (1, 4, 5, 1000, 50000, 1 << 33):
        assert q(n, 1) > 0 and q(n, 1) == q(n, 300) and q(n, 1) % 256 == 0          # a layout fixed by n alone
    assert q(50000, 40) == q(1 << 33, 40)                                          # the workgroup count is capped


def test_cosine_reference_agrees_with_torch_in_float64():
    g = np.random.default_rng(5)
    for n, d in ((7, 1), (63, 20), (257, 65), (1000, 300)):
        a, b = g.standard_normal((n, d)), g.standard_normal((n, d)) * g.uniform(0.1, 4.0, d)
        a[0] = 0.0                                                                 # a zero row: cos = 0, not NaN
        if n > 1:
            a[1], b[1] = 0.0, 0.0
            a[1, 0], b[1, 0] = 3e-9, 5e-9                                          # both norms under eps: 15e-18 / (1e-8 1e-8)
        want = torch.nn.functional.cosine_similarity(torch.from_numpy(a), torch.from_numpy(b), dim=1)
        rows = R.cosine_rows(a, b)
        assert rows[0] == 0.0
        if n > 1:
            assert abs(rows[1] - 0.15) <= 1e-15                                    # a clamp of the PRODUCT would give 1.5e-9
        assert np.abs(rows - want.numpy()).max() <= 1e-15
        assert abs(R.cosine_mean(a, b) - float(want.mean())) <= 1e-15


def test_compaction_reference():
    z = np.arange(5 * 9 * 2, dtype=np.float32).reshape(5, 9, 2)
    lens = [0, 9, 12, -3, 4]
    assert R.rows_of(lens, 9).tolist() == [0, 9, 9, 0, 4] and R.rows_of(lens, 9, 1).tolist() == [0, 8, 8, 0, 3]
    got = R.compact(z, lens)
    assert got.shape == (22, 2) and got.dtype == np.float32
    assert np.array_equal(got, np.concatenate([z[1], z[2], z[4, :4]]))
    assert np.array_equal(R.compact(z, lens, 1), np.concatenate([z[1, :8], z[2, :8], z[4, :3]]))
    assert np.array_equal(R.compact(z), z.reshape(45, 2)) and R.compact(z, None, 2).shape == (35, 2)


# ---- take_fixed_samples ----
class _Loader:
    """Batches in the reference's layout behind a ``batch_size`` attribute, deep-copied and iterated like a DataLoader."""

    def __init__(self, batches, batch_size):
        self.batches, self.batch_size = batches, batch_size

    def __iter__(self):
        return iter(self.batches)


def _batches(n, bs, seed, T=6, dx=3, dy=4, lens=None):
    g = torch.Generator().manual_seed(seed)
    x, y = torch.randn(n, T, dx, generator=g, dtype=torch.float64), torch.randn(n, T, dy, generator=g)
    lx = torch.randint(1, T + 1, (n,), generator=g) if lens is None else torch.as_tensor(lens)
    ly = lx.flip(0) if lens is None else torch.as_tensor(lens)
    lab = torch.arange(n).reshape(-1, 1) + 1000 * seed
    return [([x[s:s + bs], None, y[s:s + bs]], [lx[s:s + bs], None, ly[s:s + bs]], torch.arange(s, min(s + bs, n)), lab[s:s + bs])
            for s in range(0, n, bs)]


def _same_selection(got, l1, l2, n_samples, bs=None):
    want, labels = R.take_fixed_samples(l1, l2, [0, 2], n_samples, bs)
    for k in ("x1", "x2", "lx1", "lx2"):
        assert len(got[k]) == len(want[k]), k
        for a, b in zip(got[k], want[k]):
            assert a.dtype == b.dtype and torch.equal(a, b), k
    for k in ("x1_label", "x2_label"):
        assert torch.equal(got[k], torch.cat(labels[k], dim=0)), k
    for side in (1, 2):                                                            # host offsets: cumulative clamped lengths
        T = want[f"x{side}"][0].shape[1]
        per_batch = [int(np.clip(l.numpy(), 0, T).sum()) for l in want[f"lx{side}"]]
        assert got[f"off{side}"] == [0] + np.cumsum(per_batch).tolist()
    assert got["rows"] == got["off1"][-1] == got["off2"][-1]


def test_take_fixed_samples_is_the_reference_selection():
    from multibench.capture import take_fixed_samples
    # 7 samples from batches of 3: takes 3, 3, 1
    b = _batches(12, 3, 1, lens=[6, 2, 5, 1, 6, 6, 3, 4, 2, 6, 1, 5])
    got = take_fixed_samples(_Loader(b, 3), _Loader(b, 3), [0, 2], "mosi", n_samples=7)
    assert [t.shape[0] for t in got["x1"]] == [3, 3, 1] and got["x1"][0].dtype == torch.float32
    _same_selection(got, _Loader(b, 3), _Loader(b, 3), 7)
    # n_samples larger than the data, and a short last batch (8 = 3 + 3 + 2)
    b = _batches(8, 3, 2, lens=[4, 4, 6, 1, 3, 6, 2, 5])
    got = take_fixed_samples(_Loader(b, 3), _Loader(b, 3), [0, 2], "humor", n_samples=1000)
    assert [t.shape[0] for t in got["x1"]] == [3, 3, 2]
    _same_selection(got, _Loader(b, 3), _Loader(b, 3), 1000)
    got = take_fixed_samples(_Loader(b, 3), _Loader(b, 3), [0, 2], "humor", n_samples=8)     # the short batch is asked for 2
    assert [t.shape[0] for t in got["x1"]] == [3, 3, 2]
    _same_selection(got, _Loader(b, 3), _Loader(b, 3), 8)
    # loaders of different lengths: the zip ends with the shorter one; list loaders take the first batch's row count
    b1, b2 = _batches(12, 4, 3, lens=[3] * 12), _batches(20, 4, 4, lens=[3] * 20)
    got = take_fixed_samples(b1, b2, [0, 2], "mosei", n_samples=1000)
    assert [t.shape[0] for t in got["x2"]] == [4, 4, 4] and got["rows"] == 36
    _same_selection(got, b1, b2, 1000)
    # random lengths, the y side a permutation of the x side
    b = _batches(10, 5, 5)
    _same_selection(take_fixed_samples(b, b, [0, 2], "mosi", n_samples=10), b, b, 10)
    # lengths outside 0..T are clamped in the offsets
    b = _batches(6, 3, 6, lens=[9, -2, 6, 6, 0, 4])
    got = take_fixed_samples(b, b, [0, 2], "mosi")
    assert got["off1"] == [0, 12, 22]
    # no element 3: no labels
    bare = [(x, l) for x, l, _, _ in _batches(6, 3, 7, lens=[6] * 6)]
    got = take_fixed_samples(bare, bare, [0, 2], "mosi")
    assert got["x1_label"] is None and got["x2_label"] is None and got["rows"] == 36


def test_take_fixed_samples_errors():
    from multibench.capture import take_fixed_samples
    b = _batches(6, 3, 8, lens=[6] * 6)
    with pytest.raises(NotImplementedError):
        take_fixed_samples(b, b, [0, 2], "mimic")
    other = _batches(6, 3, 8, lens=[6, 6, 6, 6, 6, 5])
    with pytest.raises(ValueError, match=r"36 valid rows of modality x and 35 of modality y"):
        take_fixed_samples(b, other, [0, 2], "mosi")
    few = _batches(2, 2, 9, lens=[5, 5])
    with pytest.raises(ValueError, match=r"10 valid rows of modality x and 10 of modality y.*at least 11"):
        take_fixed_samples(few, few, [0, 2], "mosi")
    assert take_fixed_samples(_batches(2, 2, 9, lens=[5, 6]), _batches(2, 2, 9, lens=[6, 5]), [0, 2], "mosi")["rows"] == 11
