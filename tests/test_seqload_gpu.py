"""GPU: the affect datasets' device loader.  Each kernel of umlh_kernels_seqload.hip through ctypes against the float64 statement of
tests/_seqload_ref.py, the loader (multibench/data.py) against every batch the reference's own loader recorded in
tests/golden/seq_loader*.npz, and the consumers (``train``, ``evaluate_raw_data``, ``take_fixed_samples``) fed by device loaders
against the same batches as host lists.

Bounds.  ``start``, lengths, inds, labels and every block without normalisation: equal, bit for bit.  With ``vision_norm`` or
``z_norm``: max |got - ref64| / max |ref64| per block at most ``_seqload_ref.bound(case)``, 8 times the reference's own fp32 error
on that case rounded up to a power of two (2^-18, 2^-15, 2^-18, 2^-19; measured and pinned in tests/test_seqload_cpu.py).  Constant
columns and length-1 sequences under ``z_norm``: exactly 0.  Outputs of the direct kernel calls sit in NaN-sentinel buffers one row
longer than needed: everything inside is written, padding is +0.0, nothing behind is touched.  Every measured figure is printed
before it is asserted."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import _seqload_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


@pytest.fixture(scope="module")
def lib():
    import umlh
    return umlh.load_library()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _check(rc, lib):
    assert rc == 0, lib.umlh_last_error()


def _config(fx, case):
    ds, data_type, zn, vn, bs = fx[f"case/{case}/config"]
    return str(ds), str(data_type), bool(int(zn)), bool(int(vn)), int(bs)


_STATEMENTS = {}


def _statement(fx, case, split):
    """The float64 table of one case and split, computed once per module."""
    ds, data_type, zn, vn, _ = _config(fx, case)
    key = (ds, data_type, zn, vn, split)
    if key not in _STATEMENTS:
        _STATEMENTS[key] = R.build_table(R.fixture_split(fx, ds, split), data_type, zn, vn)
    return _STATEMENTS[key]


def _kept_fp32(fx, ds, split):
    """The kept samples of a split as the upload makes them: fp32, audio -inf -> 0."""
    t = R.build_table(R.fixture_split(fx, ds, split))
    return [a.astype(np.float32) for a in t["tables"]], t["start"][0]


# ---- the kernels through ctypes ----
@pytest.mark.parametrize("ds", ["toy_a", "toy_b", "wide_a", "wide_b"])
def test_first_nonzero_is_exact(fx, lib, ds):
    for split in ("train", "valid"):
        text = R.fixture_split(fx, ds, split)["text"].astype(np.float32)
        n, T, d = text.shape
        x = _dev(text)
        start = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device=DEV)
        _check(lib.umlh_seq_first_nonzero(x.data_ptr(), n, T, d, start.data_ptr(), _stream()), lib)
        got = start.cpu().numpy()
        want = R.first_rows(text)
        print(f"{ds}/{split}: start {got[:n].tolist()}")
        assert np.array_equal(got[:n], want) and got[n] == SENTINEL
        if split == "train":
            assert (want == T).sum() == 1 and (want == 0).any() and (want == T - 1).any()


def _raw_table(tables32, start, T):
    s = np.asarray(start, dtype=np.int64)
    return {"tables": [a.astype(np.float64) for a in tables32], "start": [s, s, s], "lengths": [T - s] * 3,
            "labels": np.zeros((len(s), 1), dtype=np.float32), "T": T}


def _gather(lib, tables, start, ids, t_out, n_src=3):
    """umlh_seq_gather_pad into NaN / SENTINEL buffers one row (one entry) longer than the batch: (out buffers, lengths buffer)."""
    b = len(ids)
    given = [t for t in tables if t is not None]
    n, T = given[0].shape[:2]
    outs = [None if t is None else torch.full((b * t_out * t.shape[2] + t.shape[2],), float("nan"), dtype=torch.float32, device=DEV)
            for t in tables]
    lengths = torch.full((b + 1,), SENTINEL, dtype=torch.int64, device=DEV)
    srcs = (C.c_void_p * n_src)(*[None if t is None else t.data_ptr() for t in tables[:n_src]])
    dsts = (C.c_void_p * n_src)(*[None if o is None else o.data_ptr() for o in outs[:n_src]])
    dims = (C.c_int32 * n_src)(*[-1 if t is None else t.shape[2] for t in tables[:n_src]])
    _check(lib.umlh_seq_gather_pad(srcs, dims, n_src, n, T, start.data_ptr(), ids.data_ptr(), b, t_out, dsts, lengths.data_ptr(),
                                   _stream()), lib)
    return outs, lengths


def _check_gather(what, outs, lengths, want, b, t_out):
    """Blocks bit for bit, padding +0.0, lengths equal, nothing behind the batch touched."""
    blocks, lens, _, _ = want
    got_len = lengths.cpu().numpy()
    assert np.array_equal(got_len[:b], lens[0]) and got_len[b] == SENTINEL, (what, got_len, lens[0])
    for m, o in enumerate(outs):
        if o is None:
            continue
        d = blocks[m].shape[2]
        flat = o.cpu().numpy()
        inside, behind = flat[:b * t_out * d].reshape(b, t_out, d), flat[b * t_out * d:]
        assert R.same_bits(inside, blocks[m]), (what, m)
        pad = np.arange(t_out)[None, :, None] >= lens[m][:, None, None]
        assert not (np.signbit(inside) & pad).any() and (inside[np.broadcast_to(pad, inside.shape)] == 0).all(), (what, m, "padding")
        assert np.isnan(behind).all() and behind.size == d, (what, m, "written behind the batch")


@pytest.mark.parametrize("ds", ["toy_b", "wide_b"])
def test_gather_pad_cases(fx, lib, ds):
    tables32, start = _kept_fp32(fx, ds, "train")
    n, T = tables32[0].shape[:2]
    tab = _raw_table(tables32, start, T)
    dev_tables = [_dev(a) for a in tables32]
    dev_start = _dev(start, np.int32)
    by_len = np.argsort(T - start)                                          # kept samples, shortest first
    short = [int(i) for i in by_len[:3]]
    assert T - start[short[-1]] < T
    cases = {
        "B = 1": ([5], None),
        "Lmax < T": (short, None),
        "a whole batch in order": (list(range(n)), None),
        "t_out below a length": ([int(by_len[-1]), short[0], 7], 3),
        "t_out beyond T": ([3, 4], T + 2),
        "ids -1 and N": ([2, -1, n, 9, -(1 << 40), 1 << 40], None),
        "repeated ids": ([6, 6, 1, 6, 1], None),
    }
    for what, (ids, t_out) in cases.items():
        if t_out is None:
            t_out = int(max(T - start[i] for i in ids if 0 <= i < n))
        want = R.batch(tab, ids, t_out=t_out)
        outs, lengths = _gather(lib, dev_tables, dev_start, _dev(ids, np.int64), t_out)
        print(f"{ds}: {what}: ids {ids} t_out {t_out} lengths {lengths[:-1].tolist()}")
        _check_gather(what, outs, lengths, want, len(ids), t_out)
    # a NULL middle source (its dims entry is garbage and its destination NULL), and two sources only
    ids, t_out = [0, 3, 8], T
    want = R.batch(tab, ids, t_out=t_out)
    outs, lengths = _gather(lib, [dev_tables[0], None, dev_tables[2]], dev_start, _dev(ids, np.int64), t_out)
    assert outs[1] is None
    _check_gather("NULL middle source", outs, lengths, want, 3, t_out)
    outs, lengths = _gather(lib, dev_tables, dev_start, _dev(ids, np.int64), t_out, n_src=2)
    _check_gather("n_src = 2", outs[:2], lengths, want, 3, t_out)
    assert np.isnan(outs[2].cpu().numpy()).all()
    # only length-1 sequences: every start at T - 1
    last = np.full(n, T - 1)
    ids = [4, 0, 11, 4]
    outs, lengths = _gather(lib, dev_tables, _dev(last, np.int32), _dev(ids, np.int64), 1)
    _check_gather("length-1 sequences", outs, lengths, R.batch(_raw_table(tables32, last, T), ids, t_out=1), 4, 1)
    # a start outside 0..T is clamped, never an address
    wild = start.copy()
    wild[0], wild[1] = -5, T + 9
    outs, lengths = _gather(lib, dev_tables, _dev(wild, np.int32), _dev([0, 1, 2], np.int64), T)
    _check_gather("clamped starts", outs, lengths, R.batch(_raw_table(tables32, np.clip(wild, 0, T), T), [0, 1, 2], t_out=T), 3, T)


def test_gather_pad_is_bitwise_reproducible_across_calls_and_streams(fx, lib):
    tables32, start = _kept_fp32(fx, "wide_a", "train")                     # with its NaN
    T = tables32[0].shape[1]
    dev_tables, dev_start = [_dev(a) for a in tables32], _dev(start, np.int32)
    ids = _dev([3, 4, 0, 21, 4, 9, 1], np.int64)
    runs = [_gather(lib, dev_tables, dev_start, ids, T), _gather(lib, dev_tables, dev_start, ids, T)]
    torch.cuda.synchronize()
    for _ in range(2):
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            runs.append(_gather(lib, dev_tables, dev_start, ids, T))
        s.synchronize()
    first = [o.cpu().numpy().view(np.uint32) for o in runs[0][0]] + [runs[0][1].cpu().numpy()]
    for outs, lengths in runs[1:]:
        again = [o.cpu().numpy().view(np.uint32) for o in outs] + [lengths.cpu().numpy()]
        assert all(np.array_equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("case", ["toy_sarcasm_vnorm", "wide_sarcasm_vnorm"])
def test_column_standardize_against_float64(fx, lib, case):
    ds = _config(fx, case)[0]
    for split in ("train", "valid"):
        tables32, _ = _kept_fp32(fx, ds, split)
        want = _statement(fx, case, split)["tables"][0]
        v = tables32[0]
        n, T, d = v.shape
        rows = n * T
        x = _dev(v)
        out = torch.full((rows * d + d,), float("nan"), dtype=torch.float32, device=DEV)
        stats = torch.full((2 * d + 1,), float("nan"), dtype=torch.float64, device=DEV)
        need = lib.umlh_seq_column_standardize_scratch(rows, d)
        scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
        call = lambda dst: _check(lib.umlh_seq_column_standardize(x.data_ptr(), rows, d, d, dst, d, stats.data_ptr(), scratch.data_ptr(),
                                                                  need, _stream()), lib)
        call(out.data_ptr())
        got, st = out.cpu().numpy(), stats.cpu().numpy()
        r64 = v.reshape(rows, d).astype(np.float64)
        e_stats = max(np.abs(st[:d] - r64.mean(0)).max() / np.abs(r64.mean(0)).max(), np.abs(st[d:2 * d] - r64.std(0)).max() / r64.std(0).max())
        err = R.rel_err(got[:rows * d].reshape(n, T, d), want)
        print(f"{case}/{split}: statistics {e_stats:.2e}, table 2^{np.log2(max(err, 1e-30)):.1f} (bound 2^{R.BOUND_LOG2[case]})")
        assert e_stats < 1e-13 and np.isnan(st[2 * d]) and np.isnan(got[rows * d:]).all()
        assert err <= R.bound(case)
        call(x.data_ptr())                                                    # in place: the same bits
        assert np.array_equal(x.cpu().numpy().reshape(-1).view(np.uint32), got[:rows * d].view(np.uint32))


@pytest.mark.parametrize("case", ["toy_mosei_znorm", "wide_mosei_znorm"])
def test_sequence_standardize_against_float64(fx, lib, case):
    ds = _config(fx, case)[0]
    tables32, start = _kept_fp32(fx, ds, "train")
    want = _statement(fx, case, "train")["tables"]
    n, T = tables32[0].shape[:2]
    dev_start = _dev(start, np.int32)
    zeros = 0
    for m, v in enumerate(tables32):
        d = v.shape[2]
        buf = torch.full((n * T * d + d,), float("nan"), dtype=torch.float32, device=DEV)
        buf[:n * T * d] = _dev(v).reshape(-1)
        _check(lib.umlh_seq_standardize(buf.data_ptr(), n, T, d, dev_start.data_ptr(), _stream()), lib)
        flat = buf.cpu().numpy()
        got = flat[:n * T * d].reshape(n, T, d)
        assert np.isnan(flat[n * T * d:]).all()
        kept = np.arange(T)[None, :, None] >= start[:, None, None]
        worst = R.rel_err(np.where(kept, got, 0.0), np.where(kept, want[m], 0.0))        # the table as one block
        per_sample = max(R.rel_err(got[i, start[i]:], want[m][i, start[i]:]) for i in range(n))
        print(f"{case}: modality {m}: worst single sequence against its own largest magnitude 2^{np.log2(max(per_sample, 1e-30)):.1f}")
        for i in range(n):
            s = start[i]
            assert R.same_bits(got[i, :s], v[i, :s]), (m, i, "rows in front of start were touched")
            const = (v[i, s:] == v[i, s]).all(0)                            # constant columns; every column of a length-1 sequence
            assert (got[i, s:][:, const] == 0).all() and not np.signbit(got[i, s:][:, const]).any(), (m, i)
            zeros += int(const.sum())
            # launch geometry: the sample alone in a table of one gives the same bits
            if i in (0, 1, 5, n - 1):
                one = _dev(v[i:i + 1])
                _check(lib.umlh_seq_standardize(one.data_ptr(), 1, T, d, dev_start[i:i + 1].data_ptr(), _stream()), lib)
                assert R.same_bits(one.cpu().numpy()[0], got[i]), (m, i, "depends on n or on the sample's position")
        print(f"{case}: modality {m}: 2^{np.log2(max(worst, 1e-30)):.1f} (bound 2^{R.BOUND_LOG2[case]})")
        assert worst <= R.bound(case)
    assert (T - start == 1).any() and zeros >= 3 + sum(v.shape[2] for v in tables32)


# ---- through the loader ----
def _loaders(fx, case, modalities=(0, 1, 2)):
    from multibench.data import AffectTable, SequenceLoader
    ds, data_type, zn, vn, bs = _config(fx, case)
    tables = {s: AffectTable(R.fixture_split(fx, ds, s), data_type=data_type, z_norm=zn, vision_norm=vn, device=DEV) for s in ("train", "valid")}
    train = SequenceLoader(tables["train"], bs, shuffle=True, generator=torch.Generator().manual_seed(42), modalities=modalities)
    return train, SequenceLoader(tables["valid"], bs, modalities=modalities), tables


@pytest.mark.parametrize("case", list(R.BOUND_LOG2))
def test_loader_gives_the_batches_of_the_reference(fx, case):
    train, valid, tables = _loaders(fx, case)
    assert len(tables["train"]) == 22 and len(tables["valid"]) == 9 and train.batch_size == _config(fx, case)[4]
    worst = 0.0
    for loader, it, split in (("train0", train, "train"), ("train1", train, "train"), ("valid", valid, "valid")):
        ref = R.fixture_batches(fx, case, loader)
        st = _statement(fx, case, split)
        got = list(it)
        assert len(got) == len(ref) == len(it)
        for batch, (xs, ls, inds, labels) in zip(got, ref):
            assert isinstance(batch, tuple) and len(batch) == 4 and isinstance(batch[0], list) and isinstance(batch[1], list)
            assert len(batch[0]) == len(batch[1]) == 3
            want = R.batch(st, inds.reshape(-1))
            for m in range(3):
                x, l = batch[0][m], batch[1][m]
                assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == xs[m].shape
                assert l.is_cuda and l.dtype == torch.int64 and tuple(l.shape) == ls[m].shape and np.array_equal(l.cpu().numpy(), ls[m])
                if R.BOUND_LOG2[case] is None:
                    assert R.same_bits(x.cpu().numpy(), xs[m]) and R.same_bits(x.cpu().numpy(), want[0][m])
                else:
                    worst = max(worst, R.rel_err(x.cpu().numpy(), want[0][m]))
            assert not batch[2].is_cuda and batch[2].dtype == torch.int64 and np.array_equal(batch[2].numpy(), inds)
            assert not batch[3].is_cuda and batch[3].dtype == torch.float32 and batch[3].shape == (len(inds), 1)
            assert R.same_bits(batch[3].numpy(), labels)
    if R.BOUND_LOG2[case] is not None:
        print(f"{case}: worst block 2^{np.log2(max(worst, 1e-30)):.1f} (bound 2^{R.BOUND_LOG2[case]})")
        assert worst <= R.bound(case)


def test_loader_skips_unrequested_modalities_and_deep_copies_replay(fx):
    train, _, _ = _loaders(fx, "toy_mosi", modalities=(0, 2))
    full, _, _ = _loaders(fx, "toy_mosi")
    state = train.generator.get_state().clone()
    twin = copy.deepcopy(train)
    assert twin.table is train.table
    replay = list(twin)
    assert torch.equal(train.generator.get_state(), state)                 # the copy drew from its own generator
    assert [b for b in copy.deepcopy(train).iter_index()] == [b[2].reshape(-1).tolist() for b in replay]
    for a, b, c in zip(list(train), replay, list(full)):
        assert a[0][1] is None and a[1][1] is None and b[0][1] is None
        for m in (0, 2):
            assert torch.equal(a[0][m].view(torch.int32), b[0][m].view(torch.int32)) and torch.equal(a[1][m], c[1][m])
            assert torch.equal(a[0][m].view(torch.int32), c[0][m].view(torch.int32))
        assert torch.equal(a[2], c[2]) and torch.equal(a[3], c[3])


def test_get_dataloader_and_dropped_samples(fx):
    from multibench.data import get_dataloader
    data = {s: R.fixture_split(fx, "toy_a", "train" if s == "train" else "valid") for s in ("train", "valid", "test")}
    train, valid, test = get_dataloader(data, batch_size=4, data_type="sarcasm", vision_norm=True, device=DEV)
    assert (len(train), len(valid), len(test)) == (6, 3, 3) and train.sampler.shuffle and not valid.sampler.shuffle
    assert train.table.kept.tolist() == [i for i in range(23) if i != 2] and train.table.ids.reshape(-1).tolist() == [100 + i for i in range(23) if i != 2]
    got = [b[2].reshape(-1).tolist() for b in train]
    assert got == [inds.reshape(-1).tolist() for _, _, inds, _ in R.fixture_batches(fx, "toy_sarcasm_vnorm", "train0")]
    assert set(torch.cat([b[3] for b in valid]).reshape(-1).tolist()) <= {-1.0, 1.0}


# ---- through the consumers ----
class _ListLoader(list):
    batch_size = 4


def _host(batch):
    cpu = lambda t: None if t is None else t.cpu()
    return [cpu(x) for x in batch[0]], [cpu(l) for l in batch[1]], batch[2], batch[3]


def _model(dx, dy, z=20):
    from multibench.models import Linear, Transformer, UML
    torch.manual_seed(3)
    return UML(Linear(dx, z), Linear(dy, z), Transformer(z, z, nhead=5, num_layers=2, conv1d=True, out_last=False, pos_embd=True,
                                                       pos_learnable=False, max_len=128), [Linear(z, dx), Linear(z, dy)], modality="xy")


def test_train_fed_by_device_loaders_equals_the_host_list(fx):
    from multibench.data import SequenceLoader
    from multibench.train import train
    _, _, tables = _loaders(fx, "toy_mosei_znorm")
    mk = lambda: SequenceLoader(tables["train"], 4, shuffle=True, generator=torch.Generator().manual_seed(42), modalities=(0, 2))
    dev_1, dev_2 = mk(), mk()
    host_1, host_2 = (_ListLoader(_host(b) for b in copy.deepcopy(l)) for l in (dev_1, dev_2))
    master = _model(tables["train"].dims[0], tables["train"].dims[2])
    results = []
    for l1, l2 in ((dev_1, dev_2), (host_1, host_2)):
        model = copy.deepcopy(master).to(DEV)
        torch.manual_seed(11)                                               # the seed of the encoder's dropout masks
        results.append(train(model, "xy", l1, l2, torch.optim.Adam(model.parameters(), lr=1e-3), num_epoch=1, step_k=-1,
                             ds_name="mosei", device=DEV))
    dev_res, host_res = results
    print("loss", dev_res["loss"])
    assert len(dev_res["loss"]) == 6 and all(np.isfinite(v) for v in dev_res["loss"])
    for k in ("loss_x", "loss_y", "loss"):
        assert dev_res[k] == host_res[k], k


def test_evaluate_raw_data_and_fixed_samples_take_device_batches(fx):
    from multibench.capture import take_fixed_samples
    from multibench.data import SequenceLoader
    from multibench.train import evaluate_raw_data
    _, valid, tables = _loaders(fx, "toy_mosei_znorm")
    ordered = SequenceLoader(tables["train"], 4)
    cfg = {"train": list(ordered), "val": list(valid), "test": list(valid)}
    host_cfg = {k: [_host(b) for b in v] for k, v in cfg.items()}
    got, want = evaluate_raw_data(cfg, "mosei", device=DEV), evaluate_raw_data(host_cfg, "mosei", device=DEV)
    print(got)
    assert got == want and all(np.isfinite(v) for v in got.values())
    mk = lambda: SequenceLoader(tables["train"], 4, shuffle=True, generator=torch.Generator().manual_seed(42))
    dev_1, dev_2 = mk(), mk()
    host_1, host_2 = (_ListLoader(_host(b) for b in copy.deepcopy(l)) for l in (dev_1, dev_2))
    state = dev_1.generator.get_state().clone()
    a, b = take_fixed_samples(dev_1, dev_2, [0, 2], "mosei", n_samples=14), take_fixed_samples(host_1, host_2, [0, 2], "mosei", n_samples=14)
    assert torch.equal(dev_1.generator.get_state(), state)                  # the sample is taken from copies of the loaders
    assert a["rows"] == b["rows"] and a["off1"] == b["off1"] and a["off2"] == b["off2"] and len(a["x1"]) == len(b["x1"]) == 4
    for k in ("x1", "x2", "lx1", "lx2"):
        for u, v in zip(a[k], b[k]):
            assert u.shape == v.shape and torch.equal(u.cpu(), v)
    for k in ("x1_label", "x2_label"):
        assert torch.equal(a[k], b[k])
