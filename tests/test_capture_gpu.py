"""GPU: the embedding capture.  umlh.seq_compact against the numpy compaction bit for bit (int32 views; the data carry NaN
payloads and -0.0), umlh.paired_cosine against float64, multibench.capture.EmbeddingCapture against the test's own eval
forward and the metric calls it stands for, and multibench.train.train(capture_embeddings_during_training=True) end to end.

Bounds.  The cosine mean: |mean - float64| <= 1e-12.  An fp64 evaluation of a d-term dot product rounds by about d 2^-53
(3e-14 at d = 300) and the mean of n such values no worse; the reference's own fp32 form is off by 4e-9 .. 3e-8 at
997 x 20 .. 50 000 x 40 (measured on a CPU).  The per-row output: within 1 ulp of fp32 of the float64 row value (one rounding of
an fp64 value that is itself good to 1e-13).  Every measured figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import _capture_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7FC0DEAD                      # a NaN no computation produces: "nobody wrote here"
BASE_LENS = [0, 9, 12, -3, 4]


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _block(shape, seed):
    """fp32 data with -0.0, quiet and signalling NaNs of distinct payloads and an Inf sprinkled in."""
    g = np.random.default_rng(seed)
    a = g.standard_normal(shape).astype(np.float32)
    flat = a.reshape(-1).view(np.int32)
    idx = g.permutation(flat.size)
    for j, word in enumerate((-0x80000000, 0x7FC00123, -0x3FABCD, 0x7F800001, 0x7F800000)):     # -0.0, qNaN, -qNaN, sNaN, +Inf
        flat[idx[j::5][: max(1, flat.size // 40)]] = word
    return a


def _compact_check(z_dev, z_host, lens, drop_last, ldo=None, short=0):
    """Packs into a sentinel buffer one row longer than needed -> everything due is there bit for bit, nothing else is touched."""
    import umlh
    B, T, d = z_host.shape
    want = R.compact(z_host, lens, drop_last)
    n = want.shape[0]
    assert n > short
    ldo = d if ldo is None else ldo
    buf = torch.full((n + 1, ldo), SENTINEL, dtype=torch.int32, device=DEV)
    out = buf.view(torch.float32)[: n - short, :d]
    l_dev = None if lens is None else torch.tensor(lens, device=DEV)
    got, total = umlh.seq_compact(z_dev, l_dev, drop_last, out=out)
    assert got is out and total.dtype == torch.int64 and total.shape == () and total.device.type == "cuda"
    assert int(total) == n                                                   # the true count, also when out is short
    b = buf.cpu().numpy()
    assert np.array_equal(b[: n - short, :d], want.view(np.int32)[: n - short])
    assert (b[n - short:] == SENTINEL).all() and (b[:, d:] == SENTINEL).all()
    return want


@pytest.mark.parametrize("drop_last", [0, 1])
def test_compact_base_case(drop_last):
    import umlh
    z = _block((5, 9, 12), 1)
    zd = torch.from_numpy(z).to(DEV)
    want = _compact_check(zd, z, BASE_LENS, drop_last)
    assert want.shape[0] == (22 if drop_last == 0 else 19)
    lens = torch.tensor(BASE_LENS, device=DEV)
    for kw in ({"rows": want.shape[0]}, {}):                                 # the count known on the host / read back once
        got, total = umlh.seq_compact(zd, lens, drop_last, **kw)
        assert got.shape == want.shape and int(total) == want.shape[0]
        assert np.array_equal(_bits(got), want.view(np.int32))
    _compact_check(zd, z, BASE_LENS, drop_last, short=2)                     # out_rows two short: the last two rows are not written


@pytest.mark.parametrize("d", [1, 33, 300])
def test_compact_widths(d):
    z = _block((5, 9, d), 10 + d)
    _compact_check(torch.from_numpy(z).to(DEV), z, BASE_LENS, 0)
    _compact_check(torch.from_numpy(z).to(DEV), z, BASE_LENS, 1, ldo=d + 3)


def test_compact_without_lengths():
    import umlh
    z = _block((5, 9, 12), 2)
    zd = torch.from_numpy(z).to(DEV)
    _compact_check(zd, z, None, 0)
    _compact_check(zd, z, None, 1)
    got, total = umlh.seq_compact(zd, drop_last=2)
    assert got.shape == (35, 12) and int(total) == 35 and np.array_equal(_bits(got), R.compact(z, None, 2).view(np.int32))


def test_compact_reads_views_in_place():
    from umlh import spectral
    z = _block((5, 9, 12), 3)
    tb = torch.from_numpy(np.ascontiguousarray(z.transpose(1, 0, 2))).to(DEV)          # a [T, B, d] block
    view = tb.transpose(0, 1)
    assert spectral._in_place(view, torch.device(DEV)).data_ptr() == tb.data_ptr()     # no copy on the way to the kernel
    _compact_check(view, z, BASE_LENS, 0)
    for width, first in ((19, 3), (20, 4)):                                  # a column block: 4-byte and 16-byte accesses
        wide = _block((5, 9, width), 4)
        col = torch.from_numpy(wide).to(DEV)[:, :, first:first + 12]
        assert spectral._in_place(col, torch.device(DEV)).data_ptr() == col.data_ptr()
        _compact_check(col, np.ascontiguousarray(wide[:, :, first:first + 12]), BASE_LENS, 1)
    _compact_check(torch.from_numpy(z).to(DEV), z, BASE_LENS, 0, ldo=16)     # ldo > d, 16-byte accesses
    _compact_check(torch.from_numpy(z).to(DEV), z, BASE_LENS, 0, ldo=15)     # ldo > d, 4-byte accesses


def test_compact_many_sequences_and_row_chunks():
    g = np.random.default_rng(6)
    z = _block((257, 3, 4), 5)                                               # the offset sums span more than one wave
    _compact_check(torch.from_numpy(z).to(DEV), z, g.integers(-1, 5, 257).tolist(), 0)
    z = _block((700, 2, 3), 7)                                               # ... and more than one pass of the workgroup
    _compact_check(torch.from_numpy(z).to(DEV), z, g.integers(0, 3, 700).tolist(), 0)
    z = _block((3, 60, 300), 8)                                              # 27 rows per workgroup at d = 300: three chunks
    _compact_check(torch.from_numpy(z).to(DEV), z, [60, 31, 27], 0)
    _compact_check(torch.from_numpy(z).to(DEV), z, [60, 31, 27], 1, short=2)
    z = _block((2, 3, 8192), 9)                                              # a row per workgroup
    _compact_check(torch.from_numpy(z).to(DEV), z, [3, 2], 0)


# ---- cosine ----
def _cos_inputs(n, d):
    g = np.random.default_rng(100 * n + d)
    a = (g.standard_normal((n, d)) * g.uniform(0.2, 3.0, d)).astype(np.float32)
    b = (0.5 * a + g.standard_normal((n, d))).astype(np.float32)
    if n >= 3:
        a[0] = 0.0                                                           # a zero row: cos = 0
        a[2], b[2] = 0.0, 0.0
        a[2, 0], b[2, 0] = 3e-9, 5e-9                                        # norms 3e-9 and 5e-9: cos = 0.15, each clamped on its own
    return a, b


def _strided(a, pad):
    wide = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), device=DEV)
    wide[:, : a.shape[1]] = torch.from_numpy(a).to(DEV)
    return wide[:, : a.shape[1]]


@pytest.mark.parametrize("d", [1, 20, 64, 65, 300])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_cosine_against_float64(n, d):
    import umlh
    a, b = _cos_inputs(n, d)
    mean, rows = umlh.paired_cosine(_strided(a, 3), _strided(b, 5), return_rows=True)
    assert mean.shape == () and mean.dtype == torch.float64 and rows.shape == (n,) and rows.dtype == torch.float32
    want_rows = R.cosine_rows(a, b)
    want = float(want_rows.mean())
    err = abs(float(mean) - want)
    rows = rows.cpu().numpy()
    ulps = np.abs(rows.astype(np.float64) - want_rows) / np.spacing(np.abs(want_rows).astype(np.float32)).astype(np.float64)
    print(f"cosine {n}x{d}: mean {float(mean):.15f} float64 {want:.15f} err {err:.3e}, rows max {ulps.max():.3f} ulp of fp32")
    assert err <= 1e-12
    assert ulps.max() <= 1.0
    if n >= 3:
        assert rows[0] == 0.0 and abs(want_rows[2] - 0.15) <= 1e-7               # 0.15 up to the fp32 rounding of 3e-9 and 5e-9
    assert torch.equal(umlh.paired_cosine(_strided(a, 3), _strided(b, 5)), mean)


def test_cosine_nan_row_and_reproducibility():
    import umlh
    a, b = _cos_inputs(1000, 300)
    ad, bd = _strided(a, 4), _strided(b, 4)
    m1, r1 = umlh.paired_cosine(ad, bd, return_rows=True)
    m2, r2 = umlh.paired_cosine(ad, bd, return_rows=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m3, r3 = umlh.paired_cosine(ad, bd, return_rows=True)
    side.synchronize()
    assert _bits(m1.reshape(1).view(torch.float32)).tolist() == _bits(m2.reshape(1).view(torch.float32)).tolist() \
        == _bits(m3.reshape(1).view(torch.float32)).tolist()
    assert torch.equal(r1, r2) and torch.equal(r1, r3)
    a[17, 5] = np.nan
    m, r = umlh.paired_cosine(torch.from_numpy(a).to(DEV), bd, return_rows=True)
    r = r.cpu().numpy()
    assert np.isnan(float(m)) and np.isnan(r[17]) and np.isfinite(np.delete(r, 17)).all()


# ---- EmbeddingCapture.measure ----
class _ListLoader(list):
    """A list of batches in the reference's layout; deep-copied and re-iterated like a DataLoader."""


X_LENS = [[9, 3, 5, 1, 6], [2, 9, 9, 4, 7], [5, 5, 8, 1, 2]]
Y_LENS = [[5, 9, 1, 6, 3], [9, 7, 2, 4, 9], [1, 8, 5, 2, 5]]                 # permutations: equal totals, different layout


def _small_model(seed):
    from multibench.models import Linear, Transformer, UML
    torch.manual_seed(seed)
    z, dx, dy = 20, 12, 24
    return UML(Linear(dx, z), Linear(dy, z), Transformer(z, z, nhead=5, num_layers=1, conv1d=True, out_last=False, pos_embd=True,
                                                           pos_learnable=False, max_len=128),
               [Linear(z, dx), Linear(z, dy)], modality="xy").to(DEV)


def _small_loaders():
    g = torch.Generator().manual_seed(99)
    mk = lambda i: [[torch.randn(5, 9, 12, generator=g), None, torch.randn(5, 9, 24, generator=g)],
                    [torch.tensor(X_LENS[i]), None, torch.tensor(Y_LENS[i])]]
    batches = [mk(i) for i in range(3)]
    return _ListLoader(batches), _ListLoader(batches)


def _own_forward(model, pairs):
    """The six packed matrices (numpy fp32) of the test's own eval forward of (x, y, lx, ly) batches."""
    was = model.training
    model.eval()
    parts = {k: [] for k in ("zx", "x_proj", "x_recon", "zy", "y_proj", "y_recon")}
    with torch.no_grad():
        for x, y, lx, ly in pairs:
            out = model(x.float().to(DEV), y.float().to(DEV), lx.to(DEV), ly.to(DEV))
            for k in parts:
                parts[k].append(R.compact(out[k].cpu().numpy(), (lx if k in ("zx", "x_proj", "x_recon") else ly).numpy()))
    torch.nn.Module.train(model, was)
    return {k: np.concatenate(v, axis=0) for k, v in parts.items()}


def _clip(v):
    return max(min(v, 1.0), 0.0)


def test_embedding_capture_measure():
    import umlh
    from multibench.capture import KEYS, EmbeddingCapture, take_fixed_samples
    model = _small_model(0).train()
    l1, l2 = _small_loaders()
    samples = take_fixed_samples(l1, l2, [0, 2], "mosi")
    n = sum(sum(min(max(v, 0), 9) for v in row) for row in X_LENS)
    assert samples["rows"] == n and samples["x1_label"] is None
    cap = EmbeddingCapture(samples, DEV)
    res, zx, zy = cap.measure(model)
    assert model.training and tuple(res) == KEYS and zx.shape == (n, 20) and zy.shape == (n, 20)
    pairs = [(b1[0][0], b2[0][2], b1[1][0], b2[1][2]) for b1, b2 in zip(l1, l2)]
    own = _own_forward(model, pairs)
    assert zx is cap.matrices["zx"] and zy is cap.matrices["zy"]
    for k, want in own.items():
        assert np.array_equal(_bits(cap.matrices[k]), want.view(np.int32)), k
    raw_x = R.compact(np.concatenate([p[0].numpy() for p in pairs]), np.concatenate(X_LENS))
    raw_y = R.compact(np.concatenate([p[1].numpy() for p in pairs]), np.concatenate(Y_LENS))
    assert np.array_equal(_bits(cap.raw_x), raw_x.view(np.int32)) and np.array_equal(_bits(cap.raw_y), raw_y.view(np.int32))
    m = {k: torch.from_numpy(v).to(DEV) for k, v in own.items()}
    ry, rx = torch.from_numpy(raw_y).to(DEV), torch.from_numpy(raw_x).to(DEV)
    cka, mknn, cos = umlh.align.cka, lambda a, b: umlh.align.mutual_knn(a, b, topk=10), umlh.paired_cosine
    want = {"val/cka_proj": _clip(float(cka(m["x_proj"], m["y_proj"]))), "val/mknn_proj": float(mknn(m["x_proj"], m["y_proj"])),
            "val/cos_sim_proj": float(cos(m["x_proj"], m["y_proj"])),
            "val/cka_embed": _clip(float(cka(m["zx"], m["zy"]))), "val/mknn_embed": float(mknn(m["zx"], m["zy"])),
            "val/cos_sim_embed": float(cos(m["zx"], m["zy"])),
            "val/cka_out": _clip(float(cka(m["x_recon"], m["y_recon"]))), "val/mknn_out": float(mknn(m["x_recon"], m["y_recon"])),
            "val/cka_text_embeddings_features": _clip(float(cka(m["zy"], ry))),
            "val/cka_raw": min(max(float(cka(rx, ry)), 0.0), 1.0), "val/mknn_raw": min(max(float(mknn(rx, ry)), 0.0), 1.0)}
    for k in KEYS:
        print(f"capture {k}: {res[k]!r} (direct call {want[k]!r})")
        assert res[k] == want[k] and np.isfinite(res[k]), k
    for k, a, b in (("val/cos_sim_proj", "x_proj", "y_proj"), ("val/cos_sim_embed", "zx", "zy")):
        ref = R.cosine_mean(own[a], own[b])
        print(f"capture {k}: err {abs(res[k] - ref):.3e} against float64")
        assert abs(res[k] - ref) <= 1e-12
    res2, zx2, zy2 = cap.measure(model)                                      # a second capture: same values, fresh zx / zy
    assert res2 == res and zx2 is not zx and torch.equal(zx2, zx) and torch.equal(zy2, zy)


# ---- train end to end ----
def _model(name):
    from multibench.models import Linear, Transformer, UML
    g = load_golden(name)
    z, dx, dy, B, T, pe, pl = (int(v) for v in g["cfg"])
    m = UML(Linear(dx, z), Linear(dy, z), Transformer(z, z, nhead=5, num_layers=5, conv1d=True, out_last=False,
                                                       pos_embd=bool(pe), pos_learnable=bool(pl), max_len=128),
            [Linear(z, dx), Linear(z, dy)], modality="xy")
    m.load_state_dict({k[4:]: torch.as_tensor(g[k]) for k in g.files if k.startswith("sd::")})
    return m.to(DEV)


def _config(g, freq=2):
    bs, cfg = int(g["batch_size"]), {"freq": freq}
    for t in ("train", "val", "test"):
        x, y, lx, ly, lab = (torch.from_numpy(g[f"{k}_{t}"]) for k in ("x", "y", "lx", "ly", "labels"))
        cfg[t] = [([x[s:s + bs], None, y[s:s + bs]], [lx[s:s + bs], None, ly[s:s + bs]], torch.arange(s, min(s + bs, len(x))),
                   lab[s:s + bs].reshape(-1, 1)) for s in range(0, len(x), bs)]
    return cfg


@pytest.fixture(scope="module")
def e2e():
    """The humor golden, an eval_config with freq 2 and a 3-batch loader whose y lengths are the x lengths rolled by one within
    each batch (equal totals of valid rows, different layout); evaluations at i_batch 0 and 2, then the closing one."""
    g = load_golden("probe_e2e_humor")
    x, y, lx, lab = (torch.from_numpy(g[f"{k}_train"]) for k in ("x", "y", "lx", "labels"))
    loader = _ListLoader(([x[s:s + 16], None, y[s:s + 16]], [lx[s:s + 16], None, lx[s:s + 16].roll(1)], torch.arange(s, s + 16),
                          lab[s:s + 16].reshape(-1, 1)) for s in range(0, 48, 16))
    return g, _config(g, freq=2), loader


def _train(e2e, opt_fn, pin=False, **kw):
    from multibench.train import train
    g, cfg, loader = e2e
    torch.manual_seed(0)
    model = _model(str(g["model"]))
    if pin:
        model.eval()
        model.train = lambda *a, **k: model                                  # stay in eval mode (dropout off): runs retrace each other
    res = train(model, "xy", loader, loader, opt_fn(model.parameters()), num_epoch=1, step_k=-1, ds_name="humor", eval_config=cfg,
                device=DEV, **kw)
    return model, res


def test_train_capture_with_a_still_model(e2e):
    from multibench.capture import KEYS
    g, cfg, loader = e2e
    model, res = _train(e2e, lambda p: torch.optim.SGD(p, lr=0.0), capture_embeddings_during_training=True)
    n = int(sum(int(b[1][0].clamp(0, 9).sum()) for b in loader))
    assert [(e, i) for e, i, _ in res["eval"]] == [(0, 0), (0, 2), (0, None)]
    emb = res["embeddings"]
    assert set(emb) == {"x1", "x2", "x1_label", "x2_label"}
    assert emb["x1"].shape == (2, n, 20) and emb["x2"].shape == (2, n, 20) and emb["x1"].dtype == torch.float32 and emb["x1"].is_cuda
    assert torch.equal(emb["x1_label"], torch.from_numpy(g["labels_train"][:48]).reshape(-1, 1)) and torch.equal(emb["x1_label"], emb["x2_label"])
    first, second = res["eval"][0][2], res["eval"][1][2]
    assert set(KEYS) <= set(first) and all(first[k] == second[k] and np.isfinite(first[k]) for k in KEYS)       # lr 0: nothing moved
    assert all(0.0 <= first[k] <= 1.0 for k in KEYS if "cka" in k or "mknn" in k) and all(-1.0 <= first[k] <= 1.0 for k in KEYS)
    own = _own_forward(model, [(b[0][0], b[0][2], b[1][0], b[1][2]) for b in loader])
    for e in range(2):
        assert np.array_equal(_bits(emb["x1"][e]), own["zx"].view(np.int32)) and np.array_equal(_bits(emb["x2"][e]), own["zy"].view(np.int32))
    for k, a, b in (("val/cos_sim_proj", "x_proj", "y_proj"), ("val/cos_sim_embed", "zx", "zy")):
        assert abs(first[k] - R.cosine_mean(own[a], own[b])) <= 1e-12


def test_train_capture_with_a_moving_model(e2e):
    from multibench.capture import KEYS
    from multibench.train import train
    model, res = _train(e2e, lambda p: torch.optim.Adam(p, lr=1e-3), capture_embeddings_during_training=True)
    assert model.training
    emb = res["embeddings"]
    assert not torch.equal(emb["x1"][0], emb["x1"][1]) and not torch.equal(emb["x2"][0], emb["x2"][1])
    assert all(set(KEYS) <= set(r) for _, i, r in res["eval"] if i is not None)
    closing = res["eval"][-1]
    assert closing[1] is None and not set(KEYS) & set(closing[2])                 # as in the reference
    assert set(res) == {"loss_x", "loss_y", "loss", "raw", "eval", "embeddings"}
    g, cfg, loader = e2e
    with pytest.raises(ValueError, match="eval_config"):
        train(model, "xy", loader, loader, None, num_epoch=1, ds_name="humor", device=DEV, capture_embeddings_during_training=True)


def test_train_capture_changes_nothing_else(e2e):
    from multibench.capture import KEYS
    g = e2e[0]
    opt = lambda p: torch.optim.Adam(p, lr=1e-3)
    _, on = _train(e2e, opt, pin=True, capture_embeddings_during_training=True, effective_rank=True)
    _, off = _train(e2e, opt, pin=True, effective_rank=True)
    for k in ("loss_x", "loss_y", "loss", "pred_effective_rank_y"):
        assert on[k] == off[k] and len(on[k]) == 3, k
    assert on["gt_effective_rank_y"] == off["gt_effective_rank_y"]                # one y sample serves both
    assert set(off) == {"loss_x", "loss_y", "loss", "raw", "eval", "pred_effective_rank_y", "gt_effective_rank_y"}
    assert set(on) == set(off) | {"embeddings"}
    logged = {k for k in g["keys_eval"] if "private" not in k and "complete" not in k} | set(g["keys_raw"])
    for (e0, i0, r0), (e1, i1, r1) in zip(off["eval"], on["eval"]):
        assert (e0, i0) == (e1, i1) and set(r0) == logged
        assert set(r1) == (logged | set(KEYS) if i1 is not None else logged)
        assert all(r0[k] == r1[k] or (np.isnan(r0[k]) and np.isnan(r1[k])) for k in logged)
    _, plain = _train(e2e, opt, pin=True)
    assert set(plain) == {"loss_x", "loss_y", "loss", "raw", "eval"} and plain["loss"] == off["loss"]
