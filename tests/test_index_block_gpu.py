"""The row ids of a block of steps written by ONE launch (umlh_index_block / index_block_kernel) instead of epoch shuffles
plus a concatenation: the kernel against the materialised permutation, the loaders' span entries against the index tensors
of a twin loader under the same seed (ids, offsets, RNG state), and the training result against per-step ``train_step`` calls.

Everything here is an integer or a bit comparison: there is no tolerance."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_IMAGENET = 1_281_167
SEEDS = [1, 2 ** 63 + 5]


@functools.lru_cache(maxsize=None)
def _perm(n, seed):
    """The reference of every kernel test: the whole materialised permutation, made once per (n, seed) and never written to."""
    import umlh
    return umlh.random_permutation(n, seed, DEV)


def _span(n, seed, start, count):
    import umlh
    return umlh.IndexSpan(umlh.EpochOrder.permutation(n, seed, DEV), start, count)


def _framed(total, pad=8):
    buf = torch.full((total + 2 * pad,), -1, dtype=torch.int64, device=DEV)
    return buf, buf[pad:pad + total]


def _launch_framed(img_parts, txt_parts):
    """index_block into destinations framed by -1 sentinels; returns the two id vectors after checking the frames."""
    import umlh
    bufs = [None if p is None else _framed(sum(q.numel() for q in p)) for p in (img_parts, txt_parts)]
    umlh.index_block(img_parts, txt_parts, DEV, out=tuple(None if b is None else b[1] for b in bufs))
    torch.cuda.synchronize()
    for b in bufs:
        if b is not None:
            assert bool((b[0][:8] == -1).all()) and bool((b[0][-8:] == -1).all()), "a sentinel next to the destination was overwritten"
    return tuple(None if b is None else b[1] for b in bufs)


# ---- 1. the kernel against the materialised permutation ----
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", [1, 2, 7, 96, 4097, 29940])
def test_spans_equal_slices_of_the_materialised_permutation(n, seed):
    ref = _perm(n, seed)
    k = min(17, n)
    mid = (n - k) // 2
    for start, count in ((0, n), (n - 1, 1), (mid, k)):
        got, _ = _launch_framed([_span(n, seed, start, count)], None)
        assert torch.equal(got, ref[start:start + count]), (n, seed, start, count)


def test_mixed_spans_of_both_modalities_in_one_launch():
    import umlh
    table = torch.randperm(500, generator=torch.Generator().manual_seed(3)).to(DEV)
    tab = umlh.EpochOrder.table(table)
    iota = umlh.EpochOrder.identity(300, DEV)
    img = [_span(29940, 1, 29000, 940), _span(4097, SEEDS[1], 5, 300), umlh.IndexSpan(tab, 100, 257), _span(96, 1, 0, 96),
           umlh.IndexSpan(iota, 290, 10), table[7:40]]
    txt = [umlh.IndexSpan(iota, 0, 300), _span(7, SEEDS[1], 2, 5), umlh.IndexSpan(tab, 0, 500), _span(29940, 1, 0, 513)]
    gi, gt = _launch_framed(img, txt)
    ar = torch.arange(300, device=DEV)
    ri = torch.cat([_perm(29940, 1)[29000:], _perm(4097, SEEDS[1])[5:305], table[100:357], _perm(96, 1), ar[290:], table[7:40]])
    rt = torch.cat([ar, _perm(7, SEEDS[1])[2:7], table, _perm(29940, 1)[:513]])
    assert torch.equal(gi, ri) and torch.equal(gt, rt)


@pytest.mark.parametrize("seed", SEEDS)
def test_imagenet_sized_epoch_first_middle_and_last_partial_batch(seed):
    ref = _perm(N_IMAGENET, seed)
    spans = [(0, 4096), (156 * 4096, 4096), (312 * 4096, 3215)]
    assert 312 * 4096 + 3215 == N_IMAGENET
    gi, gt = _launch_framed([_span(N_IMAGENET, seed, s, c) for s, c in spans[:2]], [_span(N_IMAGENET, seed, *spans[2])])
    assert torch.equal(gi, torch.cat([ref[s:s + c] for s, c in spans[:2]]))
    assert torch.equal(gt, ref[spans[2][0]:])


# ---- loaders: twin sources under the same seed ----
def _table(n, d, C, seed):
    from engine.datasets.utils import FeatureTable
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)
    return FeatureTable(x, torch.randint(0, C, (n,), generator=g), DEV)


@functools.lru_cache(maxsize=None)
def _tables(d, C, n_img=1000, n_txt=100):
    return _table(n_img, d, C, 11), _table(n_txt, d, C, 12)


def _sources(seed, tabs, bs=32, order_rng="device", shuffle=True, precision="fp32", private=False):
    """(image source, text source) whose iterators drew their base seeds from the global generator seeded with ``seed``;
    ``private``: from a generator of the pair's own, so that two pairs can be drawn from in turns."""
    from engine.datasets.utils import FeatureLoader
    from finetune import _RowSource
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed) if private else None
    return tuple(_RowSource(FeatureLoader(t, bs, shuffle=shuffle, kind=kind, order_rng=order_rng, generator=g), torch.device(DEV), kind,
                            precision) for t, kind in zip(tabs, ("image", "text")))


def _twin_steps(img, txt, n):
    """n steps of the per-step path: (image index tensors, text index tensors), image drawn before text."""
    ii, ti = [], []
    for _ in range(n):
        ii.append(img.next_index())
        ti.append(txt.next_index())
    return ii, ti


def _offsets(vs):
    return np.concatenate([[0], np.cumsum([v.numel() for v in vs])]).astype(np.int32)


def _check_block(engine, prep, ii, ti):
    (gi, oi), (gt, ot) = engine.prepared_index(prep)
    torch.cuda.synchronize()
    assert torch.equal(gi, torch.cat(ii)) and torch.equal(gt, torch.cat(ti))
    assert np.array_equal(oi, _offsets(ii)) and np.array_equal(ot, _offsets(ti))


def _small_engine(d=32, C=10, precision="fp32"):
    import umlh
    return umlh.HeadEngine(d, d, C, optimizer="adamw", weight_decay=0.01, max_rows_img=32, max_rows_txt=32, precision=precision,
                           device=DEV)


def _maybe_stream(on):
    torch.cuda.synchronize()                               # (the cached tables were written on the default stream)
    return torch.cuda.stream(torch.cuda.Stream(device=DEV)) if on else torch.cuda.stream(torch.cuda.current_stream(DEV))


# ---- 2. more spans than one launch carries by value ----
def test_seventy_spans_per_modality_take_several_launches():
    import umlh
    from finetune import _draw_block
    tabs = (_table(40, 4, 3, 21), _table(40, 4, 3, 22))
    img, txt = _sources(5, tabs, bs=16)
    bi, bt = _draw_block(img, txt, 105)              # 35 epochs of 3 batches: a span for the first batch, one for the other two
    assert len(bi) == len(bt) == 70
    gi, gt = umlh.index_block([b[0] if isinstance(b, tuple) else b for b in bi], [b[0] if isinstance(b, tuple) else b for b in bt], DEV)
    ii, ti = _twin_steps(*_sources(5, tabs, bs=16), 105)
    assert torch.equal(gi, torch.cat(ii)) and torch.equal(gt, torch.cat(ti))


# ---- 3. loader equivalence (7: once more on a side stream) ----
@pytest.mark.parametrize("side_stream", [False, True], ids=["current", "side-stream"])
@pytest.mark.parametrize("order_rng,shuffle", [("device", True), ("torch-cpu", True), ("device", False)],
                         ids=["device", "torch-cpu", "unshuffled"])
def test_block_vectors_equal_the_twin_loaders_index_tensors(order_rng, shuffle, side_stream):
    from finetune import _draw_block
    tabs = _tables(32, 10)
    e = _small_engine()
    with _maybe_stream(side_stream):
        img, txt = _sources(77, tabs, order_rng=order_rng, shuffle=shuffle)
        preps, states = [], []
        for _ in range(3):
            bi, bt = _draw_block(img, txt, 9)
            preps.append(e.prepare_steps(img.table("fp32"), bi, txt.table("fp32"), bt, [1e-3] * 9))
            states.append(torch.get_rng_state())
        img2, txt2 = _sources(77, tabs, order_rng=order_rng, shuffle=shuffle)
        for prep, state in zip(preps, states):
            ii, ti = _twin_steps(img2, txt2, 9)
            assert torch.equal(torch.get_rng_state(), state)
            _check_block(e, prep, ii, ti)
        torch.cuda.current_stream(DEV).synchronize()


# ---- 4. training equivalence (7: once more on a side stream) ----
@pytest.mark.parametrize("side_stream", [False, True], ids=["current", "side-stream"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_two_blocks_train_like_eighteen_single_steps(precision, side_stream, monkeypatch):
    """Bit equality with ``train_step`` holds where both run the same kernels.  At 32 + 32 rows ``umlh_train_steps`` would
    take the persistent micro-step kernel, whose sums are ordered differently from the per-step kernels' whatever the ids come
    from (measured at this shape, index tensors or spans alike: max |dw| 1.3e-7 bf16, 3.0e-8 fp32), so the engines are made
    with UMLH_MICRO=0: the general path, the one the 4096-row flagship shape takes.  The micro path is held to the index-tensor
    block path by ``test_micro_path_blocks_equal_the_index_tensor_blocks``."""
    import umlh
    from finetune import _draw_block
    monkeypatch.setenv("UMLH_MICRO", "0")
    d, C, steps = 128, 100, 18
    tabs = _tables(d, C)
    w0 = torch.nn.functional.normalize(torch.randn(C, d, generator=torch.Generator().manual_seed(4)), dim=1).to(DEV)
    lrs = [1e-3 * (k + 1) / steps for k in range(steps)]

    def engine():
        e = _small_engine(d, C, precision)
        e.w_head.copy_(w0)
        e.scales.fill_(20.0)
        return e, torch.zeros(steps, umlh.N_SCALARS, device=DEV)

    with _maybe_stream(side_stream):
        ea, sa = engine()
        img, txt = _sources(31, tabs, precision=precision)
        for k0 in (0, 9):
            bi, bt = _draw_block(img, txt, 9)
            prep = ea.prepare_steps(img.table(precision), bi, txt.table(precision), bt, lrs[k0:k0 + 9])
            ea.train_steps_prepared(prep, first_step=k0 + 1, scalars_out=sa[k0:k0 + 9])
        eb, sb = engine()
        img2, txt2 = _sources(31, tabs, precision=precision)
        ti_, tt_ = img2.table(precision), txt2.table(precision)
        f16 = lambda t: t[2] if len(t) > 2 else None
        for k in range(steps):
            ii, ti = img2.next_index(), txt2.next_index()
            eb.train_step(umlh.RowBatch(ti_[0], ti_[1], ii, feats_bf16=f16(ti_)), umlh.RowBatch(tt_[0], tt_[1], ti, feats_bf16=f16(tt_)),
                          lr=lrs[k], step=k + 1, scalars_out=sb[k])
        torch.cuda.current_stream(DEV).synchronize()
    torch.cuda.synchronize()
    ea.check_status()
    assert ea.micro_launches() == 0
    for name, a, b in (("w_head", ea.w_head, eb.w_head), ("m_head", ea.m_head, eb.m_head), ("v_head", ea.v_head, eb.v_head),
                       ("scalars", sa, sb)):
        diff = (a.double() - b.double()).abs().max().item()
        print(f"{precision} {name}: max |block path - step path| = {diff:.3e}")
        assert torch.equal(a, b), (name, diff)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_micro_path_blocks_equal_the_index_tensor_blocks(precision):
    """The same two blocks where ``umlh_train_steps`` takes the micro-step kernel: span entries against the twin loader's index
    tensors handed to ``train_steps``, bit for bit."""
    import umlh
    from finetune import _draw_block
    d, C, steps = 128, 100, 18
    tabs = _tables(d, C)
    w0 = torch.nn.functional.normalize(torch.randn(C, d, generator=torch.Generator().manual_seed(4)), dim=1).to(DEV)
    lrs = [1e-3 * (k + 1) / steps for k in range(steps)]
    runs = []
    for spans in (True, False):
        e = _small_engine(d, C, precision)
        e.w_head.copy_(w0)
        e.scales.fill_(20.0)
        sc = torch.zeros(steps, umlh.N_SCALARS, device=DEV)
        img, txt = _sources(31, tabs, precision=precision)
        for k0 in (0, 9):
            bi, bt = _draw_block(img, txt, 9) if spans else _twin_steps(img, txt, 9)
            e.train_steps(img.table(precision), bi, txt.table(precision), bt, lrs[k0:k0 + 9], first_step=k0 + 1, scalars_out=sc[k0:k0 + 9])
        torch.cuda.synchronize()
        e.check_status()
        runs.append((e, sc))
    (ea, sa), (eb, sb) = runs
    assert ea.micro_launches() == eb.micro_launches()
    for name, a, b in (("w_head", ea.w_head, eb.w_head), ("m_head", ea.m_head, eb.m_head), ("v_head", ea.v_head, eb.v_head),
                       ("scalars", sa, sb)):
        assert torch.equal(a, b), name


# ---- 5. many prepared blocks, dropped blocks, a long block ----
def test_dropped_blocks_blocks_in_order_and_a_long_block():
    import umlh
    from finetune import _draw_block
    tabs = _tables(32, 10)
    e = _small_engine()
    img, txt = _sources(9, tabs, private=True)
    img2, txt2 = _sources(9, tabs, private=True)
    sc = torch.zeros(64, umlh.N_SCALARS, device=DEV)
    step = 1

    def prepare(n):
        bi, bt = _draw_block(img, txt, n)
        prep = e.prepare_steps(img.table("fp32"), bi, txt.table("fp32"), bt, [1e-3] * n)
        return prep

    def consume(prep, n):
        nonlocal step
        e.train_steps_prepared(prep, first_step=step, scalars_out=sc[:n])
        step += n

    preps = [prepare(9) for _ in range(6)]                 # five of them are dropped unconsumed
    twins = [_twin_steps(img2, txt2, 9) for _ in range(6)]
    consume(preps[5], 9)
    _check_block(e, preps[5], *twins[5])
    del preps
    ahead = prepare(9)
    for _ in range(8):                                     # the look-ahead order of the training loops: prepare N+1 behind N
        cur, ahead = ahead, prepare(9)
        consume(cur, 9)
        _check_block(e, cur, *_twin_steps(img2, txt2, 9))
    consume(ahead, 9)
    _check_block(e, ahead, *_twin_steps(img2, txt2, 9))
    long_block = prepare(40)                               # longer than the blocks of the training loops
    consume(long_block, 40)
    _check_block(e, long_block, *_twin_steps(img2, txt2, 40))
    preps = [prepare(9) for _ in range(4)]                 # several blocks held at once, consumed oldest first
    twins = [_twin_steps(img2, txt2, 9) for _ in range(4)]
    for prep, twin in zip(preps, twins):
        consume(prep, 9)
        _check_block(e, prep, *twin)
    e.check_status()
    assert bool(torch.isfinite(sc[:40, :4]).all())


# ---- 6. rewind ----
def test_redraw_after_a_rewind_gives_the_same_ids():
    from finetune import _draw_block, _rewind, _rewind_point
    tabs = _tables(32, 10)
    e = _small_engine()
    img, txt = _sources(13, tabs)
    opt = types.SimpleNamespace(state={}, step_count=0)
    sch = types.SimpleNamespace(last_epoch=0)
    sch.step = lambda epoch: setattr(sch, "last_epoch", epoch)

    def block(n):
        bi, bt = _draw_block(img, txt, n)
        prep = e.prepare_steps(img.table("fp32"), bi, txt.table("fp32"), bt, [1e-3] * n)
        (gi, oi), (gt, ot) = e.prepared_index(prep)
        torch.cuda.synchronize()
        return gi.clone(), gt.clone(), oi.copy(), ot.copy(), torch.get_rng_state()

    block(5)                                               # both loaders stand inside an epoch
    back = _rewind_point(img, txt, opt, sch)
    first = block(9)                                       # crosses the text epoch's end (100 rows, batches of 32)
    _rewind(back, opt, sch)
    again = block(9)
    for a, b in zip(first, again):
        assert torch.equal(a, b) if torch.is_tensor(a) else np.array_equal(a, b)
