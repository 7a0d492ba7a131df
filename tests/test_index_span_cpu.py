"""Span bookkeeping of the blockwise loop without a GPU: what ``_draw_block`` returns for device-order loaders are positions of
epoch orders (``umlh.IndexSpan``), not tensors -- their ``numel()``, batch sizes and offsets, the row count the benchmark forms
from them, the RNG draws, and the argument checks of ``umlh_index_block`` that precede its launch."""
import ctypes as C

import numpy as np
import pytest
import torch


def _sources(seed, order_rng, n_img=1000, n_txt=100, bs=32, shuffle=True):
    from engine.datasets.utils import FeatureLoader, FeatureTable
    from finetune import _RowSource
    torch.manual_seed(seed)
    tabs = [FeatureTable(torch.zeros(n, 4), torch.zeros(n, dtype=torch.long), "cpu") for n in (n_img, n_txt)]
    return tuple(_RowSource(FeatureLoader(t, bs, shuffle=shuffle, kind=kind, order_rng=order_rng), torch.device("cpu"), kind)
                 for t, kind in zip(tabs, ("image", "text")))


def _bench_rows(entries):
    return sum(int(b[0].numel()) if isinstance(b, tuple) else int(b.numel()) for b in entries)      # bench.py's expression


def _sizes(entries):
    out = []
    for b in entries:
        out.extend(b[1] if isinstance(b, tuple) else [b.numel()])
    return out


def test_device_order_blocks_are_spans_with_the_sizes_of_the_tensor_path():
    import umlh
    from finetune import _draw_block
    img, txt = _sources(3, "device")
    img2, txt2 = _sources(3, "torch-cpu")              # the same batch structure, entries backed by CPU tensors
    for n in (9, 9, 25, 1, 40):
        bi, bt = _draw_block(img, txt, n)
        ri, rt = _draw_block(img2, txt2, n)
        for got, ref in ((bi, ri), (bt, rt)):
            heads = [b[0] if isinstance(b, tuple) else b for b in got]
            assert all(isinstance(h, umlh.IndexSpan) and h.epoch.kind == umlh._lib.SPAN_FEISTEL for h in heads)
            assert all(h.epoch._order is None for h in heads), "a device epoch was materialised by the draw"
            assert _sizes(got) == _sizes(ref) and len(_sizes(got)) == n
            assert [h.numel() for h in heads] == [(b[0] if isinstance(b, tuple) else b).numel() for b in ref]
            assert [(h.start, h.count) for h in heads] == [(s.start, s.count) for s in (b[0] if isinstance(b, tuple) else b for b in ref)]
            assert _bench_rows(got) == _bench_rows(ref) == sum(_sizes(ref))
    # text: 100 rows in batches of 32 -> 32, 32, 32, 4, and an epoch's first batch is an entry of its own
    bi, bt = _draw_block(*_sources(3, "device"), 9)
    assert _sizes(bt) == [32, 32, 32, 4, 32, 32, 32, 4, 32] and _sizes(bi) == [32] * 9
    assert [isinstance(b, tuple) for b in bt] == [False, True, False, True, False]
    assert np.array_equal(np.cumsum(_sizes(bt)), [32, 64, 96, 100, 132, 164, 196, 200, 232])


def test_span_and_tensor_draws_consume_the_generator_alike():
    from finetune import _draw_block
    img, txt = _sources(8, "device")
    _draw_block(img, txt, 70)                          # image epoch 32 batches, text epoch 4: many epoch starts of both
    after_spans = torch.get_rng_state()
    img2, txt2 = _sources(8, "torch-cpu")
    for _ in range(70):
        img2.next_index(), txt2.next_index()
    assert torch.equal(after_spans, torch.get_rng_state())


def test_materialised_orders_keep_their_slices():
    from finetune import _draw_block
    for kw in (dict(order_rng="torch-cpu"), dict(order_rng="device", shuffle=False)):
        bi, bt = _draw_block(*_sources(5, **kw), 11)
        img2, txt2 = _sources(5, **kw)                 # the twin: reseeded after the block has made its draws
        steps = [(img2.next_index(), txt2.next_index()) for _ in range(11)]
        for got, ref in ((bi, [s[0] for s in steps]), (bt, [s[1] for s in steps])):
            ids = torch.cat([(b[0] if isinstance(b, tuple) else b).tensor() for b in got])
            assert torch.equal(ids, torch.cat(ref))


def test_span_bounds():
    import umlh
    ep = umlh.EpochOrder.permutation(10, 1, "cpu")
    assert umlh.IndexSpan(ep, 3, 7).numel() == 7 and umlh.IndexSpan(ep, 10, 0).numel() == 0
    for start, count in ((-1, 2), (4, 7), (0, -1)):
        with pytest.raises(umlh.UmlhError):
            umlh.IndexSpan(ep, start, count)


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: replayed only where no GPU is visible")
def test_index_block_refuses_bad_spans_before_any_launch():
    import umlh
    from umlh._lib import IndexSpanDesc, SPAN_FEISTEL, SPAN_TABLE
    umlh.build_library()
    lib = umlh.load_library()
    fake = C.c_void_p(4096)

    def call(spans, out=fake):
        arr = (IndexSpanDesc * len(spans))(*spans)
        return lib.umlh_index_block(arr, len(spans), out, None, 0, None, None), lib.umlh_last_error().decode()

    for spans, out, what in (([IndexSpanDesc(SPAN_FEISTEL, 0, 10, 1, None, 4, 7)], fake, "outside an order"),
                             ([IndexSpanDesc(SPAN_FEISTEL, 0, 10, 1, None, -1, 2)], fake, "outside an order"),
                             ([IndexSpanDesc(SPAN_FEISTEL, 0, 10, 1, None, 0, -1)], fake, "outside an order"),
                             ([IndexSpanDesc(7, 0, 10, 1, None, 0, 1)], fake, "unknown kind"),
                             ([IndexSpanDesc(SPAN_TABLE, 0, 10, 0, None, 0, 1)], fake, "needs its order"),
                             ([IndexSpanDesc(SPAN_FEISTEL, 0, 2 ** 62 + 1, 1, None, 0, 1)], fake, "2^62"),
                             ([IndexSpanDesc(SPAN_FEISTEL, 0, 10, 1, None, 0, 5)], None, "no destination")):
        rc, msg = call(spans, out)
        assert rc == -1 and "umlh_index_block" in msg and what in msg, (rc, msg)
    assert lib.umlh_index_block(None, 3, fake, None, 0, None, None) == -1
    # nothing to write is not an error and launches nothing
    assert lib.umlh_index_block(None, 0, None, None, 0, None, None) == 0
    assert call([IndexSpanDesc(SPAN_FEISTEL, 0, 10, 1, None, 10, 0)], None)[0] == 0
