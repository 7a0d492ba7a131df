"""The two device operations of the MultiBench embedding capture on the HIP kernels of umlh_kernels_capture.hip (C ABI:
``umlh_seq_compact``, ``umlh_paired_cosine``).

``seq_compact`` packs the valid rows (b, t < len_b) of a padded [B, T, d] block into consecutive rows of an [N, d] matrix,
bit for bit, which the reference does with one ``.item()`` and one slice per sequence (MultiBench/train.py:334-345,464-489).
``paired_cosine`` is ``F.cosine_similarity(a, b, dim=1).mean()`` (:494,:499) with fp64 accumulation.  Every call enqueues on
``torch.cuda.current_stream`` and returns device tensors; only ``seq_compact`` without ``out`` and ``rows`` reads anything
back (see there).  fp32 device tensors with unit column stride are read in place through their strides; other float dtypes
are upcast and CPU tensors copied to the current device.  There is no CPU compute path.

``class_index`` and ``class_stats`` (kernels: umlh_kernels_classstats.hip; C ABI: ``umlh_class_index``, ``umlh_class_stats``) are
the class-grouped part of the fine-tune loop's feature capture (vision_language/finetune.py:222-231): a stable counting sort of
the sample's rows by label, built once per run, and per class the mean row and the mean distance of the class's rows to it,
which the reference forms in a Python loop with one ``nonzero``, two reductions and one ``.item()`` per class.
"""
from __future__ import annotations

import math

import torch

from . import _glue as glue
from . import spectral
from ._lib import check, load_library

MAX_B = 65535


def _device() -> torch.device:
    return glue.device("umlh.capture", "rows are packed and compared only by HIP kernels")


def valid_rows(lengths, t_len: int, drop_last: int = 0):
    """Rows each sequence contributes: max(clamp(len, 0, t_len) - drop_last, 0), on whatever device ``lengths`` lives."""
    return (torch.as_tensor(lengths).reshape(-1).to(torch.int64).clamp(0, t_len) - drop_last).clamp_min(0)


def seq_compact(z: torch.Tensor, lengths: torch.Tensor | None = None, drop_last: int = 0, out: torch.Tensor | None = None,
                rows: int | None = None):
    """The rows (b, t) with t < clamp(lengths[b], 0, T) - drop_last of a [B, T, d] block, in (b, t) order, as the rows of a
    matrix -> ``(matrix, rows_total)``; ``rows_total`` is a 0-d int64 device tensor, the number of valid rows.

    ``out``: an fp32 device matrix [R, d] with unit column stride (a row slice or a column block of a larger one will do); it
    is written in place and returned, rows past R are dropped and rows the block does not fill are left as they were.
    ``rows``: the count the caller already knows on the host; a fresh [rows, d] matrix is returned.  With neither, and with
    ``lengths`` given, the lengths are read back to the host ONCE to size the result: that is a synchronisation (a device
    ``lengths`` tensor), so loops that must not stall pass ``out`` or ``rows``.  A permuted view such as a [T, B, d] block's
    ``.transpose(0, 1)`` or a column block of a wider tensor is read through its strides.  B <= 65535."""
    if not isinstance(z, torch.Tensor) or z.ndim != 3:
        raise ValueError(f"seq_compact: expected a 3-D tensor [B, T, d], got {getattr(z, 'shape', type(z))}")
    if not z.is_floating_point():
        raise ValueError(f"seq_compact: expected a floating-point tensor, got {z.dtype}")
    B, T, d = z.shape
    if B < 1 or T < 1 or d < 1:
        raise ValueError(f"seq_compact: empty input {tuple(z.shape)}")
    if B > MAX_B:
        raise ValueError(f"seq_compact: B={B} sequences (need B <= {MAX_B})")
    drop_last = int(drop_last)
    if drop_last < 0:
        raise ValueError(f"seq_compact: drop_last={drop_last} < 0")
    if lengths is not None and torch.as_tensor(lengths).numel() != B:
        raise ValueError(f"seq_compact: {torch.as_tensor(lengths).numel()} lengths for {B} sequences")
    if out is not None and rows is not None:
        raise ValueError("seq_compact: give out or rows, not both")
    dev = _device()
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.ndim != 2 or out.shape[1] != d or out.dtype != torch.float32
                or out.device != dev or (out.shape[0] > 0 and (out.stride(1) != 1 or out.stride(0) < d))):
            raise ValueError(f"seq_compact: out must be an fp32 [R, {d}] matrix on {dev} with unit column stride and a row stride >= {d}")
        n_out = out.shape[0]
    elif rows is not None:
        n_out = int(rows)
        if n_out < 0:
            raise ValueError(f"seq_compact: rows={rows} < 0")
    elif lengths is None:
        n_out = B * max(T - drop_last, 0)
    else:
        n_out = int(valid_rows(lengths, T, drop_last).sum())                      # the one read-back
    x = spectral._in_place(z, dev)
    if lengths is not None:
        lengths = torch.as_tensor(lengths).detach().reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    buf = out
    if buf is None or n_out == 0:
        buf = torch.empty((max(n_out, 1), d), dtype=torch.float32, device=dev)   # an empty tensor has no address to pass
    total = torch.empty((), dtype=torch.int64, device=dev)
    check(load_library().umlh_seq_compact(x.data_ptr(), B, T, d, x.stride(0), x.stride(1), glue.ptr(lengths), drop_last,
                                          buf.data_ptr(), buf.stride(0), n_out, total.data_ptr(), glue.stream(dev)),
          "umlh_seq_compact")
    return (out if out is not None else buf[:n_out]), total


def paired_cosine(a: torch.Tensor, b: torch.Tensor, eps: float = 1e-8, return_rows: bool = False):
    """F.cosine_similarity(a, b, dim=1, eps=eps).mean() for two [N, d] matrices: a 0-d float64 device tensor (and the fp32
    [N] per-row cosines when ``return_rows``).  Each norm is clamped at ``eps`` on its own, as torch does; dot products and
    squared norms are accumulated in fp64."""
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)) or a.ndim != 2 or a.shape != b.shape:
        raise ValueError(f"paired_cosine: features of shapes {tuple(getattr(a, 'shape', ()))} and {tuple(getattr(b, 'shape', ()))} "
                         "(need 2-D of the same shape)")
    eps = float(eps)
    if not eps >= 0.0 or math.isnan(eps):
        raise ValueError(f"paired_cosine: eps={eps} (need eps >= 0)")
    dev = _device()
    xa, xb = glue.features(a, "paired_cosine", dev), glue.features(b, "paired_cosine", dev)
    n, d = xa.shape
    scratch, nbytes = glue.scratch("umlh_paired_cosine_scratch_bytes", dev, n=n, d=d)
    out = torch.empty(2, dtype=torch.float64, device=dev)
    rows = torch.empty(n, dtype=torch.float32, device=dev) if return_rows else None
    check(load_library().umlh_paired_cosine(xa.data_ptr(), xa.stride(0), xb.data_ptr(), xb.stride(0), n, d, eps, out.data_ptr(),
                                            glue.ptr(rows), scratch.data_ptr(), nbytes, glue.stream(dev)), "umlh_paired_cosine")
    return (out[0], rows) if return_rows else out[0]


def class_index(labels: torch.Tensor, n_class: int):
    """Rows grouped by label -> ``(order, offsets)``: ``order`` (int32 [n]) lists the rows whose label lies in [0, n_class),
    classes ascending and rows ascending inside a class; class c is ``order[offsets[c]:offsets[c + 1]]`` (``offsets`` int64
    [n_class + 1]).  Rows with any other label appear nowhere and the entries of ``order`` past ``offsets[n_class]`` are not
    written.  Device tensors, no host sync."""
    if not isinstance(labels, torch.Tensor) or labels.ndim != 1 or labels.numel() < 1:
        raise ValueError(f"class_index: expected a non-empty 1-D label tensor, got {getattr(labels, 'shape', type(labels))}")
    if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise ValueError(f"class_index: expected integer labels, got {labels.dtype}")
    n_class = int(n_class)
    if n_class < 1:
        raise ValueError(f"class_index: n_class={n_class} < 1")
    dev = _device()
    y = labels.detach().to(device=dev, dtype=torch.int64).contiguous()
    n = y.numel()
    scratch, nbytes = glue.scratch("umlh_class_index_scratch_bytes", dev, n=n, n_class=n_class)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    offsets = torch.empty(n_class + 1, dtype=torch.int64, device=dev)
    check(load_library().umlh_class_index(y.data_ptr(), n, n_class, order.data_ptr(), offsets.data_ptr(), scratch.data_ptr(), nbytes,
                                          glue.stream(dev)), "umlh_class_index")
    return order, offsets


def class_stats(feats: torch.Tensor, order: torch.Tensor, offsets: torch.Tensor, n_class: int, means_out: torch.Tensor | None = None):
    """Per class c with rows ``order[offsets[c]:offsets[c + 1]]`` of ``feats`` [n, d] -> ``(means, dist, out2)``: ``means`` fp32
    [n_class, d] the class mean rows (fp64 sums, rounded once), ``dist`` float64 [n_class] the mean over the class's rows of
    their distance to the mean that was written, ``out2`` float64 [2] = {mean over classes of dist, number of empty classes}.
    An empty class gives a NaN row and a NaN distance, so ``out2[0]`` is NaN when a class is empty.  ``feats`` with unit column
    stride is read in place through its row stride; ``means_out``: an fp32 device matrix [n_class, d] with unit column stride
    (a column block of a wider one will do), written in place and returned.  Device tensors, no host sync."""
    dev = _device()
    x = glue.features(feats, "class_stats", dev)
    n, d = x.shape
    n_class = int(n_class)
    if n_class < 1:
        raise ValueError(f"class_stats: n_class={n_class} < 1")
    if not isinstance(order, torch.Tensor) or order.ndim != 1 or order.numel() < n:
        raise ValueError(f"class_stats: order must be a 1-D tensor with room for {n} rows, got {getattr(order, 'shape', type(order))}")
    if not isinstance(offsets, torch.Tensor) or offsets.ndim != 1 or offsets.numel() != n_class + 1:
        raise ValueError(f"class_stats: offsets must hold n_class + 1 = {n_class + 1} entries, got {getattr(offsets, 'shape', type(offsets))}")
    order = order.detach().to(device=dev, dtype=torch.int32).contiguous()
    offsets = offsets.detach().to(device=dev, dtype=torch.int64).contiguous()
    if means_out is None:
        means = torch.empty((n_class, d), dtype=torch.float32, device=dev)
    else:
        means = means_out
        if (not isinstance(means, torch.Tensor) or means.ndim != 2 or tuple(means.shape) != (n_class, d) or means.dtype != torch.float32
                or means.device != dev or means.stride(1) != 1 or means.stride(0) < d):
            raise ValueError(f"class_stats: means_out must be an fp32 [{n_class}, {d}] matrix on {dev} with unit column stride and a "
                             f"row stride >= {d}")
    scratch, nbytes = glue.scratch("umlh_class_stats_scratch_bytes", dev, n=n, d=d, n_class=n_class)
    dist = torch.empty(n_class, dtype=torch.float64, device=dev)
    out2 = torch.empty(2, dtype=torch.float64, device=dev)
    check(load_library().umlh_class_stats(x.data_ptr(), x.stride(0), n, d, order.data_ptr(), offsets.data_ptr(), n_class,
                                          means.data_ptr(), means.stride(0), dist.data_ptr(), out2.data_ptr(), scratch.data_ptr(),
                                          nbytes, glue.stream(dev)), "umlh_class_stats")
    return means, dist, out2
