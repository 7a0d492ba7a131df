"""The per-step logged statistics of the MultiBench training loop on the HIP kernels of umlh_kernels_stepstats.hip (C ABI:
``umlh_seq_step_stats``): ``train/trivial_loss_*`` and ``train/recon_y_loss`` of MultiBench/train.py:403-426, which the
reference computes with about twenty torch launches, [B, T, D] temporaries and three ``.item()`` reads per step.  One call
enqueues two launches on ``torch.cuda.current_stream`` and returns a device tensor; nothing is read back.  There is no CPU
compute path.
"""
from __future__ import annotations

import torch

from . import _glue as glue
from ._lib import check, load_library

MAX_B = 65535
TRIVIAL, TRIVIAL_COUNT, RECON, RECON_COUNT = range(4)          # the slots of the result


def _block(t: torch.Tensor, dev: torch.device) -> torch.Tensor:
    """An fp32 [B, T, d] device view with unit column stride (copied only when the last stride is not 1; any other stride
    problem is the C entry point's to name)."""
    t = t.detach().to(device=dev, dtype=torch.float32)
    return t if t.stride(2) == 1 else t.contiguous()


def seq_step_stats(x: torch.Tensor, lengths: torch.Tensor | None = None, recon: torch.Tensor | None = None) -> torch.Tensor:
    """``[trivial_loss, trivial_count, recon_loss, recon_count]`` of a padded [B, T, d] block: a float64 device tensor [4].

    With len_b = clamp(lengths[b], 0, T) (``lengths=None``: T everywhere) and sums over b, 0 <= t < T - 1 and all d columns:
    trivial_loss = sum [t < len_b] (x[b,t] - x[b,t+1])^2 / (trivial_count + 1e-8), the reference's mask[:, :-1], which lets the
    pair (len_b - 1, len_b) reach one row into the padding; recon_loss = sum [t + 1 < len_b] (recon[b,t] - x[b,t+1])^2 /
    (recon_count + 1e-8), its mask[:, 1:], which does not.  The counts are the numbers of elements summed.  ``recon=None``:
    slots 2 and 3 are 0.  T = 1: all four are 0.  Pairs a predicate excludes are skipped: Inf or NaN in the padding does not
    reach the result.  ``x`` and ``recon`` (same shape, layouts may differ) are read through their strides: a [T, B, d] block's
    ``.transpose(0, 1)`` or a column block of a wider tensor is used in place.  B <= 65535."""
    if not isinstance(x, torch.Tensor) or x.ndim != 3:
        raise ValueError(f"seq_step_stats: expected a 3-D tensor [B, T, d], got {getattr(x, 'shape', type(x))}")
    if not x.is_floating_point():
        raise ValueError(f"seq_step_stats: expected a floating-point tensor, got {x.dtype}")
    B, T, d = x.shape
    if B < 1 or T < 1 or d < 1:
        raise ValueError(f"seq_step_stats: empty input {tuple(x.shape)}")
    if B > MAX_B:
        raise ValueError(f"seq_step_stats: B={B} sequences (need B <= {MAX_B})")
    if recon is not None and (not isinstance(recon, torch.Tensor) or recon.shape != x.shape or not recon.is_floating_point()):
        raise ValueError(f"seq_step_stats: recon must be a floating-point tensor of x's shape {tuple(x.shape)}, got "
                         f"{getattr(recon, 'shape', type(recon))}")
    if lengths is not None and torch.as_tensor(lengths).numel() != B:
        raise ValueError(f"seq_step_stats: {torch.as_tensor(lengths).numel()} lengths for {B} sequences")
    dev = glue.device("umlh.stepstats", "the statistics are summed only by HIP kernels")
    xv = _block(x, dev)
    rv = None if recon is None else _block(recon, dev)
    if lengths is not None:
        lengths = torch.as_tensor(lengths).detach().reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    scratch, nbytes = glue.scratch("umlh_seq_step_stats_scratch_bytes", dev, b=B, t_len=T, d=d)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    check(load_library().umlh_seq_step_stats(xv.data_ptr(), xv.stride(0), xv.stride(1), glue.ptr(rv),
                                             0 if rv is None else rv.stride(0), 0 if rv is None else rv.stride(1), B, T, d,
                                             glue.ptr(lengths), out.data_ptr(), scratch.data_ptr(), nbytes, glue.stream(dev)),
          "umlh_seq_step_stats")
    return out
