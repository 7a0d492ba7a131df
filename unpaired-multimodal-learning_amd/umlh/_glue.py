"""What every caller of the C ABI needs from torch: device pointers, the current stream's handle, the current device,
feature matrices the kernels can read in place and scratch sized by the library's own queries.  Host-side only; ``_lib``
stays free of torch."""
from __future__ import annotations

import ctypes as C

import torch

from ._lib import UmlhError, load_library


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def stream(dev):
    """The hipStream_t of torch's CURRENT stream on ``dev``, as the ``void* stream`` of every entry point."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def device(who: str, why: str) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who} needs a GPU: {why}")
    return torch.device("cuda", torch.cuda.current_device())


def features(t: torch.Tensor, what: str, dev: torch.device) -> torch.Tensor:
    """An fp32 [N, d] device matrix with unit column stride and a row stride >= d (a view of ``t`` where it already is one)."""
    if not isinstance(t, torch.Tensor) or t.ndim != 2:
        raise ValueError(f"{what}: expected a 2-D tensor [N, d], got {getattr(t, 'shape', type(t))}")
    if not t.is_floating_point():
        raise ValueError(f"{what}: expected a floating-point tensor, got {t.dtype}")
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: empty features {tuple(t.shape)}")
    t = t.detach().to(device=dev, dtype=torch.float32)
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def scratch(query_name: str, dev: torch.device, **args):
    """(uint8 device tensor, its size) for the ``*_scratch_bytes`` query ``query_name`` called with ``args`` in order; the
    queries answer 0 for arguments outside their entry point's envelope."""
    nbytes = getattr(load_library(), query_name)(*args.values())
    if nbytes == 0:
        raise UmlhError(f"{query_name}: invalid arguments " + " ".join(f"{k}={v}" for k, v in args.items()))
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes
