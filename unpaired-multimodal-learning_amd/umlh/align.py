"""Representation-alignment metrics on the HIP kernels of umlh_kernels_align.hip (C ABI: ``umlh_align_*``).

``knn`` is the reference's ``compute_nearest_neighbors`` (vision_language/metrics.py:272-285), ``mutual_knn`` its
``AlignmentMetrics.mutual_knn`` (:55-84) and ``cka`` its ``AlignmentMetrics.cka(kernel_metric='ip', unbiased=False)``
(:96-119, :252-255).  Every call enqueues on ``torch.cuda.current_stream`` and returns device tensors without
synchronising.  Inputs: fp32 CUDA tensors with unit column stride are used in place (the row stride is passed on);
other float dtypes are upcast and CPU tensors copied to the current device.  There is no CPU compute path.
"""
from __future__ import annotations

import ctypes as C

import torch

from ._lib import UmlhError, check, load_library

MAX_TOPK = 32


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("umlh.align needs a GPU: the metrics run only as HIP kernels")
    return torch.device("cuda", torch.cuda.current_device())


def _features(t: torch.Tensor, what: str, dev: torch.device) -> torch.Tensor:
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


def _stream(dev: torch.device):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _scratch(lib, n, d_a, d_b, topk, splits, dev):
    nbytes = lib.umlh_align_scratch_bytes(n, d_a, d_b, topk, splits)
    if nbytes == 0:
        raise UmlhError(f"umlh_align_scratch_bytes: invalid arguments n={n} d_a={d_a} d_b={d_b} topk={topk} splits={splits}")
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def _check_topk(topk: int, n: int, what: str) -> None:
    if not 1 <= topk <= MAX_TOPK:
        raise ValueError(f"{what}: topk={topk} outside 1..{MAX_TOPK}")
    if topk >= n:
        raise ValueError(f"{what}: topk={topk} needs more than topk rows (got N={n})")


def knn(feats: torch.Tensor, topk: int, splits: int = 0, return_scores: bool = False):
    """Per row i, the ``topk`` columns j != i with the largest raw inner product feats_i . feats_j, ordered by
    (score desc, index asc): int32 [N, topk] on the device (and the fp32 scores when ``return_scores``)."""
    if not isinstance(feats, torch.Tensor) or feats.ndim != 2:
        raise ValueError(f"knn: expected a 2-D tensor [N, d], got {getattr(feats, 'shape', type(feats))}")
    n = feats.shape[0]
    _check_topk(int(topk), n, "knn")
    if splits < 0:
        raise ValueError(f"knn: splits={splits} < 0")
    dev = _device()
    x = _features(feats, "knn", dev)
    lib = load_library()
    d = x.shape[1]
    scratch, nbytes = _scratch(lib, n, d, d, topk, splits, dev)
    out = torch.empty((n, topk), dtype=torch.int32, device=dev)
    scores = torch.empty((n, topk), dtype=torch.float32, device=dev) if return_scores else None
    check(lib.umlh_align_knn(x.data_ptr(), n, d, x.stride(0), topk, splits, out.data_ptr(),
                             scores.data_ptr() if scores is not None else None, scratch.data_ptr(), nbytes, _stream(dev)),
          "umlh_align_knn")
    return (out, scores) if return_scores else out


def mutual_knn_lists(knn_a: torch.Tensor, knn_b: torch.Tensor) -> torch.Tensor:
    """Mean over rows of |knn_a(i) n knn_b(i)| / k for two int32 [N, k] neighbour lists: a 0-d float64 device tensor."""
    if knn_a.shape != knn_b.shape or knn_a.ndim != 2:
        raise ValueError(f"mutual_knn: neighbour lists of shapes {tuple(knn_a.shape)} and {tuple(knn_b.shape)}")
    dev = _device()
    n, topk = knn_a.shape
    _check_topk(topk, n, "mutual_knn")
    ka = knn_a.to(device=dev, dtype=torch.int32).contiguous()
    kb = knn_b.to(device=dev, dtype=torch.int32).contiguous()
    lib = load_library()
    scratch, nbytes = _scratch(lib, n, 1, 1, 0, 0, dev)
    out = torch.empty((), dtype=torch.float64, device=dev)
    check(lib.umlh_align_mutual_knn(ka.data_ptr(), kb.data_ptr(), n, topk, out.data_ptr(), scratch.data_ptr(), nbytes,
                                    _stream(dev)), "umlh_align_mutual_knn")
    return out


def mutual_knn(a: torch.Tensor, b: torch.Tensor, topk: int = 10, splits: int = 0) -> torch.Tensor:
    """AlignmentMetrics.mutual_knn(a, b, topk): a 0-d float64 device tensor."""
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)) or a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
        raise ValueError(f"mutual_knn: features of shapes {tuple(getattr(a, 'shape', ()))} and {tuple(getattr(b, 'shape', ()))} "
                         "(need 2-D with the same N)")
    _check_topk(int(topk), a.shape[0], "mutual_knn")
    return mutual_knn_lists(knn(a, topk, splits), knn(b, topk, splits))


def cka_terms(a: torch.Tensor, b: torch.Tensor, splits: int = 0) -> torch.Tensor:
    """float64 device tensor [4] = {cka, hsic_kl, hsic_kk, hsic_ll} (biased HSIC, linear kernel, no normalisation)."""
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)) or a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
        raise ValueError(f"cka: features of shapes {tuple(getattr(a, 'shape', ()))} and {tuple(getattr(b, 'shape', ()))} "
                         "(need 2-D with the same N)")
    if splits < 0:
        raise ValueError(f"cka: splits={splits} < 0")
    dev = _device()
    xa, xb = _features(a, "cka", dev), _features(b, "cka", dev)
    n = xa.shape[0]
    lib = load_library()
    scratch, nbytes = _scratch(lib, n, xa.shape[1], xb.shape[1], 0, splits, dev)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    check(lib.umlh_align_cka(xa.data_ptr(), xa.stride(0), xa.shape[1], xb.data_ptr(), xb.stride(0), xb.shape[1], n, splits,
                             out.data_ptr(), scratch.data_ptr(), nbytes, _stream(dev)), "umlh_align_cka")
    return out


def cka(a: torch.Tensor, b: torch.Tensor, splits: int = 0) -> torch.Tensor:
    """AlignmentMetrics.cka(a, b, kernel_metric='ip'): a 0-d float64 device tensor."""
    return cka_terms(a, b, splits)[0]
