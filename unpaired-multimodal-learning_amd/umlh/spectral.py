"""Singular values, effective rank and principal subspaces on the HIP kernels of umlh_kernels_spectral.hip (C ABI:
``umlh_svdvals``, ``umlh_effective_rank``, ``umlh_effective_rank_seq``, ``umlh_principal_subspace``).

``svdvals`` is ``torch.linalg.svdvals`` for [n, d] or [batch, n, d] fp32 matrices with d <= 512, ``effective_rank`` the
reference's ``compute_effective_rank`` (MultiBench/utilis.py:27-36) and ``effective_rank_seq`` the same number for the valid
rows of a block of padded sequences pooled into one matrix, which is how MultiBench/train.py:380-389 uses it.  The singular
values are the roots of the eigenvalues of the fp64 Gram matrix; results are float64 device tensors.  Every call enqueues
on ``torch.cuda.current_stream`` and returns without synchronising.  fp32 device tensors with unit column stride are read in
place through their strides; other float dtypes are upcast and CPU tensors copied to the current device.  There is no CPU
compute path.

``principal_subspace`` returns the top-q eigenpairs of the Gram ``a^T a`` of an [n, d] matrix, or of the Gram of its
standardised columns (the PCA of the correlation matrix times n - 1): see its docstring and DESIGN section 13.
"""
from __future__ import annotations

import operator

import torch

from . import _glue as glue
from ._lib import check, load_library

MAX_D = 512
MAX_Q = 64
CHUNK_ROWS = 256
MAX_CHUNKS = 128


def chunk_count(batch: int, n: int) -> int:
    """Row chunks per matrix, each with its own d x d fp64 partial slab: min(ceil(n / 256), max(1, 128 // batch))."""
    return max(1, min(-(-n // CHUNK_ROWS), max(1, MAX_CHUNKS // batch)))


def _device() -> torch.device:
    return glue.device("umlh.spectral", "the spectrum is computed only by HIP kernels")


def _no_overlap(outer: int, inner: int, d: int, so: int, si: int) -> bool:
    if si < d or (outer > 1 and so < d):
        return False
    if outer <= 1 or inner <= 1:
        return True
    return so >= (inner - 1) * si + d or si >= (outer - 1) * so + d


def _matrix(a, what: str):
    """The checks that need no device -> (batch, n, d, batched)."""
    if not isinstance(a, torch.Tensor) or a.ndim not in (2, 3):
        raise ValueError(f"{what}: expected a 2-D [n, d] or 3-D [batch, n, d] tensor, got {getattr(a, 'shape', type(a))}")
    if not a.is_floating_point():
        raise ValueError(f"{what}: expected a floating-point tensor, got {a.dtype}")
    batched = a.ndim == 3
    batch, n, d = a.shape if batched else (1, *a.shape)
    if batch < 1 or n < 1 or d < 1:
        raise ValueError(f"{what}: empty input {tuple(a.shape)}")
    if d > MAX_D:
        raise ValueError(f"{what}: d={d} outside 1..{MAX_D}")
    if batch * n >= 2 ** 31:
        raise ValueError(f"{what}: batch * n = {batch * n} rows (need < 2^31)")
    return batch, n, d, batched


def _in_place(a: torch.Tensor, dev: torch.device) -> torch.Tensor:
    """A 3-D fp32 device view the kernels can read by (stride 0, stride 1, unit column stride)."""
    a = a.detach().to(device=dev, dtype=torch.float32)
    if a.ndim == 2:
        a = a.unsqueeze(0)
    if a.stride(2) != 1 or not _no_overlap(a.shape[0], a.shape[1], a.shape[2], a.stride(0), a.stride(1)):
        a = a.contiguous()
    return a


def svdvals(a: torch.Tensor) -> torch.Tensor:
    """torch.linalg.svdvals(a): float64 device tensor [min(n, d)] or [batch, min(n, d)], descending."""
    batch, n, d, batched = _matrix(a, "svdvals")
    dev = _device()
    x = _in_place(a, dev)
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_spectral_scratch_bytes", dev, batch=batch, n=n, d=d)
    sv = torch.empty((batch, min(n, d)), dtype=torch.float64, device=dev)
    check(lib.umlh_svdvals(x.data_ptr(), batch, n, d, x.stride(0), x.stride(1), sv.data_ptr(), scratch.data_ptr(), nbytes,
                           glue.stream(dev)), "umlh_svdvals")
    return sv if batched else sv[0]


def _eps(eps, what: str) -> float:
    eps = float(eps)
    if not (0.0 <= eps < float("inf")):
        raise ValueError(f"{what}: eps={eps} (need a finite eps >= 0)")
    return eps


def effective_rank(a: torch.Tensor, eps: float = 1e-6, return_svdvals: bool = False):
    """compute_effective_rank(a, eps): exp of the entropy of the normalised singular values; a float64 device tensor, 0-d for
    [n, d] and [batch] for [batch, n, d] (and the singular values when ``return_svdvals``)."""
    batch, n, d, batched = _matrix(a, "effective_rank")
    eps = _eps(eps, "effective_rank")
    dev = _device()
    x = _in_place(a, dev)
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_spectral_scratch_bytes", dev, batch=batch, n=n, d=d)
    out = torch.empty(batch, dtype=torch.float64, device=dev)
    sv = torch.empty((batch, min(n, d)), dtype=torch.float64, device=dev) if return_svdvals else None
    check(lib.umlh_effective_rank(x.data_ptr(), batch, n, d, x.stride(0), x.stride(1), eps, out.data_ptr(),
                                  glue.ptr(sv), scratch.data_ptr(), nbytes, glue.stream(dev)),
          "umlh_effective_rank")
    out = out if batched else out[0]
    if return_svdvals:
        return out, (sv if batched else sv[0])
    return out


def effective_rank_seq(z: torch.Tensor, lengths: torch.Tensor | None = None, drop_last: int = 0, eps: float = 1e-6,
                       return_svdvals: bool = False):
    """Effective rank of the rows (b, t) with t < clamp(lengths[b], 0, T) - drop_last of a [B, T, d] block, pooled into one
    matrix: float64 device tensor [2] = {effective rank, number of valid rows} (and the [d] singular values, zero past
    min(rows, d), when ``return_svdvals``).  A permuted view such as a [T, B, d] block's ``.transpose(0, 1)`` or a column
    block of a wider tensor is read through its strides."""
    if not isinstance(z, torch.Tensor) or z.ndim != 3:
        raise ValueError(f"effective_rank_seq: expected a 3-D tensor [B, T, d], got {getattr(z, 'shape', type(z))}")
    if not z.is_floating_point():
        raise ValueError(f"effective_rank_seq: expected a floating-point tensor, got {z.dtype}")
    B, T, d = z.shape
    if B < 1 or T < 1 or d < 1:
        raise ValueError(f"effective_rank_seq: empty input {tuple(z.shape)}")
    if d > MAX_D:
        raise ValueError(f"effective_rank_seq: d={d} outside 1..{MAX_D}")
    if B * T >= 2 ** 31:
        raise ValueError(f"effective_rank_seq: B * T = {B * T} rows (need < 2^31)")
    drop_last = int(drop_last)
    if drop_last < 0:
        raise ValueError(f"effective_rank_seq: drop_last={drop_last} < 0")
    eps = _eps(eps, "effective_rank_seq")
    if lengths is not None and lengths.numel() != B:
        raise ValueError(f"effective_rank_seq: {lengths.numel()} lengths for {B} sequences")
    dev = _device()
    x = _in_place(z, dev)
    if lengths is not None:
        lengths = lengths.detach().reshape(-1).to(device=dev, dtype=torch.int64).contiguous()
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_spectral_scratch_bytes", dev, batch=1, n=B * T, d=d)
    out = torch.empty(2, dtype=torch.float64, device=dev)
    sv = torch.empty(d, dtype=torch.float64, device=dev) if return_svdvals else None
    check(lib.umlh_effective_rank_seq(x.data_ptr(), B, T, d, x.stride(0), x.stride(1), glue.ptr(lengths), drop_last, eps,
                                      out.data_ptr(), glue.ptr(sv), scratch.data_ptr(), nbytes, glue.stream(dev)),
          "umlh_effective_rank_seq")
    return (out, sv) if return_svdvals else out


def check_view(a, what: str):
    """The checks of one [n, d] view that need no device -> (n, d)."""
    if not isinstance(a, torch.Tensor) or a.ndim != 2:
        raise ValueError(f"{what}: expected a 2-D tensor [n, d], got {getattr(a, 'shape', type(a))}")
    if not a.is_floating_point():
        raise ValueError(f"{what}: expected a floating-point tensor, got {a.dtype}")
    n, d = a.shape
    if not 2 <= n < 2 ** 31:
        raise ValueError(f"{what}: n={n} rows (need 2 <= n < 2^31)")
    if not 1 <= d <= MAX_D:
        raise ValueError(f"{what}: d={d} outside 1..{MAX_D}")
    return n, d


def check_q(q, limit: int, what: str) -> int:
    try:
        q = operator.index(q)
    except TypeError:
        raise ValueError(f"{what}: q={q!r} is not an integer") from None
    if not 1 <= q <= min(limit, MAX_Q):
        raise ValueError(f"{what}: q={q} outside 1..{min(limit, MAX_Q)} (min of n, d and {MAX_Q})")
    return q


def rows_in_place(a: torch.Tensor, dev: torch.device) -> torch.Tensor:
    """A 2-D fp32 device view with unit column stride and a row stride in d..2^31 - 1."""
    a = a.detach().to(device=dev, dtype=torch.float32)
    if a.stride(1) != 1 or not a.shape[1] <= a.stride(0) < 2 ** 31:
        a = a.contiguous()
    return a


def principal_subspace(a: torch.Tensor, q: int, standardize: bool = False):
    """The top-q eigenpairs of the Gram of an [n, d] matrix: ``(evals[q], evecs[d, q])``, float64 device tensors, eigenvalues
    descending, eigenvectors in columns, orthonormal, each with its largest-magnitude component positive.

    ``standardize=False``: the Gram is ``a^T a``, so ``evals.sqrt()`` are the first q values of ``svdvals(a)``.
    ``standardize=True``: the columns are first centred and divided by (unbiased std + 1e-8), as the reference's SVCCA does
    (MultiBench/metrics.py:132-135); a constant column is then exactly zero.  ``a @ evecs / evals.sqrt()`` of the standardised
    matrix are its top-q left singular vectors.  2 <= n < 2^31, d <= 512, q <= min(n, d, 64).  Eigenvectors of eigenvalues that
    are equal (to rounding) span the right subspace but are otherwise arbitrary; a NaN or Inf in the input makes everything NaN."""
    n, d = check_view(a, "principal_subspace")
    q = check_q(q, min(n, d), "principal_subspace")
    dev = _device()
    x = rows_in_place(a, dev)
    lib = load_library()
    scratch, nbytes = glue.scratch("umlh_subspace_scratch_bytes", dev, n=n, d_a=d, d_b=0, q=q)
    evals = torch.empty(q, dtype=torch.float64, device=dev)
    evecs = torch.empty((d, q), dtype=torch.float64, device=dev)
    check(lib.umlh_principal_subspace(x.data_ptr(), n, d, x.stride(0), q, int(bool(standardize)), evals.data_ptr(), evecs.data_ptr(),
                                      scratch.data_ptr(), nbytes, glue.stream(dev)), "umlh_principal_subspace")
    return evals, evecs
