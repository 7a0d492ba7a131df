"""The reference's MultiBench/utilis.py by name: ``set_seed``, ``cka``, ``mknn`` and ``compute_effective_rank``.  The metrics
run on the HIP kernels of ``umlh``; the augmentation helpers of the reference module are host-RNG code that its ``train``
never calls and are not mirrored."""
from __future__ import annotations

import os
import random

import numpy as np
import torch


def set_seed(seed):
    """utilis.py:8-16."""
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False
    os.environ["PYTHONHASHSEED"] = str(seed)


def cka(feats_A, feats_B):
    """utilis.py:19-21: linear CKA as a Python float."""
    import metrics
    return metrics.cka(feats_A, feats_B)


def mknn(feats_A, feats_B):
    """utilis.py:23-25: mutual k-NN with topk = 10 as a Python float."""
    import metrics
    return metrics.mknn(feats_A, feats_B)


def compute_effective_rank(A, eps=1e-6):
    """utilis.py:27-36.  A: (B, N, D) tensor; returns the (B,) fp32 tensor of effective ranks on A's device.  The spectrum
    comes from ``umlh.spectral`` (fp64 Gram + symmetric eigenvalues) rather than an fp32 SVD; nothing synchronises."""
    import umlh
    if not isinstance(A, torch.Tensor) or A.ndim != 3:
        raise ValueError(f"compute_effective_rank: expected a (B, N, D) tensor, got {getattr(A, 'shape', type(A))}")
    return umlh.effective_rank(A, eps).to(device=A.device, dtype=torch.float32)
