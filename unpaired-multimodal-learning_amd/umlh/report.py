"""The class-wise validation report on the HIP kernels of umlh_kernels_evalreport.hip (C ABI: ``umlh_eval_topk``,
``umlh_eval_classwise``).

``topk_classes`` gives, per feature row, the k classes of a linear head with the largest logits
``z_j = scale * (x . w_j + b_j)`` ordered by (z descending, class index ascending), without forming the [n, C] logits: the
streaming top-k core the k-NN probe runs picks k + 8 candidates from fp32 MFMA scores, an fp64 pass re-evaluates and re-ranks
them.  ``class_report`` turns such lists and the labels into per-class counters (support, top-1 hits, top-k hits, optionally the
confusion matrix) with integer atomics, adding into its outputs so a table can be fed in slabs.  Every call enqueues on
``torch.cuda.current_stream`` and returns device tensors; nothing synchronises.  There is no CPU compute path.
"""
from __future__ import annotations

import torch

from . import _glue as glue
from ._lib import check, load_library

MAX_K = 24


def _device() -> torch.device:
    return glue.device("umlh.report", "the top-k classes and the class-wise counters are computed only by HIP kernels")


def topk_classes(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, scale: torch.Tensor | None = None,
                 k: int = 5, splits: int = 0):
    """``(cls int32 [n, k], logits fp32 [n, k])``: the k classes with the largest ``scale * (x @ weight.T + bias)`` per row of
    ``x`` [n, d], best first, exact ties to the smaller class index, and their logits (fp64 values rounded once to fp32).

    ``x`` and ``weight`` [C, d] with unit column stride are read in place through their row strides (the packed
    [weight | bias | pad] rows of a bias head give a row stride > d); ``bias``: [C] or None; ``scale``: a 0-dim DEVICE tensor
    (it is never read on the host; a negative value ranks by the negated pre-scale logit) or None for 1.  A row containing NaN
    gets class -1 and NaN logits; every other class index lies in [0, C).  ``splits`` (0 = auto) is the number of column chunks
    of the candidate pass; no result depends on it.  1 <= k <= 24, k <= C."""
    k, splits = int(k), int(splits)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"topk_classes: k={k} outside 1..{MAX_K}")
    if splits < 0:
        raise ValueError(f"topk_classes: splits={splits} must be >= 0")
    dev = _device()
    xx, w = glue.features(x, "topk_classes (x)", dev), glue.features(weight, "topk_classes (weight)", dev)
    (n, d), c = xx.shape, w.shape[0]
    if w.shape[1] != d:
        raise ValueError(f"topk_classes: x has {d} columns, weight {w.shape[1]}")
    if c < k:
        raise ValueError(f"topk_classes: k={k} classes asked of a head with {c}")
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.numel() != c:
            raise ValueError(f"topk_classes: bias must hold {c} values, got {getattr(bias, 'shape', type(bias))}")
        bias = bias.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
    if scale is not None:
        if not isinstance(scale, torch.Tensor) or scale.numel() != 1 or scale.device != dev:
            raise ValueError(f"topk_classes: scale must be a one-element tensor on {dev} (it is read by the kernels only)")
        scale = scale.detach().reshape(()).to(torch.float32)
    scratch, nbytes = glue.scratch("umlh_eval_topk_scratch_bytes", dev, n=n, n_class=c, d=d, k=k, splits=splits)
    cls = torch.empty((n, k), dtype=torch.int32, device=dev)
    logits = torch.empty((n, k), dtype=torch.float32, device=dev)
    check(load_library().umlh_eval_topk(xx.data_ptr(), n, xx.stride(0), w.data_ptr(), c, w.stride(0), d, glue.ptr(bias), glue.ptr(scale),
                                        k, splits, cls.data_ptr(), logits.data_ptr(), scratch.data_ptr(), nbytes, glue.stream(dev)),
          "umlh_eval_topk")
    return cls, logits


def class_report(cls: torch.Tensor, labels: torch.Tensor, n_class: int, confusion: bool = False, out: dict | None = None) -> dict:
    """Class-wise counters of the lists ``cls`` (int32 [n, k], best first: what ``topk_classes`` returns) against ``labels``
    [n] -> a dict of int64 device tensors: ``support`` [C] (rows of each true class), ``hit1`` [C] (``cls[i, 0] == label``),
    ``hitk`` [C] (label among ``cls[i, :]``), ``misc`` [2] = {rows whose label lies outside [0, C), counted nowhere else; rows
    with a valid label but no prediction (``cls[i, 0]`` outside [0, C)), counted in ``support`` only} and, with ``confusion``,
    ``confusion`` [C, C] (row = true class, column = ``cls[i, 0]``).

    ``out``: the dict of an earlier call with the same ``n_class`` and ``confusion``; the counts are added into it and it is
    returned, so a table can be fed in slabs.  Integer atomics only: results are reproducible.  Nothing synchronises."""
    n_class = int(n_class)
    if n_class < 1:
        raise ValueError(f"class_report: n_class={n_class} < 1")
    if not isinstance(cls, torch.Tensor) or cls.ndim != 2 or cls.dtype != torch.int32 or cls.shape[0] < 1 or not 1 <= cls.shape[1] <= MAX_K:
        raise ValueError(f"class_report: cls must be an int32 tensor [n >= 1, 1 <= k <= {MAX_K}], got "
                         f"{getattr(cls, 'dtype', None)} {getattr(cls, 'shape', type(cls))}")
    n, k = cls.shape
    if not isinstance(labels, torch.Tensor) or labels.ndim != 1 or labels.numel() != n:
        raise ValueError(f"class_report: expected {n} labels, got {getattr(labels, 'shape', type(labels))}")
    if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool:
        raise ValueError(f"class_report: expected integer labels, got {labels.dtype}")
    dev = _device()
    cls = cls.detach().to(dev).contiguous()
    y = labels.detach().to(device=dev, dtype=torch.int64).contiguous()
    if out is None:
        out = {name: torch.zeros(n_class, dtype=torch.int64, device=dev) for name in ("support", "hit1", "hitk")}
        out["misc"] = torch.zeros(2, dtype=torch.int64, device=dev)
        if confusion:
            out["confusion"] = torch.zeros((n_class, n_class), dtype=torch.int64, device=dev)
    else:
        want = {"support": (n_class,), "hit1": (n_class,), "hitk": (n_class,), "misc": (2,)}
        if confusion:
            want["confusion"] = (n_class, n_class)
        for name, shape in want.items():
            t = out.get(name)
            if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.int64 or t.device != dev
                    or not t.is_contiguous()):
                raise ValueError(f"class_report: out[{name!r}] must be a contiguous int64 tensor {shape} on {dev}")
        if not confusion and "confusion" in out:
            raise ValueError("class_report: out holds a confusion matrix; pass confusion=True to keep adding into it")
    check(load_library().umlh_eval_classwise(cls.data_ptr(), n, k, y.data_ptr(), n_class, out["support"].data_ptr(),
                                             out["hit1"].data_ptr(), out["hitk"].data_ptr(), glue.ptr(out.get("confusion")),
                                             out["misc"].data_ptr(), glue.stream(dev)), "umlh_eval_classwise")
    return out
