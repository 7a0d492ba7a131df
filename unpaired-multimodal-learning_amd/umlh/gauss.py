"""The Gaussian toy's SharedAutoencoder on the HIP kernels of umlh_kernels_gauss.hip (C ABI: ``umlh_ae_forward``,
``umlh_ae_train_steps``; reference Gaussian_experiment/model.py:5-59, main.py:33-91).

``ae_forward`` is the evaluation forward of either or both views in one call; ``ae_train_steps`` runs whole training steps
(both views, forward, MSE, backward, optimizer update) as two launches each, with the batches gathered by index from
device-resident tables.  Both enqueue on ``torch.cuda.current_stream`` and return device tensors; nothing is read back.  The
parameter and moment tensors are updated in place through their own storages.  There is no CPU compute path."""
from __future__ import annotations

import ctypes as C

import torch

from . import _glue as glue
from ._lib import OPT_IDS, AeCfg, UmlhError, check, load_library

N_TENSORS = 16    # state_dict order: in_head_x, in_head_y, shared_encoder.0/.2, shared_decoder.0/.2, out_head_x, out_head_y (weight, bias)

_SCRATCH = {}     # (device, stream, D, C, L, rows_x, rows_y, train) -> (uint8 tensor, bytes): leased per shape and stream


def tensor_shapes(D: int, C: int, L: int):
    """The 16 shapes of the model's tensors in ``state_dict`` order."""
    return [(C, D), (C,), (C, D), (C,), (L, C), (L,), (L, L), (L,), (L, L), (L,), (C, L), (C,), (D, C), (D,), (D, C), (D,)]


def _dims(params, who):
    params = list(params)
    if len(params) != N_TENSORS:
        raise ValueError(f"{who}: expected {N_TENSORS} parameter tensors in state_dict order, got {len(params)}")
    if params[0].ndim != 2 or params[4].ndim != 2:
        raise ValueError(f"{who}: in_head_x.weight and shared_encoder.0.weight must be 2-D")
    C_, D = params[0].shape
    L = params[4].shape[0]
    return params, int(D), int(C_), int(L)


def _bound(tensors, shapes, what, who, dev):
    """The tensors themselves (their storages are what the kernels update): dense fp32 on ``dev`` with the model's shapes."""
    for i, (t, s) in enumerate(zip(tensors, shapes)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(s):
            raise ValueError(f"{who}: {what}[{i}] must have shape {tuple(s)}, got {getattr(t, 'shape', type(t))}")
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise ValueError(f"{who}: {what}[{i}] must be a contiguous fp32 tensor on {dev} (it is used in place)")
    return [t.detach() for t in tensors]


def _table(t, D, what, who, dev):
    if t is None:
        return None, 0, D
    if not isinstance(t, torch.Tensor) or t.ndim != 2 or t.shape[1] != D or t.dtype != torch.float32 or t.device != dev:
        raise ValueError(f"{who}: {what} must be an fp32 [n, {D}] tensor on {dev}, got {getattr(t, 'shape', type(t))}")
    t = t.detach()
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < D):
        t = t.contiguous()
    return t, int(t.shape[0]), int(t.stride(0)) if t.shape[0] > 1 else D


def _index(idx, count, what, who, dev):
    if idx is None:
        return None
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32 or idx.device != dev or not idx.is_contiguous() \
            or idx.numel() != count:
        raise ValueError(f"{who}: {what} must be a contiguous int32 tensor of {count} row ids on {dev}")
    return idx


def _scratch(dev, cfg, rows_x, rows_y, train):
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, cfg.dim_obs, cfg.dim_common, cfg.dim_latent, rows_x, rows_y, train)
    hit = _SCRATCH.get(key)
    if hit is None:
        nbytes = load_library().umlh_ae_scratch(C.byref(cfg), rows_x, rows_y, train)
        if nbytes == 0:
            raise UmlhError(f"umlh_ae_scratch: invalid arguments D={cfg.dim_obs} C={cfg.dim_common} L={cfg.dim_latent} "
                            f"rows_x={rows_x} rows_y={rows_y} train={train}")
        if len(_SCRATCH) >= 16:
            _SCRATCH.clear()
        hit = _SCRATCH[key] = (torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes)
    return hit


def ae_forward(params, x=None, y=None, idx_x=None, idx_y=None, losses=True, recon=True, embeddings=True):
    """``(losses, rec_x, rec_y, emb_x, emb_y)`` of the evaluation forward.  ``params``: the 16 tensors in ``state_dict`` order.
    ``x`` / ``y``: fp32 device tables [n, D] (a row stride >= D is read in place) or None (view absent; at least one).
    ``idx_x`` / ``idx_y``: optional int32 device row ids: the view's rows are ``table[idx]``.  ``losses``: a float32 device
    tensor [2] = (loss_x, loss_y), 0 for an absent view; an output that is switched off is None."""
    who = "umlh.gauss.ae_forward"
    dev = glue.device("umlh.gauss", "the autoencoder runs only on its HIP kernels")
    params, D, C_, L = _dims(params, who)
    params = _bound(params, tensor_shapes(D, C_, L), "params", who, dev)
    xt, nx, ldx = _table(x, D, "x", who, dev)
    yt, ny, ldy = _table(y, D, "y", who, dev)
    if idx_x is not None and xt is not None:
        nx = idx_x.numel()
    if idx_y is not None and yt is not None:
        ny = idx_y.numel()
    idx_x = _index(idx_x, nx, "idx_x", who, dev) if xt is not None else None
    idx_y = _index(idx_y, ny, "idx_y", who, dev) if yt is not None else None
    if nx == 0 and ny == 0:
        raise ValueError(f"{who}: both views are absent")
    cfg = AeCfg(D, C_, L)
    scratch, nbytes = _scratch(dev, cfg, nx, ny, 0)
    new = lambda on, n, w: torch.empty((n, w), dtype=torch.float32, device=dev) if on and n else None
    out_l = torch.empty(2, dtype=torch.float32, device=dev) if losses else None
    rec_x, rec_y, emb_x, emb_y = new(recon, nx, D), new(recon, ny, D), new(embeddings, nx, L), new(embeddings, ny, L)
    check(load_library().umlh_ae_forward(C.byref(cfg), glue.ptr_array(params), glue.ptr(xt), ldx, glue.ptr(idx_x), nx, glue.ptr(yt), ldy,
                                         glue.ptr(idx_y), ny, glue.ptr(out_l), glue.ptr(rec_x), glue.ptr(rec_y), glue.ptr(emb_x),
                                         glue.ptr(emb_y), scratch.data_ptr(), nbytes, glue.stream(dev)), "umlh_ae_forward")
    return out_l, rec_x, rec_y, emb_x, emb_y


def ae_train_steps(params, m, v, x, y, idx_x, idx_y, batch_x, batch_y, n_steps, *, mode="xy", alpha_x=1.0, alpha_y=1.0,
                   optimizer="adam", lr=1e-3, first_step=1, betas=(0.9, 0.999), eps=1e-8, momentum=0.9, weight_decay=0.0,
                   losses=None):
    """``n_steps`` fused training steps; returns the float32 device tensor [n_steps, 3] of (loss_x, loss_y, loss) per step.
    ``params``, ``m``, ``v``: 16 tensors each in ``state_dict`` order, UPDATED IN PLACE (``v`` may be None under sgd).  ``x`` /
    ``y``: fp32 device tables [n, D]; ``idx_x`` / ``idx_y``: int32 device row ids, ``n_steps * batch`` of them: step s takes
    ``idx[s * batch : (s + 1) * batch]``.  The ids are used as addresses unchecked: the caller guarantees ``0 <= id < n``.
    ``mode='x'``: the y view runs forward only and ``in_head_y`` / ``out_head_y`` and their moments are not touched."""
    who = "umlh.gauss.ae_train_steps"
    if mode not in ("xy", "x"):
        raise ValueError(f"{who}: mode={mode!r} (expected 'xy' or 'x')")
    if optimizer not in OPT_IDS:
        raise ValueError(f"{who}: optimizer={optimizer!r} (expected one of {sorted(OPT_IDS)})")
    dev = glue.device("umlh.gauss", "the autoencoder runs only on its HIP kernels")
    params, D, C_, L = _dims(params, who)
    shapes = tensor_shapes(D, C_, L)
    params = _bound(params, shapes, "params", who, dev)
    m = _bound(list(m), shapes, "m", who, dev)
    if v is None and optimizer != "sgd":
        raise ValueError(f"{who}: v is required under {optimizer}")
    v = None if v is None else _bound(list(v), shapes, "v", who, dev)
    batch_x, batch_y, n_steps = int(batch_x), int(batch_y), int(n_steps)
    xt, nx, ldx = _table(x if batch_x else None, D, "x", who, dev)
    yt, ny, ldy = _table(y if batch_y else None, D, "y", who, dev)
    idx_x = _index(idx_x, n_steps * batch_x, "idx_x", who, dev) if batch_x else None
    idx_y = _index(idx_y, n_steps * batch_y, "idx_y", who, dev) if batch_y else None
    if (batch_x and idx_x is None and batch_x > nx) or (batch_y and idx_y is None and batch_y > ny):
        raise ValueError(f"{who}: a batch without row ids takes the table's first rows and cannot be longer than the table")
    cfg = AeCfg(D, C_, L)
    scratch, nbytes = _scratch(dev, cfg, batch_x, batch_y, 1)
    if losses is None:
        losses = torch.empty((max(n_steps, 0), 3), dtype=torch.float32, device=dev)
    elif tuple(losses.shape) != (n_steps, 3) or losses.dtype != torch.float32 or losses.device != dev or not losses.is_contiguous():
        raise ValueError(f"{who}: losses must be a contiguous fp32 [{n_steps}, 3] tensor on {dev}")
    check(load_library().umlh_ae_train_steps(
        C.byref(cfg), glue.ptr_array(params), glue.ptr_array(m), None if v is None else glue.ptr_array(v), glue.ptr(xt), ldx,
        glue.ptr(idx_x), batch_x, glue.ptr(yt), ldy, glue.ptr(idx_y), batch_y, n_steps, 1 if mode == "xy" else 0, float(alpha_x),
        float(alpha_y), OPT_IDS[optimizer], float(lr), int(first_step), float(betas[0]), float(betas[1]), float(eps), float(momentum),
        float(weight_decay), losses.data_ptr(), scratch.data_ptr(), nbytes, glue.stream(dev)), "umlh_ae_train_steps")
    return losses
