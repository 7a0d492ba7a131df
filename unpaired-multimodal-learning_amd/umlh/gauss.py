"""The Gaussian toy's SharedAutoencoder on the HIP kernels of umlh_kernels_gauss.hip (C ABI: ``umlh_ae_forward``,
``umlh_ae_train_steps``; reference Gaussian_experiment/model.py:5-59, main.py:33-91).

``ae_forward`` is the evaluation forward of either or both views in one call; ``ae_train_steps`` runs whole training steps
(both views, forward, MSE, backward, optimizer update) as two launches each, with the batches gathered by index from
device-resident tables.  Both enqueue on ``torch.cuda.current_stream`` and return device tensors; nothing is read back.  The
parameter and moment tensors are updated in place through their own storages.  There is no CPU compute path.

``ae_train_steps_grouped`` and ``ae_forward_grouped`` run up to 64 independent runs (members) in one launch pair per step (C ABI:
``umlh_ae_train_steps_grouped``, ``umlh_ae_forward_grouped``).  A member is the keyword arguments of the single-run function, checked
by the same code, and its results are bit for bit those of the single-run call."""
from __future__ import annotations

import ctypes as C

import torch

from . import _glue as glue
from ._lib import AE_MAX_GROUP, OPT_IDS, AeCfg, AeEvalItem, AeGroupItem, UmlhError, check, load_library

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


def _forward_member(who, dev, params, x=None, y=None, idx_x=None, idx_y=None, losses=True, recon=True, embeddings=True):
    """The checked arguments and fresh outputs of one evaluation forward: what ``ae_forward`` and a member of ``ae_forward_grouped`` share."""
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
    new = lambda on, n, w: torch.empty((n, w), dtype=torch.float32, device=dev) if on and n else None
    out_l = torch.empty(2, dtype=torch.float32, device=dev) if losses else None
    out = (out_l, new(recon, nx, D), new(recon, ny, D), new(embeddings, nx, L), new(embeddings, ny, L))
    return dict(cfg=AeCfg(D, C_, L), params=params, x=xt, ldx=ldx, idx_x=idx_x, nx=nx, y=yt, ldy=ldy, idx_y=idx_y, ny=ny, out=out)


def ae_forward(params, x=None, y=None, idx_x=None, idx_y=None, losses=True, recon=True, embeddings=True):
    """``(losses, rec_x, rec_y, emb_x, emb_y)`` of the evaluation forward.  ``params``: the 16 tensors in ``state_dict`` order.
    ``x`` / ``y``: fp32 device tables [n, D] (a row stride >= D is read in place) or None (view absent; at least one).
    ``idx_x`` / ``idx_y``: optional int32 device row ids: the view's rows are ``table[idx]``.  ``losses``: a float32 device
    tensor [2] = (loss_x, loss_y), 0 for an absent view; an output that is switched off is None."""
    who = "umlh.gauss.ae_forward"
    dev = glue.device("umlh.gauss", "the autoencoder runs only on its HIP kernels")
    a = _forward_member(who, dev, params, x, y, idx_x, idx_y, losses, recon, embeddings)
    cfg = a["cfg"]
    scratch, nbytes = _scratch(dev, cfg, a["nx"], a["ny"], 0)
    out_l, rec_x, rec_y, emb_x, emb_y = a["out"]
    check(load_library().umlh_ae_forward(C.byref(cfg), glue.ptr_array(a["params"]), glue.ptr(a["x"]), a["ldx"], glue.ptr(a["idx_x"]), a["nx"],
                                         glue.ptr(a["y"]), a["ldy"], glue.ptr(a["idx_y"]), a["ny"], glue.ptr(out_l), glue.ptr(rec_x),
                                         glue.ptr(rec_y), glue.ptr(emb_x), glue.ptr(emb_y), scratch.data_ptr(), nbytes, glue.stream(dev)),
          "umlh_ae_forward")
    return a["out"]


def _mode_and_optimizer(who, mode="xy", optimizer="adam", **_):
    """The two value checks that need no GPU; they come before the device is asked for."""
    if mode not in ("xy", "x"):
        raise ValueError(f"{who}: mode={mode!r} (expected 'xy' or 'x')")
    if optimizer not in OPT_IDS:
        raise ValueError(f"{who}: optimizer={optimizer!r} (expected one of {sorted(OPT_IDS)})")


def _train_member(who, dev, n_steps, params, m, v, x, y, idx_x, idx_y, batch_x, batch_y, *, mode="xy", alpha_x=1.0, alpha_y=1.0,
                  optimizer="adam", lr=1e-3, first_step=1, betas=(0.9, 0.999), eps=1e-8, momentum=0.9, weight_decay=0.0, losses=None):
    """The checked arguments of ``n_steps`` training steps of one run: what ``ae_train_steps`` and a member of
    ``ae_train_steps_grouped`` share (``_mode_and_optimizer`` has run)."""
    params, D, C_, L = _dims(params, who)
    shapes = tensor_shapes(D, C_, L)
    params = _bound(params, shapes, "params", who, dev)
    m = _bound(list(m), shapes, "m", who, dev)
    if v is None and optimizer != "sgd":
        raise ValueError(f"{who}: v is required under {optimizer}")
    v = None if v is None else _bound(list(v), shapes, "v", who, dev)
    batch_x, batch_y = int(batch_x), int(batch_y)
    xt, nx, ldx = _table(x if batch_x else None, D, "x", who, dev)
    yt, ny, ldy = _table(y if batch_y else None, D, "y", who, dev)
    idx_x = _index(idx_x, n_steps * batch_x, "idx_x", who, dev) if batch_x else None
    idx_y = _index(idx_y, n_steps * batch_y, "idx_y", who, dev) if batch_y else None
    if (batch_x and idx_x is None and batch_x > nx) or (batch_y and idx_y is None and batch_y > ny):
        raise ValueError(f"{who}: a batch without row ids takes the table's first rows and cannot be longer than the table")
    if losses is None:
        losses = torch.empty((max(n_steps, 0), 3), dtype=torch.float32, device=dev)
    elif tuple(losses.shape) != (n_steps, 3) or losses.dtype != torch.float32 or losses.device != dev or not losses.is_contiguous():
        raise ValueError(f"{who}: losses must be a contiguous fp32 [{n_steps}, 3] tensor on {dev}")
    return dict(cfg=AeCfg(D, C_, L), params=params, m=m, v=v, x=xt, ldx=ldx, idx_x=idx_x, batch_x=batch_x, y=yt, ldy=ldy, idx_y=idx_y,
                batch_y=batch_y, backward_y=1 if mode == "xy" else 0, alpha_x=float(alpha_x), alpha_y=float(alpha_y),
                optimizer=OPT_IDS[optimizer], lr=float(lr), first_step=int(first_step), beta1=float(betas[0]), beta2=float(betas[1]),
                eps=float(eps), momentum=float(momentum), weight_decay=float(weight_decay), losses=losses)


def ae_train_steps(params, m, v, x, y, idx_x, idx_y, batch_x, batch_y, n_steps, *, mode="xy", alpha_x=1.0, alpha_y=1.0,
                   optimizer="adam", lr=1e-3, first_step=1, betas=(0.9, 0.999), eps=1e-8, momentum=0.9, weight_decay=0.0,
                   losses=None):
    """``n_steps`` fused training steps; returns the float32 device tensor [n_steps, 3] of (loss_x, loss_y, loss) per step.
    ``params``, ``m``, ``v``: 16 tensors each in ``state_dict`` order, UPDATED IN PLACE (``v`` may be None under sgd).  ``x`` /
    ``y``: fp32 device tables [n, D]; ``idx_x`` / ``idx_y``: int32 device row ids, ``n_steps * batch`` of them: step s takes
    ``idx[s * batch : (s + 1) * batch]``.  The ids are used as addresses unchecked: the caller guarantees ``0 <= id < n``.
    ``mode='x'``: the y view runs forward only and ``in_head_y`` / ``out_head_y`` and their moments are not touched."""
    who = "umlh.gauss.ae_train_steps"
    n_steps = int(n_steps)
    _mode_and_optimizer(who, mode, optimizer)
    dev = glue.device("umlh.gauss", "the autoencoder runs only on its HIP kernels")
    a = _train_member(who, dev, n_steps, params, m, v, x, y, idx_x, idx_y, batch_x, batch_y, mode=mode, alpha_x=alpha_x, alpha_y=alpha_y,
                      optimizer=optimizer, lr=lr, first_step=first_step, betas=betas, eps=eps, momentum=momentum,
                      weight_decay=weight_decay, losses=losses)
    cfg = a["cfg"]
    scratch, nbytes = _scratch(dev, cfg, a["batch_x"], a["batch_y"], 1)
    check(load_library().umlh_ae_train_steps(
        C.byref(cfg), glue.ptr_array(a["params"]), glue.ptr_array(a["m"]), None if a["v"] is None else glue.ptr_array(a["v"]),
        glue.ptr(a["x"]), a["ldx"], glue.ptr(a["idx_x"]), a["batch_x"], glue.ptr(a["y"]), a["ldy"], glue.ptr(a["idx_y"]), a["batch_y"],
        n_steps, a["backward_y"], a["alpha_x"], a["alpha_y"], a["optimizer"], a["lr"], a["first_step"], a["beta1"], a["beta2"], a["eps"],
        a["momentum"], a["weight_decay"], a["losses"].data_ptr(), scratch.data_ptr(), nbytes, glue.stream(dev)), "umlh_ae_train_steps")
    return a["losses"]


def _raw(t):
    return None if t is None else t.data_ptr()


def _group_scratch(dev, kind, items, n, n_steps, signature):
    """Scratch of a grouped call, leased per (device, stream, group signature): the members' shapes in order and the step count."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, kind, n_steps) + signature
    hit = _SCRATCH.get(key)
    if hit is None:
        lib = load_library()
        nbytes = lib.umlh_ae_group_scratch(items, n, n_steps) if kind == "train" else lib.umlh_ae_eval_group_scratch(items, n)
        if nbytes == 0:
            raise UmlhError(f"umlh_ae_{'group' if kind == 'train' else 'eval_group'}_scratch: invalid arguments n_items={n} "
                            f"n_steps={n_steps} members={signature}")
        if len(_SCRATCH) >= 16:
            _SCRATCH.clear()
        hit = _SCRATCH[key] = (torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes)
    return hit


def _members(members, who):
    members = list(members)
    if not 1 <= len(members) <= AE_MAX_GROUP:
        raise ValueError(f"{who}: {len(members)} members (expected 1..{AE_MAX_GROUP})")
    return members


def ae_train_steps_grouped(members, n_steps):
    """``n_steps`` fused training steps of every member in two launches per step, whatever the number of members.  ``members``:
    1..64 dicts of the arguments of ``ae_train_steps`` (``n_steps`` excepted), checked as that function checks them.  Members
    may differ in everything, shapes included, and may share tables and row ids; they may not share parameter or moment tensors.
    Returns the members' [n_steps, 3] loss tensors.  Per member the result is bit for bit that of ``ae_train_steps``."""
    who = "umlh.gauss.ae_train_steps_grouped"
    members, n_steps = _members(members, who), int(n_steps)
    for i, mb in enumerate(members):
        _mode_and_optimizer(f"{who}: member {i}", **mb)
    dev = glue.device("umlh.gauss", "the autoencoder runs only on its HIP kernels")
    args = [_train_member(f"{who}: member {i}", dev, n_steps, **mb) for i, mb in enumerate(members)]
    items = (AeGroupItem * len(args))()
    keep = []
    for it, a in zip(items, args):
        arrays = [glue.ptr_array(a["params"]), glue.ptr_array(a["m"]), None if a["v"] is None else glue.ptr_array(a["v"])]
        keep.append(arrays)
        it.cfg = a["cfg"]
        it.P, it.M = C.cast(arrays[0], C.POINTER(C.c_void_p)), C.cast(arrays[1], C.POINTER(C.c_void_p))
        it.V = C.cast(arrays[2], C.POINTER(C.c_void_p)) if arrays[2] is not None else None
        it.x, it.ldx, it.idx_x, it.batch_x = _raw(a["x"]), a["ldx"], _raw(a["idx_x"]), a["batch_x"]
        it.y, it.ldy, it.idx_y, it.batch_y = _raw(a["y"]), a["ldy"], _raw(a["idx_y"]), a["batch_y"]
        for k in ("backward_y", "alpha_x", "alpha_y", "optimizer", "lr", "first_step", "beta1", "beta2", "eps", "momentum", "weight_decay"):
            setattr(it, k, a[k])
        it.losses = a["losses"].data_ptr()
    sig = tuple((a["cfg"].dim_obs, a["cfg"].dim_common, a["cfg"].dim_latent, a["batch_x"], a["batch_y"]) for a in args)
    scratch, nbytes = _group_scratch(dev, "train", items, len(args), n_steps, sig)
    check(load_library().umlh_ae_train_steps_grouped(items, len(args), n_steps, scratch.data_ptr(), nbytes, glue.stream(dev)),
          "umlh_ae_train_steps_grouped")
    return [a["losses"] for a in args]


def ae_forward_grouped(members):
    """One evaluation forward of every member in one launch (one more for the losses).  ``members``: 1..64 dicts of the arguments
    of ``ae_forward``; members may share tables.  Returns the members' ``(losses, rec_x, rec_y, emb_x, emb_y)`` tuples, each bit
    for bit what ``ae_forward`` returns for that member."""
    who = "umlh.gauss.ae_forward_grouped"
    members = _members(members, who)
    dev = glue.device("umlh.gauss", "the autoencoder runs only on its HIP kernels")
    args = [_forward_member(f"{who}: member {i}", dev, **mb) for i, mb in enumerate(members)]
    items = (AeEvalItem * len(args))()
    keep = []
    for it, a in zip(items, args):
        arr = glue.ptr_array(a["params"])
        keep.append(arr)
        it.cfg, it.P = a["cfg"], C.cast(arr, C.POINTER(C.c_void_p))
        it.x, it.ldx, it.idx_x, it.n_x = _raw(a["x"]), a["ldx"], _raw(a["idx_x"]), a["nx"]
        it.y, it.ldy, it.idx_y, it.n_y = _raw(a["y"]), a["ldy"], _raw(a["idx_y"]), a["ny"]
        it.losses, it.rec_x, it.rec_y, it.emb_x, it.emb_y = (_raw(t) for t in a["out"])
    sig = tuple((a["cfg"].dim_obs, a["cfg"].dim_common, a["cfg"].dim_latent, a["nx"], a["ny"]) for a in args)
    scratch, nbytes = _group_scratch(dev, "eval", items, len(args), 0, sig)
    check(load_library().umlh_ae_forward_grouped(items, len(args), scratch.data_ptr(), nbytes, glue.stream(dev)), "umlh_ae_forward_grouped")
    return [a["out"] for a in args]
