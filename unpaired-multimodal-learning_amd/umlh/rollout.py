"""The autoregressive rollout of the MultiBench model and the spectral-bias spectra on the HIP kernels of
umlh_kernels_rollout.hip (C ABI: ``umlh_rollout``, ``umlh_seq_spectrum``; reference MultiBench/train.py:245-292).

``rollout_rows`` walks every step of every row in ONE launch: at T = 1 the causal softmax over a single key is exactly 1, a
layer's attention is ``out_proj(v_proj(h))`` and rows never meet.  ``seq_spectrum`` is
``torch.abs(torch.fft.rfft(x, dim=1)).mean(dim=(0, 2))`` as a direct fp64 DFT in two launches.  Both enqueue on
``torch.cuda.current_stream`` and return device tensors; nothing is read back.  There is no CPU compute path."""
from __future__ import annotations

import ctypes as C

import torch

from . import _glue as glue
from ._lib import RolloutCfg, check, load_library

N_LAYER_PARAMS = 12   # in_w, in_b, out_w, out_b, w1, b1, w2, b2, g1, be1, g2, be2 (umlh_encoder_layer_forward's order)


def _dense(t, shape, what, dev):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        raise ValueError(f"rollout_rows: {what} must be a tensor of shape {tuple(shape)}, got {getattr(t, 'shape', type(t))}")
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def rollout_rows(x0, w_in, b_in, conv_w, pos0, layer_params, eps, w_out, b_out, steps, out=None):
    """``[n, steps + 1, D]``: row r's seed ``x0[r]`` followed by ``steps`` generated frames,

        h = conv_w (w_in cur + b_in) + pos0;  per layer: h = LN1(h + W_o (W_v h + b_v) + b_o), h = LN2(h + W_2 relu(W_1 h + b_1) + b_2);
        cur = w_out h + b_out

    ``x0`` [n, D] (row stride >= D is used in place); ``w_in`` [Z, D], ``b_in`` [Z]; ``conv_w`` None or [Z, Z] (a Conv1d's
    [Z, Z, 1] weight is accepted); ``pos0`` None or [Z], row 0 of the position table; ``layer_params`` 12 tensors per layer
    in the order of ``multibench.encoder.layer_params``; ``w_out`` [D, Z], ``b_out`` [D].  ``out``: an fp32 device view
    [n, steps + 1, D] with unit column stride to write into.  A row's values do not depend on n or on its index."""
    if not isinstance(x0, torch.Tensor) or x0.ndim != 2 or not x0.is_floating_point():
        raise ValueError(f"rollout_rows: x0 must be a floating-point [n, D] tensor, got {getattr(x0, 'shape', type(x0))}")
    n, D = x0.shape
    steps = int(steps)
    if n < 1 or D < 1:
        raise ValueError(f"rollout_rows: empty seed {tuple(x0.shape)}")
    if steps < 0:
        raise ValueError(f"rollout_rows: steps={steps} < 0")
    lp = list(layer_params)
    if len(lp) % N_LAYER_PARAMS:
        raise ValueError(f"rollout_rows: {len(lp)} layer tensors (need {N_LAYER_PARAMS} per layer)")
    n_layers = len(lp) // N_LAYER_PARAMS
    if not isinstance(w_in, torch.Tensor) or w_in.ndim != 2 or w_in.shape[1] != D:
        raise ValueError(f"rollout_rows: w_in must be [Z, {D}], got {getattr(w_in, 'shape', type(w_in))}")
    Z = w_in.shape[0]
    dev = glue.device("umlh.rollout", "the rollout runs only on its HIP kernel")
    w_in, b_in = _dense(w_in, (Z, D), "w_in", dev), _dense(b_in, (Z,), "b_in", dev)
    w_out, b_out = _dense(w_out, (D, Z), "w_out", dev), _dense(b_out, (D,), "b_out", dev)
    if conv_w is not None:
        if conv_w.ndim == 3 and conv_w.shape[2] == 1:
            conv_w = conv_w[:, :, 0]
        conv_w = _dense(conv_w, (Z, Z), "conv_w", dev)
    if pos0 is not None:
        pos0 = _dense(pos0, (Z,), "pos0", dev)
    dff = lp[4].shape[0] if n_layers else 1
    shapes = [(3 * Z, Z), (3 * Z,), (Z, Z), (Z,), (dff, Z), (dff,), (Z, dff), (Z,), (Z,), (Z,), (Z,), (Z,)]
    lp = [_dense(t, shapes[i % N_LAYER_PARAMS], f"layer_params[{i}]", dev) for i, t in enumerate(lp)]
    xv = x0.detach().to(device=dev, dtype=torch.float32)
    if xv.stride(1) != 1 or (n > 1 and xv.stride(0) < D):
        xv = xv.contiguous()
    if out is None:
        out = torch.empty((n, steps + 1, D), dtype=torch.float32, device=dev)
    elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != (n, steps + 1, D) or out.dtype != torch.float32
          or out.device != dev or out.stride(2) != 1):
        raise ValueError(f"rollout_rows: out must be an fp32 view [{n}, {steps + 1}, {D}] on {dev} with unit column stride")
    cfg = RolloutCfg(Z, dff, D, n_layers, steps, float(eps))
    P = glue.ptr_array(lp) if lp else None
    ldx = xv.stride(0) if n > 1 else D                    # the stride of a dimension of size 1 means nothing
    ldt = out.stride(1) if steps > 0 else D
    ldb = out.stride(0) if n > 1 else steps * ldt + D
    check(load_library().umlh_rollout(C.byref(cfg), P, glue.ptr(conv_w), glue.ptr(pos0), glue.ptr(w_in), glue.ptr(b_in),
                                      glue.ptr(w_out), glue.ptr(b_out), xv.data_ptr(), ldx, n, out.data_ptr(), ldb, ldt,
                                      glue.stream(dev)), "umlh_rollout")
    return out


def seq_spectrum(x: torch.Tensor) -> torch.Tensor:
    """``torch.abs(torch.fft.rfft(x, dim=1)).mean(dim=(0, 2))`` of a [B, T, d] block: a float64 device tensor [T // 2 + 1].
    ``x`` is read through its strides (a copy is made only when the last stride is not 1).  1 <= T <= 1024, B <= 2^20."""
    if not isinstance(x, torch.Tensor) or x.ndim != 3:
        raise ValueError(f"seq_spectrum: expected a 3-D tensor [B, T, d], got {getattr(x, 'shape', type(x))}")
    if not x.is_floating_point():
        raise ValueError(f"seq_spectrum: expected a floating-point tensor, got {x.dtype}")
    B, T, d = x.shape
    if B < 1 or T < 1 or d < 1:
        raise ValueError(f"seq_spectrum: empty input {tuple(x.shape)}")
    dev = glue.device("umlh.rollout", "the spectrum is summed only by HIP kernels")
    xv = x.detach().to(device=dev, dtype=torch.float32)
    if xv.stride(2) != 1:
        xv = xv.contiguous()
    scratch, nbytes = glue.scratch("umlh_seq_spectrum_scratch_bytes", dev, b=B, t_len=T, d=d)
    out = torch.empty(T // 2 + 1, dtype=torch.float64, device=dev)
    check(load_library().umlh_seq_spectrum(xv.data_ptr(), xv.stride(0), xv.stride(1), B, T, d, out.data_ptr(), scratch.data_ptr(),
                                           nbytes, glue.stream(dev)), "umlh_seq_spectrum")
    return out
