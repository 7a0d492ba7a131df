"""GPU: the bf16 step against float64, BIT FOR BIT, on the exactly representable operands of tests/_bf16_exact_ref.py.

Every rounding the bf16 step performs (features, W_head, W_proj, H, dZ, dH to bf16) is the identity on these operands and every
fp32 accumulation is exact in any order, so the float64 gradient cast to fp32 is the only correct answer: all elements of
dW_head and dW_proj, and of the weights after one plain SGD step, are compared as uint32 words, under every launch form of the
step.  The accuracies are exact as well (first-arg-max hits / global_rows with global_rows = 2^15); only the two losses carry
a tolerance, 1e-5 * max(1, |loss|) as for the fused decoder loss: one __logf per row is the only inexact operation left
(each case prints its loss errors; observed on MI355X: 9.5e-7 at the most, typically 1e-7).

Every case drives the public engine (umlh.HeadEngine grad_step / train_step / apply_update) as tests/test_bf16_gpu.py does."""
import functools

import numpy as np
import pytest
import torch

import _bf16_exact_ref as R
from _switches import monkeypatch_engine_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# environment of each launch form (read by the engine when it is created)
VARIANTS = {
    "fuse0": {"UMLH_BF16_FUSE": "0"},                                  # launch per kernel
    "stw2": {"UMLH_BF16_FUSE": "0", "UMLH_BF16_STW": "2"},             # two sample tiles per wave of the 1-D forward
    "fwd2d": {"UMLH_BF16_FUSE": "0", "UMLH_BF16_FWD2D": "1"},          # the 2-D forward
    "fuse1": {"UMLH_BF16_FUSE": "1"},                                  # forward + dW as one launch
    "fuse2": {"UMLH_BF16_FUSE": "2"},                                  # the one-launch step
    "fuse2_grid7": {"UMLH_BF16_FUSE": "2", "UMLH_STEP_GRID": "7"},     # ... on 7 workgroups
}
_ALWAYS = ["fuse0", "fuse1", "fuse2", "fuse2_grid7"]


def _variants(s):
    v = list(_ALWAYS)
    # UMLH_BF16_STW=2 is ignored unless the forward runs 8 waves along the classes with at least two 32-class tiles each
    # (C > 256): removed from the shapes with 2, 37, 64 and 200 classes
    if s.C > 256:
        v.insert(1, "stw2")
    # UMLH_BF16_FWD2D=1 is ignored unless C > 256, d % 256 == 0 and d <= 512: removed from the shapes above and from d = 1024
    if s.C > 256 and s.d % 256 == 0 and s.d <= 512:
        v.insert(2, "fwd2d")
    return v


SINGLE_CASES = [(s, v) for s in R.SINGLE_SHAPES for v in _variants(s)] + [(s, v) for s in R.DENSE_SHAPES for v in ("fuse0", "fuse2")]
# the two-layer head always takes the launch-per-kernel form (the engine ignores UMLH_BF16_FUSE for it: the one-launch step is the
# linear head's); both settings are run all the same, so a fused form for it, once there is one, is covered from its first day
DOUBLE_CASES = [(s, v) for s in R.DOUBLE_SHAPES for v in ("fuse0", "fuse2")]
_ids = lambda v: v if isinstance(v, str) else v.id


@functools.lru_cache(maxsize=None)
def _device_tables(s):
    """The two tables of a shape on the device (fp32, labels, bf16 shadow, row ids), uploaded once for all its variants."""
    import umlh
    case, _ = R.case_and_reference(s)
    T = lambda a, t: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV, t).contiguous()
    out = []
    for x, y, idx in ((case.xi, case.yi, case.ii), (case.xt, case.yt, case.ti)):
        f = T(x, torch.float32)
        out.append((f, T(y, torch.int64), T(idx, torch.int64), umlh.to_bf16(f)))
    return out


def _batches(s):
    import umlh
    (fi, yi, ii, fi16), (ft, yt, ti, ft16) = _device_tables(s)
    bi = umlh.RowBatch(fi, yi, ii, rows=s.ri, global_rows=R.G, feats_bf16=fi16) if s.ri else None
    bt = umlh.RowBatch(ft, yt, ti, rows=s.rt, global_rows=R.G, feats_bf16=ft16) if s.rt else None
    return bi, bt


def _engine(s, env, monkeypatch):
    import umlh
    monkeypatch_engine_env(monkeypatch, env)
    case, _ = R.case_and_reference(s)
    e = umlh.HeadEngine(s.d_img, s.d, s.C, has_proj=s.two_layer, optimizer="sgd", momentum=0.0, weight_decay=0.0,
                        max_rows_img=s.cap, max_rows_txt=512, precision="bf16", device=DEV)
    e.w_head.copy_(torch.from_numpy(case.w_head))
    if s.two_layer:
        e.w_proj.copy_(torch.from_numpy(case.w_proj))
    e.scales.fill_(s.scale)
    return e


def _assert_bits(name, got, want):
    n, first = R.mismatches(got, want)
    assert n == 0, f"{name}: {n} of {want.size} elements differ; first (row, column, got, want): {first}"


def _assert_scalars(s, sc, ref):
    import umlh
    for rows, acc, loss, want_acc, want_loss in ((s.ri, umlh.S_ACC_IMG, umlh.S_LOSS_IMG, ref.acc_img, ref.loss_img),
                                                 (s.rt, umlh.S_ACC_TXT, umlh.S_LOSS_TXT, ref.acc_txt, ref.loss_txt)):
        if rows == 0:
            continue
        print(f"loss error {abs(float(sc[loss]) - want_loss):.3e} of {want_loss:.6f}; hits {float(sc[acc]) * R.G:.0f} of {rows}")
        assert np.float32(sc[acc]).view(np.uint32) == np.float32(want_acc).view(np.uint32), (float(sc[acc]) * R.G, float(want_acc) * R.G)
        assert abs(float(sc[loss]) - want_loss) <= 1e-5 * max(1.0, abs(want_loss)), (float(sc[loss]), want_loss)


def _grad_case(s, variant, monkeypatch):
    case, ref = R.case_and_reference(s)
    e = _engine(s, VARIANTS[variant], monkeypatch)
    bi, bt = _batches(s)
    flat = e.grad_step(bi, bt, alpha=R.ALPHA, img_alpha=R.IMG_ALPHA)
    torch.cuda.synchronize()
    assert e.step_status() == (0, 0, 0, 0)
    assert (e.step_launches() > 0) == (variant.startswith(("fuse1", "fuse2")) and not s.two_layer)      # the form asked for ran
    f = flat.cpu().numpy()
    nh, npj = s.C * s.d, (s.d * s.d_img if s.two_layer else 0)
    assert f.size == nh + npj + 2 + 12
    _assert_bits("dW_head", f[:nh].reshape(s.C, s.d), ref.g_head)
    if s.two_layer:
        _assert_bits("dW_proj", f[nh:nh + npj].reshape(s.d, s.d_img), ref.g_proj)
    _assert_scalars(s, f[nh + npj + 2:], ref)


@pytest.mark.parametrize("shape,variant", SINGLE_CASES, ids=_ids)
def test_bf16_exact_single_layer_gradient(shape, variant, monkeypatch):
    """dW_head of the linear head, all C x d elements as bits, gathered rows (with duplicates) or dense ones, ragged row counts,
    partial class tiles, live classes only in the second class tile, negative scale, several split-K slabs."""
    _grad_case(shape, variant, monkeypatch)


@pytest.mark.parametrize("shape,variant", DOUBLE_CASES, ids=_ids)
def test_bf16_exact_two_layer_gradients(shape, variant, monkeypatch):
    """dW_head and dW_proj of the two-layer head: H = X W_proj^T and dH = dZ W_head are bf16 numbers, dH is row dependent."""
    _grad_case(shape, variant, monkeypatch)


@pytest.mark.parametrize("path", ["train_step", "grad_then_update"])
@pytest.mark.parametrize("shape", R.UPDATE_SHAPES, ids=_ids)
def test_bf16_exact_sgd_step(shape, path, monkeypatch):
    """One plain SGD step (momentum 0, no decay, lr = 2^-3): W - lr g is exact, so the weights are compared as bits; through
    the fused step (the one-launch step for the linear heads) and through grad_step + apply_update."""
    import umlh
    s = shape
    case, ref = R.case_and_reference(s)
    e = _engine(s, {}, monkeypatch)
    bi, bt = _batches(s)
    sc = torch.zeros(umlh.N_SCALARS, device=DEV)
    if path == "train_step":
        e.train_step(bi, bt, lr=R.LR, step=1, alpha=R.ALPHA, img_alpha=R.IMG_ALPHA, scalars_out=sc)
    else:
        e.grad_step(bi, bt, alpha=R.ALPHA, img_alpha=R.IMG_ALPHA)
        e.apply_update(lr=R.LR, step=1, scalars_out=sc, alpha=R.ALPHA, img_alpha=R.IMG_ALPHA)
    torch.cuda.synchronize()
    assert e.step_status() == (0, 0, 0, 0)
    assert (e.step_launches() > 0) == (not s.two_layer)
    _assert_bits("w_head", e.w_head.cpu().numpy(), ref.w_head_new)
    if s.two_layer:
        _assert_bits("w_proj", e.w_proj.cpu().numpy(), ref.w_proj_new)
    _assert_scalars(s, sc.cpu().numpy(), ref)
