"""GPU: the split-K slab sum of the head update (step_update_task through slab_sum in csrc/umlh_common.h, head_step_kernel,
reduce_update).  The documented order -- image slabs from 0.0 in ascending index, text slabs from 0.0 in ascending index,
then image + text -- is checked BIT for BIT on operands whose slab partials are exact in fp32, so the expected gradient is
a pure CPU computation; then the one-launch step is run with a narrow grid and with lazy workgroups (whoever needs a dW
tile takes it) against the launch-per-kernel step."""
import numpy as np
import pytest
import torch

from _switches import monkeypatch_engine_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

D, C = 128, 64                 # one 128 x 128 output tile: the slab capacity is 64 (split_cap, umlh_api.cpp)
GLOBAL_ROWS = 1 << 15          # CE-mean denominator: a power of two, so scale / rows is exact
SCALE, LR = 64.0, 2.0 ** -3
DZ = SCALE / GLOBAL_ROWS / C   # d loss / d logit of a class that is nobody's label: softmax 1/64 exactly (w_head = 0)
COUNTS = [(1, 1), (2, 1), (7, 1), (8, 1), (8, 8), (17, 3), (63, 1), (5, 0), (0, 3)]   # 256-row slabs (image, text) of a bf16 engine


def _plan_splits(r0, r1, want, quantum, min_chunk):
    """plan_splits of csrc/umlh_api.cpp restated: (chunk, n_img, n_txt).  bf16_dw_head calls it with (64, 256, 256) here,
    f32_dw_head with (64, 16, 64); the padded row counts are the row counts (multiples of 256)."""
    tot = r0 + r1
    s0 = (want * r0 + tot // 2) // tot if r0 > 0 else 0
    if r0 > 0 and s0 < 1: s0 = 1
    if r1 > 0 and s0 > want - 1: s0 = want - 1
    s1 = want - s0 if r1 > 0 else 0
    if r1 > 0 and s1 < 1: s1 = 1
    c0 = (r0 + s0 - 1) // s0 if s0 > 0 else 0
    c1 = (r1 + s1 - 1) // s1 if s1 > 0 else 0
    chunk = max(-(-max(c0, c1) // quantum) * quantum, min_chunk)
    return chunk, -(-r0 // chunk), -(-r1 // chunk)


def _slab_rows(rows, chunk):
    return [(a, min(a + chunk, rows)) for a in range(0, rows, chunk)]


def _operands(r0, r1, plan, seed):
    """Feature rows = small integers (|x| <= 7) times +-2^a(s), s = the slab the row falls in under `plan`: a(s) is 0 on
    even slabs and 24 on odd ones with the sign alternating every two slabs, so the fp32 sum over slabs depends on the
    order of the additions and on every slab being there.  Labels in classes 0..31 only."""
    rng = np.random.default_rng(seed)
    chunk, n_img, n_txt = plan
    out, s = [], 0
    for rows in (r0, r1):
        x = rng.integers(-7, 8, (rows, D)).astype(np.float32)
        for a, b in _slab_rows(rows, chunk):
            x[a:b] *= np.float32((2.0 ** 24 if s & 1 else 1.0) * (-1.0 if s & 2 else 1.0))
            s += 1
        out.append((x, rng.integers(0, 32, rows)))
    assert s == n_img + n_txt
    return out


def _expected(ops, plan):
    """Rows [32, 64) of dW (they are equal: no label falls there) by the documented order in np.float32, and all of dW
    in float64."""
    chunk = plan[0]
    sums = []
    for x, _ in ops:
        acc = np.zeros(D, np.float32)
        for a, b in _slab_rows(len(x), chunk):
            part = DZ * x[a:b].astype(np.float64).sum(0)
            assert np.array_equal(part, part.astype(np.float32).astype(np.float64))   # every slab partial is exact in fp32
            acc = acc + part.astype(np.float32)
        sums.append(acc)
    g = sums[0] + sums[1]
    assert g.dtype == np.float32
    g64 = np.zeros((C, D))
    for x, y in ops:
        if len(x):
            p = np.full((len(x), C), 1.0 / C)
            p[np.arange(len(x)), y] -= 1.0
            g64 += (SCALE / GLOBAL_ROWS) * (p.T @ x.astype(np.float64))
    return g, g64


def _batch(x, y):
    import umlh
    if len(x) == 0:
        return None
    f = torch.from_numpy(x).to(DEV).contiguous()
    return umlh.RowBatch(f, torch.from_numpy(y).to(DEV), None, global_rows=GLOBAL_ROWS)


def _one_sgd_step(precision, ops, split):
    """w after ONE plain SGD step (no momentum, no weight decay) from w = 0: -lr * gradient, exactly (lr = 2^-3)."""
    import umlh
    cap = max(256, max(len(x) for x, _ in ops))
    e = umlh.HeadEngine(D, D, C, optimizer="sgd", momentum=0.0, weight_decay=0.0, max_rows_img=cap, max_rows_txt=cap,
                        precision=precision, device=DEV)
    e.scales.fill_(SCALE)
    bi, bt = _batch(*ops[0]), _batch(*ops[1])
    if split:
        e.grad_step(bi, bt)
        e.apply_update(lr=LR, step=1)
    else:
        e.train_step(bi, bt, lr=LR, step=1)
    torch.cuda.synchronize()
    assert e.step_status() == (0, 0, 0, 0)
    return e.w_head.cpu().numpy(), e.step_launches()


@pytest.mark.parametrize("path", ["launch_per_kernel", "one_launch", "grad_then_update", "fp32"])
@pytest.mark.parametrize("n_img,n_txt", COUNTS)
def test_slab_sum_order_bit_for_bit_on_exact_partials(n_img, n_txt, path, monkeypatch):
    """Slab counts on both sides of the group of 8 loads (1+1 ... 63+1, image only, text only).  The fp32 engine plans its
    own split of the same row counts (16-row quantum, 64-row minimum: 4+4, 8+4, 28+4, 32+4, 32+32, 46+8 with a short last
    image slab, 63+1, 20+0, 0+12), restated here as well."""
    monkeypatch_engine_env(monkeypatch, {"UMLH_BF16_FUSE": "0" if path == "launch_per_kernel" else "2"})
    r0, r1 = 256 * n_img, 256 * n_txt
    plan = _plan_splits(r0, r1, 64, 16, 64) if path == "fp32" else _plan_splits(r0, r1, 64, 256, 256)
    if path != "fp32":
        assert plan == (256, n_img, n_txt)
    ops = _operands(r0, r1, plan, 1000 * n_img + n_txt)
    want, want64 = _expected(ops, plan)
    w, launches = _one_sgd_step("fp32" if path == "fp32" else "bf16", ops, path == "grad_then_update")
    assert (launches > 0) == (path in ("one_launch", "grad_then_update"))
    # the optimizer's own recurrence on the expected gradient (m = 0 * 0 + g, w = 0 - lr * m: a zero comes out as +0.0)
    want_w = np.float32(0.0) - np.float32(LR) * (np.float32(0.0) * np.float32(0.0) + want)
    assert want_w.dtype == np.float32
    bad = np.argwhere(w[32:].view(np.uint32) != want_w.view(np.uint32)[None, :])
    assert bad.size == 0, (len(bad), [(32 + c, k, float(w[32 + c, k]).hex(), float(want_w[k]).hex()) for c, k in bad[:6]])
    # all classes, the criterion of test_bf16_grad_step_vs_oracle_on_rounded_operands
    np.testing.assert_allclose(w / -LR, want64, atol=8e-3 * np.abs(want64).max(), rtol=2e-2)


@pytest.mark.parametrize("variant", ["grid3", "lazy", "lazy_grid3"])
def test_update_slices_under_stealing_equal_launch_per_kernel_step(variant, monkeypatch):
    """d = 512, C = 256 (8 dW tiles x 4 + 4 slabs; a short text batch makes it 6 + 2, an image-only step 8 + 0): six AdamW
    steps of the one-launch step on 3 workgroups, with every fourth workgroup leaving its forward and dW tiles to whoever
    needs them, and both, end bit-identical to the launch-per-kernel step; no wait gave up."""
    import umlh
    rng = np.random.default_rng(5)
    d, Cn, n = 512, 256, 4096
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    w = rng.standard_normal((Cn, d)).astype(np.float32)
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    feats, labels = torch.from_numpy(x).to(DEV), torch.from_numpy(rng.integers(0, Cn, n)).to(DEV)
    f16 = umlh.to_bf16(feats)
    sizes = [(4096, 4096), (4096, 1000), (3000, 4096), (4096, 0), (0, 4096), (4096, 4096)]
    out = {}
    for mode in ("0", "2"):
        env = {"UMLH_BF16_FUSE": mode}
        if mode == "2":
            if "grid3" in variant: env["UMLH_STEP_GRID"] = "3"
            if "lazy" in variant: env["UMLH_STEP_LAZY"] = "1"
        monkeypatch_engine_env(monkeypatch, env)
        e = umlh.HeadEngine(d, d, Cn, optimizer="adamw", weight_decay=0.01, max_rows_img=4096, max_rows_txt=4096,
                            precision="bf16", device=DEV)
        e.w_head.copy_(torch.from_numpy(w))
        e.scales.fill_(100.0)
        g = torch.Generator().manual_seed(7)
        scal = torch.zeros(len(sizes), umlh.N_SCALARS, device=DEV)
        for k, (ni, nt) in enumerate(sizes):
            ii, ti = torch.randint(0, n, (ni,), generator=g).to(DEV), torch.randint(0, n, (nt,), generator=g).to(DEV)
            bi = umlh.RowBatch(feats, labels, ii, feats_bf16=f16) if ni else None
            bt = umlh.RowBatch(feats, labels, ti, feats_bf16=f16) if nt else None
            e.train_step(bi, bt, lr=1e-3, step=k + 1, scalars_out=scal[k])
        torch.cuda.synchronize()
        assert e.step_status() == (0, 0, 0, 0)
        assert (e.step_launches() > 0) == (mode == "2")
        out[mode] = (e.w_head.clone(), e.m_head.clone(), e.v_head.clone(), scal.clone())
    for a, b in zip(out["0"], out["2"]):
        assert torch.equal(a, b)
    assert torch.isfinite(out["2"][0]).all()
