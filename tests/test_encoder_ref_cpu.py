"""CPU: the float64 reference of the encoder kernels (tests/_encoder_ref.py) is itself pinned -- against torch.nn's
TransformerEncoderLayer in float64, against explicit formulas and finite differences -- and the criterion it carries is shown to be
calibrated (the levels of the module docstring re-measured) and to discriminate (every deliberately wrong variant breaks its bound
by 8x or more).  No GPU, no `umlh` import."""
import re

import numpy as np
import pytest
import torch

import _encoder_ref as R

F64 = np.float64


def _t(a):
    return torch.from_numpy(np.asarray(a, F64))


# ---- layer_ref == torch.nn.TransformerEncoderLayer (float64, nothing dropped) ----
@pytest.mark.parametrize("c", R.LAYER_CASES + [R.STACK_CASE], ids=lambda c: c["id"])
def test_layer_ref_equals_torch_encoder_layer(c):
    T, B, Z, H, F = c["T"], c["B"], c["Z"], c["H"], c["d_ff"]
    params, h_in, dh_out = R.build_layer(c, c["seeds"][0])
    r = R.layer_ref(dict(c, p=0.0), params, h_in, c["lengths"], None, dh_out)
    layer = torch.nn.TransformerEncoderLayer(Z, H, dim_feedforward=F, dropout=0.0, activation="relu", norm_first=False,
                                             layer_norm_eps=float(np.float32(c["eps"]))).double()
    tp = [layer.self_attn.in_proj_weight, layer.self_attn.in_proj_bias, layer.self_attn.out_proj.weight, layer.self_attn.out_proj.bias,
          layer.linear1.weight, layer.linear1.bias, layer.linear2.weight, layer.linear2.bias, layer.norm1.weight, layer.norm1.bias,
          layer.norm2.weight, layer.norm2.bias]
    with torch.no_grad():
        for t, p in zip(tp, params[:12]):
            t.copy_(_t(p))
    layer.train()                                             # autograd on: the inference fast path is off
    x = _t(h_in).reshape(T, B, Z).clone().requires_grad_(True)
    causal = torch.triu(torch.ones(T, T, dtype=torch.bool), diagonal=1)
    pad = None
    if c["lengths"] is not None:
        pad = torch.arange(T)[None, :] >= torch.tensor(c["lengths"])[:, None]
    out = layer(x, src_mask=causal, src_key_padding_mask=pad)
    (out * _t(dh_out).reshape(T, B, Z)).sum().backward()

    def rel(got, ref):
        ref = ref.detach().numpy().reshape(got.shape)
        return np.abs(got - ref).max() / np.abs(ref).max()
    assert rel(r["h_out"], out) < 1e-10
    assert rel(r["dh_in"], x.grad) < 1e-10
    for name, g, t in zip(R.PARAM_NAMES, r["grads"], tp):
        assert rel(g, t.grad) < 1e-10, name


# ---- attention_ref ----
def _attention_explicit(qkv, lengths, T, B, Z, H):
    """Loops, one (b, h, t) at a time."""
    dh = Z // H
    x = np.asarray(qkv, F64).reshape(T, B, 3, H, dh)
    ctx, lse = np.zeros((T, B, H, dh)), np.zeros((B, H, T))
    for b in range(B):
        ln = T if lengths is None else lengths[b]
        for h in range(H):
            for t in range(T):
                js = [j for j in range(T) if j <= t and j < ln]
                s = np.array([x[t, b, 0, h] @ x[j, b, 1, h] for j in js]) / np.sqrt(dh)
                w = np.exp(s - s.max())
                lse[b, h, t] = s.max() + np.log(w.sum())
                ctx[t, b, h] = sum(wi / w.sum() * x[j, b, 2, h] for wi, j in zip(w, js))
    return ctx.reshape(T, B, Z), lse


@pytest.mark.parametrize("c", [c for c in R.ATT_CASES if c["T"] <= 9], ids=lambda c: c["id"])
def test_attention_ref_equals_explicit_masked_softmax(c):
    T, B, Z, H = c["T"], c["B"], c["Z"], c["H"]
    qkv, _ = R.build_attention(c)
    ctx, lse = R.attention_ref(qkv, c["lengths"], T, B, Z, H)
    ectx, else_ = _attention_explicit(qkv, c["lengths"], T, B, Z, H)
    np.testing.assert_allclose(ctx, ectx, rtol=0, atol=1e-12 * np.abs(ectx).max())
    np.testing.assert_allclose(lse, else_, rtol=0, atol=1e-12 * np.abs(else_).max())


def _directional(f, x, d, eps):
    return (f(x + eps * d) - f(x - eps * d)) / (2 * eps)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_attention_ref_gradient_against_central_difference(p):
    """With the mask held fixed the dropped attention is differentiable: d sum(ctx * dctx) / d qkv along random directions."""
    c = R.ATT_CASES[3]
    T, B, Z, H = c["T"], c["B"], c["Z"], c["H"]
    qkv, dctx = (a.astype(F64) for a in R.build_attention(c))
    keep = R.keep_mask(c["seed"], B * H * T * T, p).reshape(B, H, T, T) if p else None
    ik = R.inv_keep(p)
    dqkv = R.attention_ref(qkv, c["lengths"], T, B, Z, H, keep, ik, dctx)[2]
    f = lambda x: float((R.attention_ref(x, c["lengths"], T, B, Z, H, keep, ik)[0] * dctx).sum())
    rng = np.random.default_rng(5)
    for _ in range(3):
        d = rng.standard_normal(qkv.shape)
        fd, an = _directional(f, qkv, d, 1e-5), float((dqkv * d).sum())
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (fd, an)
    # dk, dv of padded keys are exactly 0
    g = dqkv.reshape(T, B, 3, Z)
    for b, ln in enumerate(c["lengths"]):
        assert not g[ln:, b, 1:].any()


def test_layer_ref_backward_against_central_difference_with_fixed_masks():
    """The masked layer is differentiable as written (the table's seeds keep every relu unit away from its kink): the backward
    of layer_ref agrees with a float64 central difference in h_in and in every parameter, all four masks active."""
    c = dict(R.STACK_CASE)
    del c["n_layers"]
    params, h_in, dh_out = R.build_layer(c, c["seeds"][0])
    params, h_in, dh_out = [p.astype(F64) for p in params], h_in.astype(F64), dh_out.astype(F64)
    masks = R.layer_masks(c, c["seed"])
    assert not all(m.all() for m in masks.values())
    r = R.layer_ref(c, params, h_in, c["lengths"], masks, dh_out)
    rng = np.random.default_rng(6)
    loss = lambda ps, h: float((R.layer_ref(c, ps, h, c["lengths"], masks)["h_out"] * dh_out).sum())
    d = rng.standard_normal(h_in.shape)
    fd, an = _directional(lambda h: loss(params, h), h_in, d, 1e-6), float((r["dh_in"] * d).sum())
    assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), ("h_in", fd, an)
    for i, name in enumerate(R.PARAM_NAMES):
        d = rng.standard_normal(params[i].shape)
        fd = _directional(lambda t: loss(params[:i] + [t] + params[i + 1:], h_in), params[i], d, 1e-6)
        an = float((r["grads"][i] * d).sum())
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (name, fd, an)


def test_stack_ref_is_layer_ref_chained():
    c = R.STACK_CASE
    params, h0, dh_out = R.build_layer(c, c["seeds"][0], 2)
    masks = R.stack_masks(c, c["p"])
    s = R.stack_ref(c, 2, params, h0, c["lengths"], masks, dh_out)
    l0 = R.layer_ref(c, params[:12], h0, c["lengths"], masks[0])
    l1 = R.layer_ref(c, params[12:], l0["h_out"], c["lengths"], masks[1], dh_out)
    b0 = R.layer_ref(c, params[:12], h0, c["lengths"], masks[0], l1["dh_in"])
    assert np.array_equal(s["h_out"], l1["h_out"]) and np.array_equal(s["dh_in"], b0["dh_in"])
    for a, b in zip(s["grads"], b0["grads"] + l1["grads"]):
        assert np.array_equal(a, b)
    # layer 1 draws from other streams than layer 0
    assert any((masks[0][k] != masks[1][k]).any() for k in masks[0])


# ---- small ops ----
def test_layernorm_ref_against_torch_and_autograd():
    for M, N, scale in ((5, 65, 1.0), (3, 1, 1.0), (5, 64, 1e-2)):
        x, r, gamma, beta, dy = R.build_layernorm(M, N, scale)
        s, y, mean, rstd = R.layernorm_ref(x, r, gamma, beta)
        ts = (_t(x) + _t(r)).requires_grad_(True)
        tg, tb = _t(gamma).requires_grad_(True), _t(beta).requires_grad_(True)
        ty = torch.nn.functional.layer_norm(ts, (N,), tg, tb, float(np.float32(R.EPS)))
        (ty * _t(dy)).sum().backward()
        np.testing.assert_allclose(y, ty.detach().numpy(), rtol=1e-12, atol=1e-12)
        ds, dg, db, _, _ = R.layernorm_bwd_ref(dy, s, gamma, mean, rstd)
        for got, ref in ((ds, ts.grad), (dg, tg.grad), (db, tb.grad)):
            np.testing.assert_allclose(got, ref.numpy(), rtol=1e-10, atol=1e-10 * max(1.0, float(ref.abs().max())))
        if N == 1:
            assert np.array_equal(y, np.broadcast_to(beta.astype(F64), y.shape))       # zero variance: y is beta


def test_keep_mask_and_inv_keep():
    for p in (0.1, 0.25, 0.3, 0.5):
        # the kernels' fp32 1.f / (1.f - p) is the float64 quotient rounded once, for every rate the tables use
        assert R.inv_keep(p, np.float32) == np.float32(R.inv_keep(p))
        n = 1 << 18
        m = R.keep_mask(77, n, p)
        q = 1.0 - float(np.float32(p))
        assert abs(m.mean() - q) < 5 * np.sqrt(q * (1 - q) / n)
        assert np.array_equal(m[:1000], R.keep_mask(77, 1000, p))
    assert R.keep_mask(1, 10, 0.0).all()


# ---- the criterion ----
@pytest.mark.parametrize("c", R.LAYER_CASES + [R.STACK_CASE], ids=lambda c: c["id"])
def test_table_seeds_have_no_relu_kink(c):
    assert c["seeds"][0] < 256                                # the GPU test's seed comes from a search over at most 256
    for s in c["seeds"]:
        assert R.case_kink_margin(c, s) > R.KINK, (c["id"], s)


def test_levels_of_the_docstring_are_remeasured_and_under_their_bounds():
    lv = R.measure_levels()
    assert {f: set(d) for f, d in lv.items()} == {f: set(d) for f, d in R.LEVELS_LOG2.items()}
    rows = {(m[1], m[2]): (float(m[3]), int(m[4])) for m in re.finditer(r"(\w+) +(\w+) +(-\d+\.\d) +(-\d+)(?= |\n)", R.__doc__)}
    for fam, d in lv.items():
        for k, v in d.items():
            rec = R.LEVELS_LOG2[fam][k]
            assert np.log2(v) <= rec + 0.3, (fam, k, np.log2(v), rec)
            assert 8 * v <= R.BOUNDS[fam][k] * 2 ** 0.3 and R.BOUNDS[fam][k] <= 16 * 2.0 ** rec
            assert rows[fam, k] == (rec, int(np.log2(R.BOUNDS[fam][k]))), (fam, k, rows.get((fam, k)))


@pytest.mark.parametrize("name", R.WRONG_VARIANTS)
def test_every_wrong_variant_breaks_its_bound_by_8x(name):
    assert R.variant_excess(name) >= 8.0, name
