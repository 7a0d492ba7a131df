"""GPU: umlh.spectral (fp64 Gram + Householder tridiagonalisation + Sturm bisection) against float64 numpy.

The accuracy condition: for every case max|sv - sv64| / sigma_max and |erank - erank64| / erank64 are no larger than the same
errors of the reference's own fp32 CPU results (torch.linalg.svdvals + utilis.py:27-36), with a floor of 4 ulp of fp64 for
the cases the reference gets exactly.  For the golden cases the reference's errors are stored in the golden; for generated
cases they are computed here on the CPU copy.  Every measured figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import _spectral_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 4 * np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def gold():
    return load_golden("effective_rank")


def _reference_errors(a):
    """The reference's arithmetic in fp32 on the CPU, measured against float64: (sv error / sigma_max, erank error)."""
    t = torch.from_numpy(a).unsqueeze(0)
    sv = torch.linalg.svdvals(t)
    p = sv / sv.sum(dim=-1, keepdim=True)
    er = torch.exp(-torch.sum(p * torch.log(p + 1e-6), dim=-1))
    return R.errors(sv[0].numpy(), float(er[0]), R.svdvals64(a), R.erank64(a))


def _check(tag, sv, er, sv64, er64, ref_err):
    got = R.errors(sv, er, sv64, er64)
    print(f"{tag}: sv err {got[0]:.3e} sigma_max (reference fp32 {ref_err[0]:.3e}), erank err {got[1]:.3e} "
          f"(reference fp32 {ref_err[1]:.3e}), erank {float(er):.12f} float64 {float(er64):.12f}")
    assert got[0] <= max(ref_err[0], FLOOR), (tag, got, ref_err)
    assert got[1] <= max(ref_err[1], FLOOR), (tag, got, ref_err)


def _gen(n, d):
    g = np.random.default_rng(1000 * n + d)
    a = g.standard_normal((n, d)) * g.uniform(0.3, 3.0, d)
    return a.astype(np.float32)


@pytest.mark.parametrize("n,d", [(1, 1), (5, 7), (257, 35), (40, 64), (64, 65), (1600, 300)])
def test_accuracy_against_float64_generated(n, d):
    import umlh
    a = _gen(n, d)
    x = torch.from_numpy(a).to(DEV)
    er, sv = umlh.effective_rank(x, return_svdvals=True)
    sv2 = umlh.svdvals(x)
    assert sv.shape == (min(n, d),) and sv.dtype == torch.float64 and er.shape == () and er.dtype == torch.float64
    assert torch.equal(sv, sv2)
    sv = sv.cpu().numpy()
    assert (np.diff(sv) <= 0).all()
    _check(f"gen {n}x{d}", sv, float(er), R.svdvals64(a), R.erank64(a), _reference_errors(a))


@pytest.mark.parametrize("case", ["ragged", "wide", "rank5"])
def test_accuracy_against_float64_golden(gold, case):
    import umlh
    a = gold[f"{case}/a"]
    er, sv = umlh.effective_rank(torch.from_numpy(a).to(DEV), return_svdvals=True)
    assert sv.shape == (min(a.shape),)
    _check(case, sv.cpu().numpy(), float(er), gold[f"{case}/sv64"][0], gold[f"{case}/erank64"][0],
           (float(gold[f"{case}/ref_sv_err"][0]), float(gold[f"{case}/ref_erank_err"][0])))


def test_batch_of_three_and_the_utilis_drop_in(gold):
    import umlh
    from multibench import utilis
    a = gold["batch3/a"]
    x = torch.from_numpy(a).to(DEV)
    er, sv = umlh.effective_rank(x, return_svdvals=True)
    assert er.shape == (3,) and sv.shape == (3, 24)
    drop_in = utilis.compute_effective_rank(x)
    assert drop_in.shape == (3,) and drop_in.dtype == torch.float32 and drop_in.device == x.device
    er, sv, drop_in = er.cpu().numpy(), sv.cpu().numpy(), drop_in.cpu().numpy()
    for b in range(3):
        ref_err = (float(gold["batch3/ref_sv_err"][b]), float(gold["batch3/ref_erank_err"][b]))
        _check(f"batch3[{b}]", sv[b], er[b], gold["batch3/sv64"][b], gold["batch3/erank64"][b], ref_err)
        _check(f"batch3[{b}] utilis", sv[b], drop_in[b], gold["batch3/sv64"][b], gold["batch3/erank64"][b], ref_err)
    # a batch is the same computation as its matrices one by one, and a strided batch view is read in place
    one = umlh.effective_rank(x[1])
    assert float(one) == er[1]
    wide = torch.zeros(3, 130, 40, device=DEV)
    wide[:, 5:125, 8:32] = x
    assert torch.equal(umlh.effective_rank(wide[:, 5:125, 8:32]), torch.from_numpy(er).to(DEV))


def test_batch_of_three_with_two_column_tiles():
    """batch > 1 with d > 64: three tile pairs per matrix, each matrix with its own slabs; a batch is its matrices one by one."""
    import umlh
    a = np.stack([_gen(40, 65 + 100 * b)[:, :65] for b in range(3)])
    x = torch.from_numpy(a).to(DEV)
    er, sv = umlh.effective_rank(x, return_svdvals=True)
    assert er.shape == (3,) and sv.shape == (3, 40) and torch.equal(sv, umlh.svdvals(x))
    for b in range(3):
        _check(f"batch 3 x 40x65 [{b}]", sv[b].cpu().numpy(), float(er[b]), R.svdvals64(a[b]), R.erank64(a[b]), _reference_errors(a[b]))
        assert float(umlh.effective_rank(x[b])) == float(er[b])


def test_fewer_rows_than_columns_returns_n_values(gold):
    """The d - n surplus eigenvalues of the Gram matrix (rounding noise around zero) must not reach the entropy."""
    import umlh
    a = gold["wide/a"]
    er, sv = umlh.effective_rank(torch.from_numpy(a).to(DEV), return_svdvals=True)
    assert sv.shape == (40,)
    got = R.errors(sv.cpu().numpy(), float(er), gold["wide/sv64"][0], gold["wide/erank64"][0])
    print(f"wide 40x64: erank {float(er):.12f} float64 {float(gold['wide/erank64'][0]):.12f} rel err {got[1]:.3e}")
    assert got[1] <= max(float(gold["wide/ref_erank_err"][0]), FLOOR)
    # the sequence form reports all d slots: 40 values, then exact zeros
    out, svd = umlh.effective_rank_seq(torch.from_numpy(a).to(DEV).unsqueeze(0), return_svdvals=True)
    svd = svd.cpu().numpy()
    assert svd.shape == (64,) and (svd[40:] == 0).all() and (svd[:40] > 0).all()
    assert out.cpu().tolist() == [float(er), 40.0]


SEQ_LENS = [9, 1, 4, 9, 2]


@pytest.fixture(scope="module")
def seq_block():
    g = np.random.default_rng(7)
    return (g.standard_normal((5, 9, 24)) * g.uniform(0.5, 2.0, 24)).astype(np.float32)


def _seq_check(tag, out, z, lens, drop):
    want, rows = R.erank_seq64(z, lens, drop)
    out = out.cpu().numpy()
    rel = abs(out[0] - want) / want
    ref = _reference_errors(np.ascontiguousarray(R.valid_rows(z, lens, drop)))[1]
    print(f"{tag}: rows {out[1]:.0f} (float64 {rows}), erank {out[0]:.12f} float64 {want:.12f} rel err {rel:.3e} (reference fp32 {ref:.3e})")
    assert out[1] == rows
    assert rel <= max(ref, FLOOR)
    return out


@pytest.mark.parametrize("drop,rows", [(0, 25), (1, 20)])
def test_sequence_form(seq_block, drop, rows):
    import umlh
    z = torch.from_numpy(seq_block).to(DEV)
    lens = torch.tensor(SEQ_LENS, device=DEV)
    base = _seq_check(f"seq drop={drop}", umlh.effective_rank_seq(z, lens, drop_last=drop), seq_block, SEQ_LENS, drop)
    assert base[1] == rows
    # lengths on the host, as int32, and out of range (clamped to 0..T)
    assert umlh.effective_rank_seq(z, torch.tensor(SEQ_LENS, dtype=torch.int32), drop_last=drop).cpu().tolist() == base.tolist()
    assert umlh.effective_rank_seq(z, torch.tensor([50, 1, 4, 9, 2]), drop_last=drop).cpu().tolist() == base.tolist()
    _seq_check(f"seq drop={drop} lengths=None", umlh.effective_rank_seq(z, None, drop_last=drop), seq_block, None, drop)
    # a [T, B, d] block passed by strides and a column block of a wider tensor: the same rows in the same order
    tbd = z.transpose(0, 1).contiguous()
    view = tbd.transpose(0, 1)
    assert view.stride() == (24, 5 * 24, 1)
    assert umlh.effective_rank_seq(view, lens, drop_last=drop).cpu().tolist() == base.tolist()
    wide = torch.full((5, 9, 40), 3.0, device=DEV)
    wide[:, :, 11:35] = z
    block = wide[:, :, 11:35]
    assert block.stride() == (360, 40, 1)
    assert umlh.effective_rank_seq(block, lens, drop_last=drop).cpu().tolist() == base.tolist()
    # rows past a sequence's length never enter: garbage there changes nothing
    dirty = z.clone()
    for b, l in enumerate(SEQ_LENS):
        dirty[b, max(l - drop, 0):] = float("nan")
    assert umlh.effective_rank_seq(dirty, lens, drop_last=drop).cpu().tolist() == base.tolist()


def test_sequence_edge_cases(seq_block):
    import umlh
    z = torch.from_numpy(seq_block).to(DEV)
    out, sv = umlh.effective_rank_seq(z, torch.ones(5, dtype=torch.int64), drop_last=1, return_svdvals=True)
    print("no valid rows:", out.cpu().tolist())
    assert out.cpu().tolist() == [1.0, 0.0] and (sv == 0).all()
    out = umlh.effective_rank_seq(torch.zeros_like(z), torch.tensor(SEQ_LENS)).cpu().numpy()
    print("all-zero block:", out)
    assert np.isnan(out[0]) and out[1] == 25
    assert np.isnan(float(umlh.effective_rank(torch.zeros(6, 4, device=DEV))))
    assert (umlh.svdvals(torch.zeros(6, 4, device=DEV)) == 0).all()


def test_bitwise_reproducible_and_stream_independent():
    import umlh
    a = torch.from_numpy(_gen(700, 130)).to(DEV)
    er1, sv1 = umlh.effective_rank(a, return_svdvals=True)
    er2, sv2 = umlh.effective_rank(a, return_svdvals=True)
    assert torch.equal(er1, er2) and torch.equal(sv1, sv2)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        er3, sv3 = umlh.effective_rank(a, return_svdvals=True)
    side.synchronize()
    assert torch.equal(er1, er3) and torch.equal(sv1, sv3)
    sv64 = R.svdvals64(a.cpu().numpy())
    assert np.abs(sv1.cpu().numpy() - sv64).max() <= 1e-9 * sv64.max()


class _ListLoader(list):
    """A list of batches in the reference's layout; deep-copied and re-iterated like a DataLoader."""


def _train_setup(seed):
    from engine.optimizer.optim import build_optimizer
    from multibench.models import Linear, Transformer, UML
    torch.manual_seed(seed)
    z, dx, dy, B, T = 20, 12, 24, 5, 9
    m = UML(Linear(dx, z), Linear(dy, z), Transformer(z, z, nhead=5, num_layers=1, conv1d=True, out_last=False, pos_embd=True,
                                                       pos_learnable=False, max_len=128),
            [Linear(z, dx), Linear(z, dy)], modality="xy").to(DEV).eval()
    m.train = lambda *a, **k: m                   # stay in eval mode (dropout off): the run with the switch retraces the one without
    g = torch.Generator().manual_seed(99)
    lens = [torch.tensor(SEQ_LENS), torch.tensor([3, 9, 9, 1, 6]), torch.tensor([2, 2, 9, 5, 7])]
    mk = lambda i: [[torch.randn(B, T, dx, generator=g), None, torch.randn(B, T, dy, generator=g)], [lens[i], None, lens[(i + 1) % 3]]]
    l1, l2 = _ListLoader(mk(i) for i in range(3)), _ListLoader(mk(i) for i in range(3))
    return m, l1, l2, build_optimizer(m.parameters(), "adam", 1e-3, 0.0)


def test_train_effective_rank_switch():
    from multibench import train as mbt
    seen = []
    m, l1, l2, opt = _train_setup(0)
    res = mbt.train(m, "xy", l1, l2, opt, modalities=[0, 2], num_epoch=1, step_k=-1, device=DEV, effective_rank=True,
                    on_step=lambda e, i, out, loss: seen.append(out["y_recon"].detach().cpu().numpy().copy()))
    assert len(res["pred_effective_rank_y"]) == 3 and len(seen) == 3
    for i, (got, recon) in enumerate(zip(res["pred_effective_rank_y"], seen)):
        lens = l2[i][1][2].numpy()
        want, rows = R.erank_seq64(recon, lens, 1)
        ref = _reference_errors(np.ascontiguousarray(R.valid_rows(recon, lens, 1)))[1]
        rel = abs(got - want) / want
        print(f"train step {i}: rows {rows}, pred erank {got:.12f} float64 {want:.12f} rel err {rel:.3e} (reference fp32 {ref:.3e})")
        assert rel <= max(ref, FLOOR)
    y_all = np.concatenate([b[0][2].numpy() for b in l2])
    len_all = np.concatenate([b[1][2].numpy() for b in l2])
    want, rows = R.erank_seq64(y_all, len_all, 0)
    ref = _reference_errors(np.ascontiguousarray(R.valid_rows(y_all, len_all, 0)))[1]
    rel = abs(res["gt_effective_rank_y"] - want) / want
    print(f"train gt: rows {rows}, erank {res['gt_effective_rank_y']:.12f} float64 {want:.12f} rel err {rel:.3e} (reference fp32 {ref:.3e})")
    assert rel <= max(ref, FLOOR)
    # the switch changes nothing else: same seed, switch off -> bit-equal losses, and no rank keys
    m2, k1, k2, opt2 = _train_setup(0)
    off = mbt.train(m2, "xy", k1, k2, opt2, modalities=[0, 2], num_epoch=1, step_k=-1, device=DEV)
    assert "pred_effective_rank_y" not in off and "gt_effective_rank_y" not in off
    for k in ("loss_x", "loss_y", "loss"):
        assert off[k] == res[k], k
    # 'y' not trained: nothing to measure
    m3, j1, j2, opt3 = _train_setup(0)
    only_x = mbt.train(m3, "x", j1, j2, opt3, modalities=[0, 2], num_epoch=1, step_k=-1, device=DEV, effective_rank=True)
    assert "pred_effective_rank_y" not in only_x
