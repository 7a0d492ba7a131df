"""GPU: umlh.seq_step_stats (umlh_kernels_stepstats.hip) against the float64 statement of tests/_stepstats_ref.py, and
multibench.train.train(step_diagnostics=True) end to end.

Bounds.  Values against float64: 1e-12 relative.  The kernel adds non-negative fp64 terms in chains of at most 4096 (256 per
thread in the partial kernel, ceil(partials / 1024) in the final) and trees above them, so its error is below
(4096 + log2(partials) + 4) 2^-53 < 5e-13; the numpy statement's pairwise sums are far inside that.  Counts are integers and
must be equal.  Against what the reference logged: the fixture's ``bound`` (tests/_stepstats_ref.py).  recon_y_loss against the
model's own loss_y under the MSE critic: 1e-4 relative, the project's loss parity bar (the two come from different kernels, one
of them fp32).  Every measured figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import _stepstats_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _data(B, T, d, seed, lengths=True):
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, T, d)).astype(np.float32)
    r = (x + 0.5 * g.standard_normal((B, T, d))).astype(np.float32)
    lens = None
    if lengths:
        pool = np.array([-1, 0, 1, 2, T - 1, T, T + 5])
        lens = pool[(np.arange(B) + g.integers(0, 7)) % 7] if B >= 7 else g.choice(pool, B)
    return x, r, lens


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def _compare(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (4,)
    for i in (0, 2):
        err = abs(got[i] - want[i]) / abs(want[i]) if want[i] != 0 else abs(got[i])
        print(f"{what} slot {i}: got {got[i]!r} float64 {want[i]!r} rel {err:.2e}")
        assert err <= TOL, (what, i)
    assert got[1] == want[1] and got[3] == want[3], (what, got, want)


@pytest.mark.parametrize("d", [1, 3, 35, 64, 65, 300])
def test_against_float64(d):
    import umlh
    for T in (1, 2, 3, 50):
        for B in (1, 2, 33):
            x, r, lens = _data(B, T, d, 1000 * d + 10 * T + B)
            xd, rd, ld = _dev(x), _dev(r), _dev(lens)
            _compare(umlh.seq_step_stats(xd, ld, rd), R.step_stats(x, lens, r), f"d={d} T={T} B={B}")
    x, r, lens = _data(33, 50, d, d)
    xd, rd, ld = _dev(x), _dev(r), _dev(lens)
    _compare(umlh.seq_step_stats(xd, None, rd), R.step_stats(x, None, r), f"d={d} no lengths")
    got = umlh.seq_step_stats(xd, ld)
    _compare(got, R.step_stats(x, lens), f"d={d} no recon")
    assert got[2].item() == 0.0 and got[3].item() == 0.0
    assert np.array_equal(_bits(got[:2]), _bits(umlh.seq_step_stats(xd, ld, rd)[:2]))          # recon does not touch the trivial sums


def test_more_than_one_row_chunk_and_column_chunk():
    import umlh
    for B, T, d in ((3, 131, 9), (2, 4, 1030), (2, 70, 1025)):                  # 64 pair rows and 1024 columns per workgroup
        x, r, _ = _data(B, T, d, T + d)
        lens = np.array([T, T - 3, 66][:B])
        _compare(umlh.seq_step_stats(_dev(x), _dev(lens), _dev(r)), R.step_stats(x, lens, r), f"B={B} T={T} d={d}")


def test_more_partial_sums_than_threads_in_the_final():
    """B = 2500 at T = 3: 2500 partial sums, so every thread of the 1024-thread final adds a chain of up to three and strides
    the lengths more than once."""
    import umlh
    x, r, lens = _data(2500, 3, 3, 77)
    assert set(lens.tolist()) == {-1, 0, 1, 2, 3, 8}
    _compare(umlh.seq_step_stats(_dev(x), _dev(lens), _dev(r)), R.step_stats(x, lens, r), "B=2500 T=3 d=3")


@pytest.mark.parametrize("d", [35, 64])
def test_strided_views_are_read_in_place(d):
    import umlh
    from umlh import stepstats
    B, T = 5, 9
    x, r, lens = _data(B, T, d, 7 + d)
    lens = np.array([9, 4, 0, 1, 12])
    want = R.step_stats(x, lens, r)
    base = umlh.seq_step_stats(_dev(x), _dev(lens), _dev(r))
    _compare(base, want, "contiguous")
    x_tb, r_tb = _dev(x.transpose(1, 0, 2)), _dev(r.transpose(1, 0, 2))          # [T, B, d] blocks
    wide_x, wide_r = np.zeros((B, T, d + 7), np.float32), np.full((B, T, d + 8), np.nan, np.float32)
    wide_x[:, :, 3:3 + d], wide_r[:, :, 4:4 + d] = x, r
    x_col, r_col = _dev(wide_x)[:, :, 3:3 + d], _dev(wide_r)[:, :, 4:4 + d]      # column blocks of wider tensors
    for v in (x_tb.transpose(0, 1), x_col):
        assert stepstats._block(v, torch.device(DEV)).data_ptr() == v.data_ptr()                 # no copy on the way to the kernel
    for what, xv, rv in (("[T, B, d] both", x_tb.transpose(0, 1), r_tb.transpose(0, 1)), ("column blocks", x_col, r_col),
                         ("x contiguous, recon [T, B, d]", _dev(x), r_tb.transpose(0, 1)),
                         ("x column block, recon contiguous", x_col, _dev(r))):
        got = umlh.seq_step_stats(xv, _dev(lens), rv)
        _compare(got, want, what)
        assert np.array_equal(_bits(got), _bits(base)), what                     # 16-byte and 4-byte loads add in the same order
    col_major = _dev(x.transpose(0, 2, 1)).transpose(1, 2)                        # last stride T: copied, same values
    assert np.array_equal(_bits(umlh.seq_step_stats(col_major, _dev(lens), _dev(r))), _bits(base))


@pytest.mark.parametrize("d,T", [(35, 9), (64, 9), (300, 50)])
def test_padding_does_not_reach_the_result(d, T):
    """Inf in x rows t > len_b and in recon rows t >= max(len_b - 1, 0): both masks, the one-row reach of the trivial one included."""
    import umlh
    B = 9
    x, r, _ = _data(B, T, d, 50 + d)
    lens = np.array([-1, 0, 1, 2, T - 1, T, T + 5, 3, T - 2])
    clean = umlh.seq_step_stats(_dev(x), _dev(lens), _dev(r))
    _compare(clean, R.step_stats(x, lens, r), f"d={d} clean")
    xp, rp = x.copy(), r.copy()
    for b, n in enumerate(np.clip(lens, 0, T)):
        xp[b, n + 1:] = np.inf
        rp[b, max(n - 1, 0):] = np.inf
    assert np.isinf(xp).any() and np.isinf(rp).any()
    got = umlh.seq_step_stats(_dev(xp), _dev(lens), _dev(rp))
    assert torch.isfinite(got).all() and np.array_equal(_bits(got), _bits(clean))
    xq = x.copy()                                                                # one row earlier: the trivial pair (len - 1, len) sees it
    xq[3, 2] = np.inf
    assert torch.isinf(umlh.seq_step_stats(_dev(xq), _dev(lens), _dev(r))[0])
    rq = r.copy()                                                                # recon row len - 2 is the last one that counts
    rq[3, 0] = np.inf
    assert torch.isinf(umlh.seq_step_stats(_dev(x), _dev(lens), _dev(rq))[2])


def test_writes_four_slots_and_nothing_else():
    import umlh
    from umlh import _glue as glue
    lib = umlh.load_library()
    x, r, lens = _data(5, 9, 35, 11)
    xd, rd, ld = _dev(x), _dev(r), _dev(lens)
    nbytes = lib.umlh_seq_step_stats_scratch_bytes(5, 9, 35)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    for recon in (rd, None):
        out = torch.full((5,), float("nan"), dtype=torch.float64, device=DEV)
        rc = lib.umlh_seq_step_stats(xd.data_ptr(), 9 * 35, 35, glue.ptr(recon), 9 * 35, 35, 5, 9, 35, ld.data_ptr(), out.data_ptr(),
                                     scratch.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.umlh_last_error()
        got = out.cpu().numpy()
        assert np.isfinite(got[:4]).all() and np.isnan(got[4])
        _compare(out[:4], R.step_stats(x, lens, None if recon is None else r), "sentinel buffer")


def test_calls_and_streams_are_bit_equal():
    import umlh
    x, r, lens = _data(33, 50, 300, 12)
    xd, rd, ld = _dev(x), _dev(r), _dev(lens)
    first = umlh.seq_step_stats(xd, ld, rd)
    second = umlh.seq_step_stats(xd, ld, rd)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third = umlh.seq_step_stats(xd, ld, rd)
    side.synchronize()
    assert np.array_equal(_bits(first), _bits(second)) and np.array_equal(_bits(first), _bits(third))
    _compare(first, R.step_stats(x, lens, r), "B=33 T=50 d=300")


def test_golden_tensors_reproduce_the_logged_values():
    import umlh
    g = load_golden("step_stats")
    bound = float(g["bound"])
    for run in ("mse", "nce"):
        for s in range(g[f"{run}::x"].shape[0]):
            logged = dict(zip(R.LOGGED_KEYS, g[f"{run}::logged"][s]))
            x, lx, y, ly, yr = (g[f"{run}::{k}"][s] for k in ("x", "lx", "y", "ly", "y_recon"))
            sx = umlh.seq_step_stats(_dev(x), _dev(lx)).cpu().numpy()
            sy = umlh.seq_step_stats(_dev(y), _dev(ly), _dev(yr)).cpu().numpy()
            for key, got in (("train/trivial_loss_x", sx[0]), ("train/trivial_loss_y", sy[0]), ("train/recon_y_loss", sy[2])):
                rel = abs(got - logged[key]) / abs(logged[key])
                print(f"{run} step {s} {key}: logged {logged[key]:.9g} got {got:.12g} rel {rel:.2e} (bound {bound:.2e})")
                assert rel <= bound, (run, s, key)


# ---- train end to end ----
class _ListLoader(list):
    batch_size = 16


def _model(name):
    from multibench.models import Linear, Transformer, UML
    g = load_golden(name)
    z, dx, dy, B, T, pe, pl = (int(v) for v in g["cfg"])
    m = UML(Linear(dx, z), Linear(dy, z), Transformer(z, z, nhead=5, num_layers=5, conv1d=True, out_last=False,
                                                       pos_embd=bool(pe), pos_learnable=bool(pl), max_len=128),
            [Linear(z, dx), Linear(z, dy)], modality="xy")
    m.load_state_dict({k[4:]: torch.as_tensor(g[k]) for k in g.files if k.startswith("sd::")})
    m = m.to(DEV).eval()
    m.train = lambda *a, **k: m                                              # stay in eval mode (dropout off): runs retrace each other
    return m


@pytest.fixture(scope="module")
def e2e():
    """The model and the first 48 training sequences of the humor golden, three batch pairs; the y lengths are the x lengths
    rolled by one within each batch."""
    g = load_golden("probe_e2e_humor")
    x, y, lx = (torch.from_numpy(g[f"{k}_train"]) for k in ("x", "y", "lx"))
    loader = _ListLoader(([x[s:s + 16], None, y[s:s + 16]], [lx[s:s + 16], None, lx[s:s + 16].roll(1)]) for s in range(0, 48, 16))
    return str(g["model"]), loader


def _train(e2e, mode="xy", **kw):
    from multibench.train import train
    name, loader = e2e
    model = _model(name)
    seen = []
    res = train(model, mode, loader, loader, torch.optim.Adam(model.parameters(), lr=1e-3), num_epoch=1, step_k=-1, ds_name="humor",
                device=DEV, on_step=lambda e, i, out, loss: seen.append(out["y_recon"].detach().clone() if out["y_recon"] is not None
                                                                        else None), **kw)
    return res, seen


NEW = ("trivial_loss_x", "trivial_loss_y", "recon_y_loss", "loss_x_norm", "loss_y_norm", "loss_private", "diff_next_x", "diff_next_y")


def test_train_step_diagnostics(e2e):
    import umlh
    _, loader = e2e
    on, seen = _train(e2e, step_diagnostics=True)
    off, _ = _train(e2e)
    assert set(off) == {"loss_x", "loss_y", "loss"} and set(on) == set(off) | set(NEW)
    for k in ("loss_x", "loss_y", "loss"):
        assert on[k] == off[k] and len(on[k]) == 3, k                            # the flag leaves the training untouched
    for k in NEW:
        assert len(on[k]) == 3 and all(isinstance(v, float) and np.isfinite(v) for v in on[k]), k
    for i, (batch, y_recon) in enumerate(zip(loader, seen)):
        x, y, lx, ly = batch[0][0].to(DEV), batch[0][2].to(DEV), batch[1][0].to(DEV), batch[1][2].to(DEV)
        sx, sy = umlh.seq_step_stats(x, lx).tolist(), umlh.seq_step_stats(y, ly, y_recon).tolist()
        assert on["trivial_loss_x"][i] == sx[0] and on["trivial_loss_y"][i] == sy[0] and on["recon_y_loss"][i] == sy[2]
        _compare(torch.tensor(sy, dtype=torch.float64), R.step_stats(y.cpu().numpy(), ly.cpu().numpy(), y_recon.cpu().numpy()), f"step {i} y")
        rel = abs(on["recon_y_loss"][i] - on["loss_y"][i]) / on["loss_y"][i]
        print(f"step {i}: recon_y_loss {on['recon_y_loss'][i]!r} loss_y {on['loss_y'][i]!r} rel {rel:.2e}")
        assert rel <= 1e-4                                                       # MSE critic: the same quantity from another kernel
        assert on["loss_x_norm"][i] == abs(on["loss_x"][i]) and on["loss_y_norm"][i] == abs(on["loss_y"][i])
        assert on["trivial_loss_x"][i] > 0 and on["diff_next_x"][i] > 0 and on["diff_next_y"][i] > 0 and on["loss_private"][i] >= 0


def test_train_step_diagnostics_follow_the_train_mode(e2e):
    only_y, _ = _train(e2e, mode="y", step_diagnostics=True)
    assert set(only_y) == {"loss_x", "loss_y", "loss", "trivial_loss_y", "recon_y_loss", "loss_x_norm", "loss_y_norm", "loss_private",
                           "diff_next_y"}
    assert only_y["loss_x_norm"] == [0.0] * 3 and only_y["loss_private"] == [0.0] * 3 and len(only_y["trivial_loss_y"]) == 3
    only_x, _ = _train(e2e, mode="x", step_diagnostics=True)
    assert set(only_x) == {"loss_x", "loss_y", "loss", "trivial_loss_x", "loss_x_norm", "loss_y_norm", "loss_private", "diff_next_x"}
    assert len(only_x["trivial_loss_x"]) == 3 and only_x["loss_y_norm"] == [0.0] * 3
