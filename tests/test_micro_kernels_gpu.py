"""GPU: every instantiation of the single-launch micro step (csrc/umlh_kernels_micro.hip: 13 fp32 and 7 bf16 (NCH, CW) kernels)
against the float64 statement of ONE step (tests/_micro_ref.py), and multi-step launches against chains of single steps.

  * gradient probe: SGD with momentum 0, no decay and zero moments makes m_head after one step the dW the kernel formed
    (0 * m + g is exact); it is compared element by element, |got - ref64| / S, with the losses, accuracies and d loss / d scale;
  * a real optimizer step from a live state (sgd / adam / adamw; moments in registers, v in memory, m and v in memory):
    W', m', v', the scale triple and all eight scalars -- the test of opt_update_fast's hardware rcp / sqrt;
  * bf16 operand mode bit for bit on exactly representable operands (tests/_bf16_exact_ref.py on the step's own denominators);
  * one call of n steps == n calls of one step, bit for bit, for every instantiation (row tables two steps ahead, the offsets
    window, buffer parities, a full period of the resident-rows ring), across the 512-step launch split, and a grouped launch
    of heterogeneous heads == isolated runs.  With the single-step results this carries correctness to any number of steps.

Every bound is calibrated on the CPU (tests/_micro_ref.py, re-measured by tests/test_micro_ref_cpu.py), never on the device.
Every run keeps W / m / v and the scalar rows between guard rows of a NaN pattern no kernel produces and checks them after.
Each case prints its figures (`MICRO_ACC ...`); profiles/micro_accuracy.txt is that output."""
import numpy as np
import pytest
import torch

import _bf16_exact_ref as X
import _micro_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x7FBADBAD
LR_PROBE = 1e-2
PREC = {"fp32": False, "bf16": True}
INSTANCES = [("fp32", d) for d in R.WIDTHS_F32] + [("bf16", d) for d in R.WIDTHS_BF16]


def _T(a, t=torch.float32):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV, t).contiguous()          # (a copy: the shared tables are read-only)


_DEV_TABLES = {}


def _tables(tab, bf16):
    """((x, y[, x as bf16]) image, text) on the device, uploaded once per table set."""
    import umlh
    key = (id(tab), bf16)
    if key not in _DEV_TABLES:
        out = []
        for x, y in ((tab["xi"], tab["yi"]), (tab["xt"], tab["yt"])):
            xd = _T(x)
            out.append((xd, _T(y, torch.int64)) + ((umlh.to_bf16(xd),) if bf16 else ()))
        _DEV_TABLES[key] = (tab, tuple(out))
    return _DEV_TABLES[key][1]


def _guarded(rows, cols):
    """[rows, cols] fp32 view with one guard row of the sentinel pattern on either side: (whole buffer, view)."""
    whole = torch.full(((rows + 2) * cols,), SENT, dtype=torch.int32, device=DEV).view(torch.float32)
    return whole, whole[cols:(rows + 1) * cols].view(rows, cols)


def _guards_intact(whole, rows, cols):
    bits = whole.view(torch.int32)
    return bool((bits[:cols] == SENT).all()) and bool((bits[(rows + 1) * cols:] == SENT).all())


def _run(tab, d, C, batches, st, kind, lrs, first_step=1, *, wd=0.0, learn=False, momentum=0.9, precision="fp32", calls=None,
         weights=R.WEIGHTS, expect_micro=True):
    """Run len(batches) steps (batches[k] = (image row ids or None, text row ids or None)) from the state `st` as the calls
    `calls` (step counts; default one call).  Returns the state after, the scalar rows and the launch count."""
    import umlh
    n = len(batches)
    calls = calls or [n]
    assert sum(calls) == n == len(lrs)
    e = umlh.HeadEngine(d, d, C, learnable_temp=learn, optimizer=kind, weight_decay=wd, momentum=momentum, max_rows_img=64,
                        max_rows_txt=64, precision=precision, device=DEV)
    bufs = {k: _guarded(C, d) for k in ("w_head", "m_head", "v_head")}
    e.rebind(**{k: v[1] for k, v in bufs.items()})
    for k, src in (("w_head", "W"), ("m_head", "m"), ("v_head", "v"), ("scales", "scales"), ("m_scales", "m_scales"), ("v_scales", "v_scales")):
        getattr(e, k).copy_(_T(st[src]))
    sc_whole, sc = _guarded(n, umlh.N_SCALARS)
    ti, tt = _tables(tab, precision == "bf16")
    has_i, has_t = any(b[0] is not None for b in batches), any(b[1] is not None for b in batches)
    assert all((b[0] is not None) == has_i and (b[1] is not None) == has_t for b in batches), "a present stream has rows in every step"
    k0 = 0
    for c in calls:
        part = batches[k0:k0 + c]
        if c > 64:                                          # a long call: one concatenated vector per modality and the step sizes
            vec = lambda j: [(_T(np.concatenate([b[j] for b in part]), torch.int64), [len(b[j]) for b in part])]
        else:
            vec = lambda j: [_T(b[j], torch.int64) for b in part]
        bi, bt = (vec(0) if has_i else None), (vec(1) if has_t else None)
        e.train_steps(ti if has_i else None, bi, tt if has_t else None, bt, lrs[k0:k0 + c], first_step=first_step + k0,
                      alpha=weights[1], img_alpha=weights[0], scalars_out=sc[k0:k0 + c])
        k0 += c
    try:
        torch.cuda.synchronize()
    except RuntimeError as ex:                              # a device fault: nothing more is started on that GPU by this session
        pytest.exit(f"the device reported an error after a micro-step launch: {ex}", returncode=3)
    assert e.micro_status() == 0
    want = sum(-(-c // 512) for c in calls) if expect_micro else 0
    assert e.micro_launches() == want, (e.micro_launches(), want)
    for k, (whole, _) in bufs.items():
        assert _guards_intact(whole, C, d), f"{k}: a guard row was written"
    assert _guards_intact(sc_whole, n, umlh.N_SCALARS), "a scalar row outside the call's own was written"
    out = {dst: getattr(e, k).cpu().numpy().copy() for k, dst in (("w_head", "W"), ("m_head", "m"), ("v_head", "v"), ("scales", "scales"),
                                                                  ("m_scales", "m_scales"), ("v_scales", "v_scales"))}
    out["scalars"] = sc.cpu().numpy().copy()
    e.close()
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b, names=("W", "m", "v", "scales", "m_scales", "v_scales", "scalars")):
    for k in names:
        n = int((_bits(a[k]) != _bits(b[k])).sum())
        assert n == 0, f"{k}: {n} of {a[k].size} words differ"


def _report(tag, errs, mode, regime, prefix=""):
    """Print every figure next to its level and bound, then assert the bounds."""
    parts, bad = [], []
    for k, e in errs.items():
        if k == "acc":
            parts.append(f"acc {'exact' if e == 0 else 'WRONG'}")
            if e != 0:
                bad.append(k)
            continue
        lv, bd = R.LEVELS[(mode, regime)][prefix + k], R.bound(mode, regime, prefix + k)
        if k.startswith("g_"):
            parts.append(f"{k} 2^{np.log2(max(e, 1e-300)):.2f} (level 2^{np.log2(lv):.2f}, bound 2^{np.log2(bd):.0f})")
        else:
            parts.append(f"{prefix}{k} {e:.3g} (level {lv:.3g}, bound {bd:g})")
        if not e <= bd:
            bad.append(k)
    print(f"MICRO_ACC {tag}: " + "; ".join(parts))
    assert not bad, f"{tag}: {bad} above the bound"


def _probe(d, C, ri, rt, regime, precision, tag, *, tie=False, last_slice=False, expect_micro=True, v_pattern=True):
    """One step under the gradient probe; returns (device output, reference, tables)."""
    tab, ii, ti = R.build_case(d, C, ri, rt, regime, tie=tie, last_slice=last_slice)
    st = R.probe_state(tab)
    if v_pattern:                                           # SGD must leave v_head alone, bit for bit
        st["v"] = np.random.default_rng(d + C).standard_normal(st["v"].shape).astype(np.float32)
    out = _run(tab, d, C, [(ii, ti)], st, "sgd", [LR_PROBE], learn=True, momentum=0.0, precision=precision, expect_micro=expect_micro)
    ref = R.grad64(st, R.step_mods(tab, ii, ti), R.WEIGHTS, bf16=PREC[precision])
    mx, rms = R.grad_err(out["m"], ref)
    errs = dict(g_max=mx, g_rms=rms, **R.scalar_errs(out["scalars"][0], ref, True))
    _report(f"{tag} {precision} d={d} C={C} rows=({ri},{rt}) {regime}", errs, precision, regime)
    assert np.array_equal(_bits(out["v"]), _bits(st["v"])) and np.array_equal(_bits(out["v_scales"]), _bits(st["v_scales"]))
    # the probe's own premise: m_scales is d loss / d scale of the present modalities, an absent one keeps its scale
    for mod in (0, 1):
        if ref["present"][mod]:
            assert out["m_scales"][mod] == out["scalars"][0][R.S_GSCALE_IMG + mod]
        else:
            assert out["scales"][mod] == st["scales"][mod] and out["m_scales"][mod] == 0
    return out, ref, tab


# ---- the gradient itself, every instantiation ----
@pytest.mark.parametrize("regime", list(R.REGIMES))
@pytest.mark.parametrize("ri,rt", R.PROBE_ROWS)
@pytest.mark.parametrize("precision,d", INSTANCES)
def test_gradient_probe_every_instantiation(precision, d, ri, rt, regime):
    _probe(d, R.PROBE_C, ri, rt, regime, precision, "probe")


@pytest.mark.parametrize("ri,rt", R.PATTERNS)
@pytest.mark.parametrize("d,precision", R.PATTERN_WIDTHS)
def test_gradient_probe_row_patterns(d, precision, ri, rt):
    _probe(d, R.PROBE_C, ri, rt, "small", precision, "rows")


@pytest.mark.parametrize("C", R.CLASS_SWEEP)
@pytest.mark.parametrize("d", R.CLASS_WIDTHS)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_gradient_probe_class_counts(precision, d, C):
    """1 .. 64 class slices; half of the labels in the last (partial) slice; for C > 16 two bit-identical weight rows in the
    first and the last slice win some rows: the lower index must be reported (accuracy, and the merge of the arg-max)."""
    tie = C > R.CS
    out, ref, tab = _probe(d, C, 32, 32, "small", precision, "classes", tie=tie, last_slice=True)
    assert (tab["yi"] >= R.CS * ((C - 1) // R.CS)).sum() >= 20
    if tie:
        a, b = tab["tie"]
        assert a // R.CS == 0 and b // R.CS == (C - 1) // R.CS and np.array_equal(tab["W"][a], tab["W"][b])
        assert 0 < ref["scalars"][R.S_CORRECT] < 64         # rows labelled a count, rows labelled b do not


# ---- envelope edges: outside the micro path the general path must give the same step ----
@pytest.mark.parametrize("d,C,ri,rt", [(128, 37, 17, 47), (128, 37, 49, 15), (192, 37, 32, 32)],
                         ids=["5tiles_17_47", "5tiles_49_15", "width192"])
def test_outside_the_envelope_the_general_path_meets_the_same_bounds(d, C, ri, rt):
    assert not R.eligible(d, C, ri, rt)
    for regime in R.REGIMES:
        _probe(d, C, ri, rt, regime, "fp32", "general-path", expect_micro=False)


def test_a_65th_class_slice_is_no_valid_config():
    """include/umlh.h: num_classes is 1 .. 1024, so the 64 slices of C = 1024 (run by the class sweep above) are the end of the
    class axis for every path: C = 1025 is refused when the handle is made, not handed to the general path."""
    import umlh
    assert R.eligible(128, 1024, 8, 8) and not R.eligible(128, 1025, 8, 8)
    with pytest.raises(umlh.UmlhError):
        umlh.HeadEngine(128, 128, 1025, max_rows_img=64, max_rows_txt=64, device=DEV)


def test_bf16_refuses_a_width_that_is_no_multiple_of_128():
    """include/umlh.h: the bf16 operand mode of the micro path covers the multiples of 128 among its widths, the general bf16
    path needs d % 128 == 0 as well: a bf16 head of width 96 is no valid config."""
    import umlh
    assert R.eligible(96, 37, 8, 8) and not R.eligible(96, 37, 8, 8, bf16=True)
    with pytest.raises(umlh.UmlhError):
        umlh.HeadEngine(96, 96, 37, max_rows_img=64, max_rows_txt=64, precision="bf16", device=DEV)


# ---- a real optimizer step from a live state ----
@pytest.mark.parametrize("regime", list(R.REGIMES))
@pytest.mark.parametrize("learn", [False, True], ids=["fixed", "learnable"])
@pytest.mark.parametrize("kind", R.OPT_KINDS)
@pytest.mark.parametrize("precision,d", [("fp32", d) for d in R.OPT_WIDTHS] + [("bf16", d) for d in R.OPT_WIDTHS_BF16])
def test_optimizer_step_from_a_live_state(precision, d, kind, learn, regime):
    ri, rt = 17, 30
    tab, ii, ti = R.build_case(d, R.PROBE_C, ri, rt, regime)
    mods = R.step_mods(tab, ii, ti)
    st = R.live_case(tab, mods, d, bf16=PREC[precision])
    for step in R.OPT_STEPS:
        out = _run(tab, d, R.PROBE_C, [(ii, ti)], st, kind, [R.LR], first_step=step, wd=R.KIND_WD[kind], learn=learn, precision=precision)
        g, want = R.step64(st, mods, R.WEIGHTS, kind, R.LR, step, R.KIND_WD[kind], learn, bf16=PREC[precision])
        tag = f"update {precision} {kind} d={d} {'learnable' if learn else 'fixed'} step={step} {regime}"
        _report(tag, R.scalar_errs(out["scalars"][0], g, learn), precision, regime)
        _report(tag, R.state_errs(out, want, st, kind, learn), precision, regime, kind + ".")
        if kind == "sgd":
            assert np.array_equal(_bits(out["v"]), _bits(st["v"])) and np.array_equal(_bits(out["v_scales"]), _bits(st["v_scales"]))
        if not learn:
            for k in ("scales", "m_scales", "v_scales"):
                assert np.array_equal(_bits(out[k]), _bits(st[k])), k


# ---- bf16 operand mode, bit for bit ----
@pytest.mark.parametrize("shape", R.exact_shapes(), ids=lambda s: s.id)
def test_bf16_mode_is_bit_exact_on_representable_operands(shape):
    s = shape
    case, ref = X.case_and_reference(s)
    tab = dict(xi=case.xi, yi=case.yi, xt=case.xt, yt=case.yt, W=case.w_head, scale=s.scale, _case=case)
    st = R.make_state(case.w_head, scales=(s.scale, s.scale))
    ii, ti = (case.ii if s.ri else None), (case.ti if s.rt else None)
    weights = (X.IMG_ALPHA, X.ALPHA)
    out = _run(tab, s.d, s.C, [(ii, ti)], st, "sgd", [X.LR], momentum=0.0, precision="bf16", weights=weights)
    n_g, first_g = X.mismatches(out["m"], ref.g_head)
    n_w, first_w = X.mismatches(out["W"], ref.w_head_new)
    sc = out["scalars"][0]
    print(f"MICRO_ACC exact bf16 {s.id}: dW {n_g} words differ, W - lr g {n_w} words differ")
    assert n_g == 0, first_g
    assert n_w == 0, first_w
    for rows, loss, acc, want_loss, want_acc in ((s.ri, R.S_LOSS_IMG, R.S_ACC_IMG, ref.loss_img, ref.acc_img),
                                                 (s.rt, R.S_LOSS_TXT, R.S_ACC_TXT, ref.loss_txt, ref.acc_txt)):
        if rows:
            assert abs(float(sc[loss]) - want_loss) <= 1e-5 * max(1.0, abs(want_loss)), (float(sc[loss]), want_loss)
            assert np.float32(sc[acc]).view(np.uint32) == np.float32(want_acc).view(np.uint32), (float(sc[acc]), float(want_acc))
    # the same shape in fp32 mode: under the bounds of the sharp regime; whether it is bit-exact too is recorded, not asserted
    # (the reciprocal of the softmax sum is a 1-ulp instruction and fp32 mode has no bf16 rounding to absorb it)
    out32 = _run(tab, s.d, s.C, [(ii, ti)], st, "sgd", [X.LR], momentum=0.0, precision="fp32", weights=weights)
    g64 = R.grad64(st, R.step_mods(tab, ii, ti), weights)
    assert np.array_equal(g64["dW"].astype(np.float32), ref.g_head)            # the two float64 statements agree exactly
    mx, rms = R.grad_err(out32["m"], g64)
    exact32 = X.mismatches(out32["m"], ref.g_head)[0] == 0 and X.mismatches(out32["W"], ref.w_head_new)[0] == 0
    _report(f"exact fp32 {s.id} (bit-exact: {'yes' if exact32 else 'no'})", dict(g_max=mx, g_rms=rms, **R.scalar_errs(out32["scalars"][0], g64, False)),
            "fp32", "small")


# ---- multi-step == chain of single steps ----
CHAIN_ROWS = ((8, 8), (1, 1), (32, 32), (16, 48), (1, 48), (48, 16), (33, 16), (20, 30), (17, 30))   # 1-row next to 64-row steps


def _chain_batches(n, seed):
    rng = np.random.default_rng(seed)
    return [(R.draw_ids(rng, R.N_IMG, CHAIN_ROWS[k % 9][0]), R.draw_ids(rng, R.N_TXT, CHAIN_ROWS[k % 9][1])) for k in range(n)]


@pytest.mark.parametrize("precision,d", INSTANCES)
def test_nine_steps_in_one_call_equal_nine_calls_bit_for_bit(precision, d):
    """Row counts change every step (all of CHAIN_ROWS: no present stream is ever without rows); adamw, learnable scales.  Nine
    steps cover the row tables built two steps ahead, the 4-entry offsets window, both buffer parities and a full period of
    the resident-rows ring (NCH + 1 <= 6 regions)."""
    assert set(CHAIN_ROWS) <= set(R.PATTERNS) | set(R.PROBE_ROWS)
    tab = R.tables(d, R.PROBE_C, "op")
    s = tab["scale"]
    st = R.make_state(tab["W"], scales=(s, 0.75 * s))
    batches = _chain_batches(9, d)
    lrs = [1e-3 * (k + 1) / 9 for k in range(9)]
    kw = dict(wd=0.01, learn=True, precision=precision)
    one = _run(tab, d, R.PROBE_C, batches, st, "adamw", lrs, **kw)
    chain = _run(tab, d, R.PROBE_C, batches, st, "adamw", lrs, calls=[1] * 9, **kw)
    _same_bits(one, chain)
    assert not np.array_equal(one["W"], st["W"]) and np.isfinite(one["scalars"][:, :8]).all()


def test_515_steps_cross_the_launch_split_bit_for_bit():
    """One call of 515 steps (two launches: 512 + 3, the epoch parity carried across) == 515 calls of one step."""
    d, n = 128, 515
    tab = R.tables(d, R.PROBE_C, "op")
    st = R.make_state(tab["W"], scales=(tab["scale"], 0.75 * tab["scale"]))
    batches = _chain_batches(n, 515)
    lrs = [1e-3] * n
    kw = dict(wd=0.01, learn=True)
    one = _run(tab, d, R.PROBE_C, batches, st, "adamw", lrs, **kw)
    chain = _run(tab, d, R.PROBE_C, batches, st, "adamw", lrs, calls=[1] * n, **kw)
    _same_bits(one, chain)


def test_grouped_launch_of_heterogeneous_heads_equals_isolated_runs():
    """Seven heads of one width (d = 256) but 1 / 3 / 7 / 63 class slices, sgd / adam / adamw, learnable scales on and off, their
    own lr, decay and index streams: ONE grouped launch == seven isolated calls, bit for bit."""
    import umlh
    d, n = 256, 6
    heads = [(2, "sgd", False, 1e-2, 1e-3), (37, "adam", True, 1e-3, 0.01), (100, "adamw", False, 2e-3, 0.0), (1000, "adamw", True, 1e-3, 0.1),
             (37, "sgd", True, 5e-3, 0.0), (100, "adam", False, 1e-4, 0.001), (2, "adamw", True, 3e-3, 0.01)]

    def make(h, C, kind, learn, lr, wd):
        tab = R.tables(d, C, "op")
        e = umlh.HeadEngine(d, d, C, learnable_temp=learn, optimizer=kind, weight_decay=wd, max_rows_img=64, max_rows_txt=64, device=DEV)
        e.w_head.copy_(_T(tab["W"]))
        e.scales.copy_(_T(np.array([tab["scale"], 0.75 * tab["scale"]], np.float32)))
        ti, tt = _tables(tab, False)
        batches = _chain_batches(n, 1000 + h)
        sc = torch.zeros(n, umlh.N_SCALARS, device=DEV)
        return dict(engine=e, img_table=ti, img_index_batches=[_T(b[0], torch.int64) for b in batches], txt_table=tt,
                    txt_index_batches=[_T(b[1], torch.int64) for b in batches], lrs=[lr * (k + 1) / n for k in range(n)], first_step=3,
                    alpha=0.3 + 0.1 * h, img_alpha=1.0, scalars_out=sc)
    iso = [make(h, *cfg) for h, cfg in enumerate(heads)]
    for j in iso:
        kw = {k: v for k, v in j.items() if k != "engine"}
        j["engine"].train_steps(kw.pop("img_table"), kw.pop("img_index_batches"), kw.pop("txt_table"), kw.pop("txt_index_batches"),
                                kw.pop("lrs"), **kw)
    grp = [make(h, *cfg) for h, cfg in enumerate(heads)]
    umlh.train_steps_grouped(grp, n)
    torch.cuda.synchronize()
    for a, b in zip(iso, grp):
        ea, eb = a["engine"], b["engine"]
        assert ea.micro_status() == 0 and eb.micro_status() == 0 and ea.micro_launches() == 1 and eb.micro_launches() == 1
        for name in ("w_head", "m_head", "v_head", "scales", "m_scales", "v_scales"):
            assert np.array_equal(_bits(getattr(ea, name).cpu().numpy()), _bits(getattr(eb, name).cpu().numpy())), name
        assert np.array_equal(_bits(a["scalars_out"].cpu().numpy()), _bits(b["scalars_out"].cpu().numpy()))
        assert not np.array_equal(eb.w_head.cpu().numpy(), R.tables(d, eb.num_classes, "op")["W"])
