"""GPU: umlh_align_pairs / umlh.align.measure_pairs against the single-pair calls, word for word.  Every comparison is on the
bits (int64 / int32 views) of what align.cka_terms, align.knn(..., return_scores=True) and align.mutual_knn_lists give for the
same tensors and the same ``splits`` called alone; those are held to float64 and to the reference's values by test_align_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import _align_ref as R
from conftest import load_golden
from test_align_gpu import CASES, _tie_features, dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPLITS = (0, 1, 2, 7)
NAN64 = 0x7FF80000DEADBEEF          # a quiet NaN with a payload no kernel produces
NAN32 = 0x7FC0BEEF


def w64(t):
    return t.contiguous().view(torch.int64)


def w32(t):
    return t.contiguous().view(torch.int32)


def _view(x, layout):
    """x [n, d] on the device as: 'dense'; 'strided' (row stride d + pad, NaN in the padding); 'offset' (a view that starts 4 bytes
    into a 16-byte aligned buffer, so a width that is a multiple of 4 still takes the scalar load form)."""
    t = dev(x)
    if layout == "dense":
        return t
    n, d = t.shape
    lo, width = (0, d + (4 if d % 4 == 0 else 3)) if layout == "strided" else (1, d + 4)
    buf = torch.full((n, width), float("nan"), device=DEV)
    buf[:, lo:lo + d] = t
    return buf[:, lo:lo + d]


# n, d_a, d_b, topk (0: none), cka, layout of a, layout of b.  Load forms: d % 4, ld % 4 and the base address decide per view.
MEMBERS = [
    (6, 1, 1, 1, True, "dense", "dense"),                 # below one strip; scalar | scalar
    (33, 5, 33, 10, True, "dense", "dense"),              # one row over a strip
    (255, 32, 32, 32, True, "dense", "dense"),            # vector | vector, the widest list
    (256, 33, 100, 10, False, "strided", "strided"),      # mknn only; ld 36 and 104: scalar (d = 33) | vector
    (257, 128, 128, 10, True, "offset", "dense"),         # scalar (4-byte offset) | vector within one member
    (2000, 35, 300, 10, True, "dense", "dense"),          # eight tiles; scalar | vector
    (2000, 128, 128, 0, True, "strided", "dense"),        # CKA only
    (257, 32, 32, 1, True, "strided", "offset"),          # two tiles, k = 1
    (33, 128, 128, 32, True, "dense", "strided"),         # k = n - 1
]


def _features(n, d, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal((n, 4)) @ g.standard_normal((4, d)) + 0.5 * g.standard_normal((n, d))).astype(np.float32)


@pytest.fixture(scope="module")
def members():
    out = []
    for i, (n, da, db, k, cka, la, lb) in enumerate(MEMBERS):
        out.append((_view(_features(n, da, 100 + i), la), _view(_features(n, db, 200 + i), lb), {"topk": k, "cka": cka}))
    return out


def single(a, b, k, cka, splits):
    """What the single-pair calls give: (out5 words with None where nothing is asked, (knn_a, scores_a, knn_b, scores_b) or None)."""
    from umlh import align
    terms = w64(align.cka_terms(a, b, splits=splits)).tolist() if cka else [None] * 4
    if not k:
        return terms + [None], None
    ka, sa = align.knn(a, k, splits=splits, return_scores=True)
    kb, sb = align.knn(b, k, splits=splits, return_scores=True)
    return terms + [int(w64(align.mutual_knn_lists(ka, kb).reshape(1)))], (ka, sa, kb, sb)


_REFS = {}


def refs_for(members, splits):
    """The single-call results of the module's members, computed once per ``splits`` and never changed."""
    if splits not in _REFS:
        _REFS[splits] = [single(a, b, o["topk"], o["cka"], splits) for a, b, o in members]
    return _REFS[splits]


def same_as_single(out_row, lists, ref, what):
    want, want_lists = ref
    got = w64(out_row).tolist()
    for j, w in enumerate(want):
        if w is None:
            assert np.isnan(float(out_row[j])), (what, j)
        else:
            assert got[j] == w, (what, j, float(out_row[j]))
    assert (lists is None) == (want_lists is None), what
    if lists is not None:
        for got_t, want_t, name in zip(lists, want_lists, ("knn_a", "scores_a", "knn_b", "scores_b")):
            assert torch.equal(w32(got_t), w32(want_t)), (what, name)


@pytest.mark.parametrize("splits", SPLITS)
def test_heterogeneous_group_equals_the_single_calls(members, splits):
    from umlh import align
    out, lists = align.measure_pairs(members, splits=splits, return_lists=True)
    assert out.shape == (len(members), 5) and out.dtype == torch.float64 and out.is_cuda
    for i, ref in enumerate(refs_for(members, splits)):
        same_as_single(out[i], lists[i], ref, (splits, MEMBERS[i]))
    plain = align.measure_pairs(members, splits=splits)                       # the lists in scratch: the same five words
    assert torch.equal(w64(plain.nan_to_num(nan=-7.0)), w64(out.nan_to_num(nan=-7.0)))


@pytest.fixture(scope="module")
def seventy():
    """70 pairs at n = 257 (two tiles, nine strips) with their single-call results at automatic chunk counts."""
    g = torch.Generator().manual_seed(3)
    a = torch.randn(70, 257, 16, generator=g).to(DEV)
    b = (a[:, :, :8] * 0.5 + torch.randn(70, 257, 8, generator=g).to(DEV)).contiguous()
    pairs = [(a[i], b[i]) for i in range(70)]
    return pairs, [single(x, y, 10, True, 0) for x, y in pairs]


@pytest.mark.parametrize("count", [1, 2, 64, 70])
def test_group_sizes(seventy, count):
    """One member, two, the largest group of the C entry point, and 70 through the Python split (64 + 6)."""
    from umlh import align
    pairs, refs = seventy
    out, lists = align.measure_pairs(pairs[:count], return_lists=True)
    assert out.shape == (count, 5)
    for i in range(count):
        same_as_single(out[i], lists[i], refs[i], (count, i))


def test_members_do_not_depend_on_their_group(members):
    from umlh import align
    for splits in (0, 2):
        full, full_l = align.measure_pairs(members, splits=splits, return_lists=True)
        rev, rev_l = align.measure_pairs(members[::-1], splits=splits, return_lists=True)
        for i, m in enumerate(members):
            alone, alone_l = align.measure_pairs([m], splits=splits, return_lists=True)
            j = len(members) - 1 - i
            for other, other_l in ((alone[0], alone_l[0]), (rev[j], rev_l[j])):
                assert torch.equal(w64(full[i].nan_to_num(nan=-7.0)), w64(other.nan_to_num(nan=-7.0))), (splits, i)
                assert (full_l[i] is None) == (other_l is None)
                for t, u in zip(full_l[i] or (), other_l or ()):
                    assert torch.equal(w32(t), w32(u)), (splits, i)


def test_a_nan_row_stays_inside_its_member(members):
    """A member with a NaN row changes no word of any other member; its own lists carry the sentinels of the single call.

    The words of a list that no column fills depend on how many column chunks were merged into it (topk_merge keeps one sentinel
    run per chunk), between two single calls as well.  With ``splits`` given both forms merge that many chunks.  With splits = 0
    the group's count follows from the strips of all its views (the contract of include/umlh.h): ceil(512 / total strips), at
    most one per tile; the single call it has to match is the one made with that count."""
    from umlh import align
    bad = 5                                                        # the (2000, 35, 300) member
    a, b, o = members[bad]
    an = a.clone()
    an[13] = float("nan")
    poisoned = list(members)
    poisoned[bad] = (an, b, o)
    for splits in (0, 2):
        clean, clean_l = align.measure_pairs(members, splits=splits, return_lists=True)
        out, lists = align.measure_pairs(poisoned, splits=splits, return_lists=True)
        for i in range(len(members)):
            if i == bad:
                continue
            assert torch.equal(w64(out[i].nan_to_num(nan=-7.0)), w64(clean[i].nan_to_num(nan=-7.0))), (splits, i)
            for t, u in zip(lists[i] or (), clean_l[i] or ()):
                assert torch.equal(w32(t), w32(u)), (splits, i)
        chunks = splits
        if splits == 0:
            strips = sum(2 * ((x.shape[0] + 31) // 32) for x, _, oo in members if oo["topk"])
            chunks = min(-(-512 // strips), (an.shape[0] + 255) // 256)
            assert chunks == 3                                     # 204 strips; the member alone would take all 8 tiles
        want_terms, _ = single(an, b, 0, True, splits)
        want_knn, want_lists = single(an, b, o["topk"], False, chunks)
        same_as_single(out[bad], lists[bad], (want_terms[:4] + want_knn[4:], want_lists), ("nan member", splits))
        ka, sa = lists[bad][0].cpu().numpy(), lists[bad][1].cpu().numpy()
        assert (ka[13] >= 2000).all() and (sa[13] == -np.inf).all() and not (np.delete(ka, 13, 0) == 13).any()
        assert np.isnan(float(out[bad, 0]))


def _raw_call(members, splits, guard=4096):
    """umlh_align_pairs itself on pattern-filled buffers one slot longer than needed and a scratch with a guard region behind the
    queried size.  Returns (out [G, 6] int64 words, per member the four list buffers as int32 words, the guard bytes)."""
    import umlh
    from umlh._lib import AlignPair
    lib = umlh.load_library()
    items = (AlignPair * len(members))()
    out = torch.full((len(members), 6), NAN64, dtype=torch.int64, device=DEV)
    lists = []
    for i, (it, (a, b, o)) in enumerate(zip(items, members)):
        n, k = a.shape[0], o["topk"]
        it.a, it.lda, it.d_a, it.b, it.ldb, it.d_b = a.data_ptr(), a.stride(0), a.shape[1], b.data_ptr(), b.stride(0), b.shape[1]
        it.n, it.cka, it.topk, it.out5 = n, int(o["cka"]), k, out[i].data_ptr()
        bufs = [torch.full((n * k + 1,), NAN32, dtype=torch.int32, device=DEV) for _ in range(4)] if k else None
        if k:
            it.knn_a, it.scores_a, it.knn_b, it.scores_b = (t.data_ptr() for t in bufs)
        lists.append(bufs)
    nbytes = lib.umlh_align_pairs_scratch(items, len(members), splits)
    assert nbytes > 0 and nbytes % 256 == 0
    scratch = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    rc = lib.umlh_align_pairs(items, len(members), splits, scratch.data_ptr(), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.umlh_last_error()
    torch.cuda.synchronize()
    return out, lists, scratch[nbytes:]


@pytest.mark.parametrize("splits", (0, 3))
def test_nothing_is_written_outside_what_a_member_asks_for(members, splits):
    out, lists, guard = _raw_call(members, splits)
    assert (guard == 0xA5).all()
    for i, ((a, b, o), (want, want_lists)) in enumerate(zip(members, refs_for(members, splits))):
        row = out[i].tolist()
        assert row[5] == NAN64, i                                            # the slot behind out5
        for j, w in enumerate(want):
            assert row[j] == (NAN64 if w is None else w), (i, j)             # untouched where the member skips a metric
        if lists[i] is not None:
            nk = a.shape[0] * o["topk"]
            for buf, want_t in zip(lists[i], want_lists):
                assert int(buf[nk]) == NAN32, i
                assert torch.equal(buf[:nk], w32(want_t).reshape(-1)), i


def test_ties_follow_score_desc_index_asc_in_a_group():
    """Integer-valued features, every score exact and many ties: each member's lists are numpy's lexsort (score desc, index asc),
    for any ``splits``.  The construction of test_ties_follow_score_desc_index_asc_for_any_splits, four shapes in one group."""
    from umlh import align
    shapes = [(300, 3, 10), (1000, 5, 32), (777, 2, 7), (64, 1, 5)]
    pairs, want = [], []
    for n, d, k in shapes:
        x = _tie_features(n, d, n + d)
        full = x.astype(np.float64) @ x.T.astype(np.float64)
        np.fill_diagonal(full, -np.inf)
        wi = np.stack([np.lexsort((np.arange(n), -full[r]))[:k] for r in range(n)])
        want.append((wi, np.take_along_axis(full, wi, 1).astype(np.float32)))
        xd = dev(x)
        pairs.append((xd, xd, {"topk": k, "cka": False}))
    for splits in (1, 2, 7, 0):
        out, lists = align.measure_pairs(pairs, splits=splits, return_lists=True)
        for (wi, ws), (ka, sa, kb, sb), row in zip(want, lists, out):
            for i_, s_ in ((ka, sa), (kb, sb)):
                np.testing.assert_array_equal(i_.cpu().numpy(), wi, err_msg=f"splits={splits}")
                np.testing.assert_array_equal(s_.cpu().numpy(), ws, err_msg=f"splits={splits}")
            assert float(row[4]) == 1.0 and np.isnan(float(row[0]))           # a view against itself


def test_streams_and_repetition(members):
    """The call is enqueued on the CURRENT stream (read after synchronising that stream alone), two streams give the same words,
    and three calls in a row -- more than the staging ring has buffers -- give the same words each time."""
    from umlh import align
    want = w64(align.measure_pairs(members).nan_to_num(nan=-7.0)).cpu()
    for _ in range(3):
        assert torch.equal(w64(align.measure_pairs(members).nan_to_num(nan=-7.0)).cpu(), want)
    sides = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    got = []
    for s in sides:
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got.append(align.measure_pairs(members))
    for s, g in zip(sides, got):
        s.synchronize()
        assert torch.equal(w64(g.nan_to_num(nan=-7.0)).cpu(), want)
    back_to_back = [align.measure_pairs(members[:3]) for _ in range(3)]       # no host wait in between
    torch.cuda.synchronize()
    assert all(torch.equal(w64(t), w64(back_to_back[0])) for t in back_to_back)


def test_golden_cases_as_one_group():
    """The six golden cases in one call, held to what test_golden_cka and test_golden_neighbours_and_mutual_knn of
    test_align_gpu.py hold the single calls to (their cases, their reference, their expressions)."""
    from umlh import align
    gold = load_golden("alignment")
    for k in (1, 10, 32):
        pairs = [(dev(gold[f"{c}/a"]), dev(gold[f"{c}/b"])) for c in CASES]
        out, lists = align.measure_pairs(pairs, topk=k, return_lists=True)
        got = out.cpu().numpy()
        for i, case in enumerate(CASES):
            c64, ref = gold[f"{case}/cka64"], float(gold[f"{case}/ref_cka"])
            assert abs(got[i, 0] - c64[0]) <= 1e-5, (case, got[i, 0], c64[0])
            assert abs(got[i, 0] - ref) <= 1e-5 + abs(ref - c64[0]), (case, got[i, 0], ref)
            np.testing.assert_allclose(got[i, 1:4], c64[1:], rtol=1e-5)
            und, n = int(gold[f"{case}/undecidable"]), pairs[i][0].shape[0]
            assert abs(got[i, 4] - float(gold[f"{case}/ref_mknn_k{k}"])) <= 1e-6 + und / n, (case, k, got[i, 4])
            assert abs(got[i, 4] - float(gold[f"{case}/mknn64_k{k}"])) <= 1e-12 + und / n, (case, k, got[i, 4])
            if k == 10:
                for v, lst in (("a", lists[i][0]), ("b", lists[i][2])):
                    x = gold[f"{case}/{v}"]
                    _, s64 = R.knn64(x, 10)
                    ok = R.list_decidable(s64, R.tau(x), 10)
                    np.testing.assert_array_equal(lst.cpu().numpy()[ok], gold[f"{case}/ref_knn_{v}"][ok])


# ---------------------------------------------------------------------------------------------------------------------------- #
# callers
# ---------------------------------------------------------------------------------------------------------------------------- #
def _lone_run_with_single_calls(point, steps):
    """One grid point alone, an evaluation after every step, the alignment metrics through the single-pair calls."""
    from gaussian import sweep
    from gaussian.fused import FusedTrainer
    from umlh import align
    _, _, val = sweep.make_data(point)
    ds, gen, model, opt = sweep.build_point(point, DEV)
    trainer = FusedTrainer(model, opt, ds, point["batch_size"], gen, DEV, span_steps=steps, total_steps=steps)
    vx, vy = val["x"].to(device=DEV, dtype=torch.float32), val["y"].to(device=DEV, dtype=torch.float32)
    cka, mknn = [], []
    for _ in range(steps):
        trainer.steps(1, mode=point["mode"], alpha_x=1.0, alpha_y=point["alpha_y"])
        _, ex, ey = trainer.evaluate(vx, vy, embeddings=True)
        cka.append(align.cka(ex, ey)); mknn.append(align.mutual_knn(ex, ey, 10))
    return [float(t) for t in torch.stack(cka).cpu()], [float(t) for t in torch.stack(mknn).cpu()]


def test_sweep_and_single_run_log_the_bits_of_the_single_calls():
    from gaussian import sweep
    from gaussian.train import train_model_steps_fused
    grid = dict(dim_obs=12, dim_common=16, dim_latent=4, train_num_samples=64, batch_size=16, val_num_samples=40, num_steps=6, lr=1e-3,
                seed=[0, 1, 2], mode="xy", alpha_y=0.5)
    points = [sweep._full(p) for p in sweep.expand_grid(grid)]
    assert len(points) == 3
    logs = sweep.sweep_grouped(points, eval_every=1, alignment=True, device=DEV)
    for point, log in zip(points, logs):
        cka, mknn = _lone_run_with_single_calls(point, 6)
        assert len(log["val_cka"]) == 6 and log["val_cka"] == cka and log["val_mknn"] == mknn, point
        _, _, val = sweep.make_data(point)
        ds, gen, lone, opt = sweep.build_point(point, DEV)
        ref = train_model_steps_fused(lone, ds, opt, 6, val["x"], val["y"], DEV, batch_size=16, generator=gen, mode="xy", alpha_x=1.0,
                                      alpha_y=0.5, eval_every=1, alignment=True)
        assert set(ref) == set(log) and all(ref[k] == log[k] for k in ref), point
    assert len({tuple(log["val_cka"]) for log in logs}) == 3


def test_embedding_capture_logs_the_bits_of_the_seven_single_calls():
    import umlh
    from multibench.capture import EmbeddingCapture, take_fixed_samples
    from test_capture_gpu import _small_loaders, _small_model
    model = _small_model(0).train()
    l1, l2 = _small_loaders()
    cap = EmbeddingCapture(take_fixed_samples(l1, l2, [0, 2], "mosi"), DEV)
    res, _, _ = cap.measure(model)
    m = cap.matrices
    clip = lambda v: max(min(v, 1.0), 0.0)
    cka, mknn = umlh.align.cka, lambda a, b: umlh.align.mutual_knn(a, b, topk=10)
    want = {"val/cka_proj": clip(float(cka(m["x_proj"], m["y_proj"]))), "val/mknn_proj": float(mknn(m["x_proj"], m["y_proj"])),
            "val/cka_embed": clip(float(cka(m["zx"], m["zy"]))), "val/mknn_embed": float(mknn(m["zx"], m["zy"])),
            "val/cka_out": clip(float(cka(m["x_recon"], m["y_recon"]))), "val/mknn_out": float(mknn(m["x_recon"], m["y_recon"])),
            "val/cka_text_embeddings_features": clip(float(cka(m["zy"], cap.raw_y)))}
    for k, v in want.items():
        assert res[k] == v and np.isfinite(v), (k, res[k], v)
