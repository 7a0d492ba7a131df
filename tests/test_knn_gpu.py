"""GPU: the k-nearest-neighbour probe (umlh_knn_search / umlh_knn_vote, umlh.KNeighborsProbe, the 'knn' classifier type of
multibench.train.evaluate) against the float64 restatement tests/_knn_ref.py and what scikit-learn recorded in
tests/golden/knn_probe*.npz.

A query is compared list for list where it is sharp (tests/_knn_ref.py: the gap between its k-th and (k+1)-th squared distance
exceeds TAU x scale); a non-sharp query must still return neighbours no farther than d2_(k) + TAU x scale, ordered by the float64
(value, index).  On integer-valued data everything is exact and no allowance is made.  Measured figures are printed before they
are asserted (scripts/bench_knn.py writes them to profiles/knn_accuracy.txt)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _knn_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ["a600x40_k5", "b1000x35_k5", "c900x64_c10_k5", "d700x33_k1", "d700x33_k24", "e513x7_k8"]
IDX_FILL, PRED_FILL = -77, -55


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def golden():
    g = load_golden("knn_probe")
    return {tag: {k.split("::", 1)[1]: v for k, v in g.items() if k.startswith(tag + "::")} for tag in CASES}


def search(train, query, k, splits=0, want_dist=True):
    """umlh_knn_search through ctypes on fp32 device matrices (views with a row stride are used in place).  The outputs sit in
    sentinel-filled buffers one row longer than needed: everything must be written, nothing behind it."""
    from umlh._lib import check, load_library
    lib = load_library()
    (nt, d), nq = train.shape, query.shape[0]
    assert train.stride(1) == 1 and query.stride(1) == 1 and query.shape[1] == d
    nbytes = lib.umlh_knn_scratch_bytes(nt, nq, d, k, splits)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    idx = torch.full((nq + 1, k), IDX_FILL, dtype=torch.int32, device=DEV)
    dist = torch.full((nq + 1, k), -3.0, dtype=torch.float32, device=DEV) if want_dist else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.umlh_knn_search(train.data_ptr(), nt, train.stride(0), query.data_ptr(), nq, query.stride(0), d, k, splits, idx.data_ptr(),
                              dist.data_ptr() if want_dist else None, scratch.data_ptr(), nbytes, st), "umlh_knn_search")
    torch.cuda.current_stream().synchronize()
    assert (idx[nq] == IDX_FILL).all() and (not want_dist or (dist[nq] == -3.0).all())
    return idx[:nq], (dist[:nq] if want_dist else None)


def vote(idx, labels, y=None):
    from umlh._lib import check, load_library
    nq, k = idx.shape
    idx = idx.contiguous()
    pred = torch.full((nq + 1,), PRED_FILL, dtype=torch.int32, device=DEV)
    votes = torch.full((nq + 1,), PRED_FILL, dtype=torch.int32, device=DEV)
    correct = torch.full((2,), -9, dtype=torch.int64, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(load_library().umlh_knn_vote(idx.data_ptr(), nq, k, labels.data_ptr(), labels.numel(), None if y is None else y.data_ptr(),
                                       pred.data_ptr(), votes.data_ptr(), None if y is None else correct.data_ptr(), st), "umlh_knn_vote")
    torch.cuda.current_stream().synchronize()
    assert pred[nq] == PRED_FILL and votes[nq] == PRED_FILL and correct[1] == -9
    return pred[:nq].cpu().numpy(), votes[:nq].cpu().numpy(), (None if y is None else int(correct[0]))


def check_against_restatement(what, q, t, k, idx, dist, sk_idx=None):
    """The list rules of the module docstring; returns the sharp mask.  ``sk_idx``: sklearn's recorded lists."""
    nq, nt = len(q), len(t)
    assert idx.shape == (nq, k) and idx.min() >= 0 and idx.max() < nt, what
    d2 = R.sqdist(q, t)
    want_d2, want_idx = R.kneighbors(q, t, k)
    sharp = R.sharp(q, t, k)
    got_d2 = np.take_along_axis(d2, idx.astype(np.int64), 1)
    assert np.array_equal(idx[sharp], want_idx[sharp]), what
    if sk_idx is not None:
        assert np.array_equal(idx[sharp], sk_idx[sharp]), what
    rel = np.abs(dist.astype(np.float64) - np.sqrt(got_d2)) / np.maximum(np.sqrt(got_d2), 1e-300)
    rel[got_d2 == 0] = np.abs(dist[got_d2 == 0])
    blunt = ~sharp
    print(f"{what}: non-sharp {int(blunt.sum())} of {nq}, worst dist error 2^{np.log2(max(rel.max(), 2.0 ** -60)):.1f}")
    assert rel.max() <= 2.0 ** -22, what
    if blunt.any():
        bound = want_d2[blunt, k - 1] + R.TAU * R.scale(q, t)[blunt]
        assert (got_d2[blunt] <= bound[:, None]).all(), what
        for row_d2, row_idx in zip(got_d2[blunt], idx[blunt]):
            assert len(set(row_idx.tolist())) == k, what
            assert np.array_equal(np.lexsort((row_idx, row_d2)), np.arange(k)), what
    return sharp


# ---- 1. the recorded cases through the C ABI ----
@pytest.mark.parametrize("tag", CASES)
def test_golden_cases(golden, tag):
    g = golden[tag]
    k, t, q, yt, yq = int(g["k"]), g["train"], g["query"], g["train_labels"], g["query_labels"]
    idx_d, dist_d = search(dev(t), dev(q), k)
    idx, dist = idx_d.cpu().numpy(), dist_d.cpu().numpy()
    sharp = check_against_restatement(tag, q, t, k, idx, dist, sk_idx=g["idx"])
    assert (~sharp).sum() <= R.CAP * len(q)
    pred, votes, correct = vote(idx_d, dev(yt), dev(yq))
    want_pred, want_votes = R.vote(yt[idx])                                      # the vote over the RETURNED lists: exact
    assert np.array_equal(pred, want_pred) and np.array_equal(votes, want_votes)
    assert np.array_equal(pred[sharp], g["pred"][sharp])
    assert correct == int((pred == yq).sum())
    if sharp.all():
        assert correct / len(q) == float(g["score"])
    # the same matrices as views with a row stride (a multiple of 4 floats: the vector-load path) give the same bits
    wide_t, wide_q = torch.full((len(t), t.shape[1] + 4), float("nan"), device=DEV), torch.full((len(q), q.shape[1] + 4), float("inf"), device=DEV)
    wide_t[:, :t.shape[1]] = dev(t)
    wide_q[:, :q.shape[1]] = dev(q)
    idx2, dist2 = search(wide_t[:, :t.shape[1]], wide_q[:, :q.shape[1]], k)
    assert torch.equal(idx2, idx_d) and torch.equal(dist2, dist_d)


# ---- 2. exact ties ----
@pytest.mark.parametrize("k", [5, 24])
def test_exact_ties_on_integer_features(k):
    t, yt, q, yq = R.integer_case()
    idx_d, dist_d = search(dev(t), dev(q), k)
    want_d2, want_idx = R.kneighbors(q, t, k)
    ties = int((np.sort(R.sqdist(q, t), 1)[:, k - 1] == np.sort(R.sqdist(q, t), 1)[:, k]).sum())
    print(f"k={k}: {ties} of {len(q)} queries have d2_(k) == d2_(k+1)")
    assert ties > len(q) // 2
    assert np.array_equal(idx_d.cpu().numpy(), want_idx)
    assert np.array_equal(dist_d.cpu().numpy(), np.sqrt(want_d2).astype(np.float32))
    pred, votes, correct = vote(idx_d, dev(yt), dev(yq))
    want_pred, want_votes = R.vote(yt[want_idx])
    assert not np.array_equal(R.vote(yt[want_idx], larger_label=True)[0], want_pred)      # count ties occur
    assert np.array_equal(pred, want_pred) and np.array_equal(votes, want_votes) and correct == int((want_pred == yq).sum())


# ---- 3. edges ----
EDGES = [  # n_query, n_train, d, k
    (1, 5, 1, 5), (33, 5, 7, 5), (97, 5, 33, 5),                                  # n_train == k < kc
    (1, 255, 7, 1), (33, 257, 33, 24), (97, 2048, 1, 1), (33, 2048, 7, 24), (97, 255, 33, 5), (1, 257, 1, 24), (97, 257, 7, 5),
]


@pytest.mark.parametrize("nq,nt,d,k", EDGES)
def test_edges_are_bitwise_independent_of_splits_calls_and_streams(nq, nt, d, k):
    rng = np.random.default_rng(1000 * nq + nt + d + k)
    t, q = rng.standard_normal((nt, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
    labels = rng.choice(np.array([0, 7, 999], np.int32), nt)
    # row-strided views whose padding columns hold NaN and Inf
    wt, wq = torch.full((nt, d + 3), float("nan"), device=DEV), torch.full((nq, d + 2), float("inf"), device=DEV)
    wt[:, :d], wq[:, :d] = dev(t), dev(q)
    tv, qv = wt[:, :d], wq[:, :d]
    base_i, base_d = search(tv, qv, k, splits=1)
    for splits in (2, 3, 0, 1):                                                  # (1 again: a second call)
        i2, d2 = search(tv, qv, k, splits=splits)
        assert torch.equal(i2, base_i) and torch.equal(d2.view(torch.int32), base_d.view(torch.int32)), splits
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        i3, d3 = search(tv, qv, k, splits=2)
    side.synchronize()
    assert torch.equal(i3, base_i) and torch.equal(d3.view(torch.int32), base_d.view(torch.int32))
    i4, _ = search(dev(t), dev(q), k, want_dist=False)                           # dense, no distances
    assert torch.equal(i4, base_i)
    idx = base_i.cpu().numpy()
    check_against_restatement(f"edge nq={nq} nt={nt} d={d} k={k}", q, t, k, idx, base_d.cpu().numpy())
    pred, votes, _ = vote(base_i, dev(labels))
    want_pred, want_votes = R.vote(labels[idx])
    assert np.array_equal(pred, want_pred) and np.array_equal(votes, want_votes) and set(pred.tolist()) <= {0, 7, 999}


# ---- 4. every index stays in range on bad data ----
def test_indices_stay_in_range_with_nan_rows():
    rng = np.random.default_rng(7)
    nt, nq, d, k = 300, 70, 9, 5
    t, q = rng.standard_normal((nt, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
    clean_i, clean_d = search(dev(t), dev(q), k)
    clean_i, clean_d = clean_i.cpu().numpy(), clean_d.cpu().numpy()
    # one query row of NaNs: that row's list is in range, every other row is as before
    qn = q.copy()
    qn[13] = np.nan
    i1, d1 = search(dev(t), dev(qn), k)
    i1, d1 = i1.cpu().numpy(), d1.cpu().numpy()
    assert i1.min() >= 0 and i1.max() < nt
    assert np.array_equal(i1[13], np.arange(k)) and np.isnan(d1[13]).all()       # a fully open list: its own positions, NaN
    others = np.arange(nq) != 13
    assert np.array_equal(i1[others], clean_i[others]) and np.array_equal(d1[others], clean_d[others])
    pred, _, _ = vote(dev(i1), dev(np.zeros(nt, np.int32)))
    assert (pred == 0).all()
    # one train row of NaNs: in range everywhere; rows whose clean lists do not hold that train row are as before
    poisoned = int(clean_i[0, 0])
    tn = t.copy()
    tn[poisoned] = np.nan
    i2, d2 = search(dev(tn), dev(q), k)
    i2, d2 = i2.cpu().numpy(), d2.cpu().numpy()
    assert i2.min() >= 0 and i2.max() < nt
    free = ~(clean_i == poisoned).any(1)
    assert 0 < free.sum() < nq
    assert np.array_equal(i2[free], clean_i[free]) and np.array_equal(d2[free], clean_d[free])
    assert not (i2[free] == poisoned).any()
    # n_train < k + 8 with a NaN query row: the lists are shorter than the candidate width
    i3, d3 = search(dev(t[:6]), dev(qn[:20]), 5)
    i3, d3 = i3.cpu().numpy(), d3.cpu().numpy()
    assert i3.min() >= 0 and i3.max() < 6
    assert np.array_equal(i3[13], np.arange(5)) and np.isnan(d3[13]).all()
    want = R.kneighbors(q[:20], t[:6], 5)[1]
    assert np.array_equal(np.delete(i3, 13, 0), np.delete(want, 13, 0))


def test_nan_train_row_with_n_train_equal_k_leaves_one_slot_open():
    """n_train == k and one train row of NaNs: four finite neighbours in the float64 order, then position 4 as an open slot (its
    own index, a NaN distance).  The probe's twin of the k = C NaN-weight case of tests/test_evalreport_gpu.py."""
    rng = np.random.default_rng(8)
    nt = k = 5
    t, q = rng.standard_normal((nt, 3)).astype(np.float32), rng.standard_normal((3, 3)).astype(np.float32)
    t[2] = np.nan
    idx, dist = search(dev(t), dev(q), k)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    finite = np.array([0, 1, 3, 4])
    want_d2, order = R.kneighbors(q, t[finite], 4)
    assert np.array_equal(idx[:, :4], finite[order])
    want = np.sqrt(want_d2)
    assert (np.abs(dist[:, :4] - want) <= 2.0 ** -22 * want).all()
    assert (idx[:, 4] == 4).all() and np.isnan(dist[:, 4]).all()


# ---- 5. the Python class ----
def test_kneighbors_probe(golden):
    import umlh
    g = golden["c900x64_c10_k5"]
    t, q, yt, yq = g["train"], g["query"], g["train_labels"], g["query_labels"]
    pr = umlh.KNeighborsProbe().fit(dev(t), dev(yt))
    assert pr.n_neighbors == 5
    dist, idx = pr.kneighbors(dev(q))
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.is_cuda and idx.is_cuda
    sharp = R.sharp(q, t, 5)
    assert np.array_equal(idx.cpu().numpy()[sharp], g["idx"][sharp])
    assert torch.equal(pr.kneighbors(dev(q), return_distance=False), idx)
    pred = pr.predict(dev(q))
    assert pred.dtype == torch.int64 and np.array_equal(pred.cpu().numpy(), R.vote(yt[idx.cpu().numpy()])[0])
    qd, yqd = dev(q), dev(yq)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        correct = pr.correct(qd, yqd)                                            # enqueues only
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert correct.dtype == torch.int64 and correct.ndim == 0 and correct.is_cuda
    score = pr.score(dev(q), dev(yq))
    assert isinstance(score, float) and score == int(correct) / len(q) == float((pred.cpu().numpy() == yq).mean())
    if sharp.all():
        assert score == float(g["score"])
    # host / strided / fp64 inputs, as LogisticProbe takes them
    padded = dev(np.concatenate([t, t + 1.0], axis=1))[:, :t.shape[1]]            # row stride 2 d, used in place
    assert padded.data_ptr() == umlh.KNeighborsProbe().fit(padded, yt)._x.data_ptr()
    for probe, queries in ((umlh.KNeighborsProbe().fit(padded, dev(yt)), dev(q)),
                           (umlh.KNeighborsProbe(splits=3).fit(torch.from_numpy(t).double(), torch.from_numpy(yt).long()), torch.from_numpy(q)),
                           (pr, dev(q).double()), (pr, dev(q).t().contiguous().t())):
        d2, i2 = probe.kneighbors(queries)
        assert torch.equal(i2, idx) and torch.equal(d2, dist)
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        umlh.KNeighborsProbe(n_neighbors=7).fit(dev(t[:6]), dev(yt[:6]))
    with pytest.raises(ValueError):
        pr.predict(dev(q[:, :-1]))
    with pytest.raises(ValueError):
        pr.fit(dev(t), dev(yt[:-1]))
    with pytest.raises(ValueError):
        umlh.KNeighborsProbe(n_neighbors=25)
    with pytest.raises(umlh.UmlhError):
        umlh.KNeighborsProbe().predict(dev(q))


# ---- 6. multibench.train.evaluate(classifier_types=...) ----
def _model(name):
    from multibench.models import Linear, Transformer, UML
    g = load_golden(name)
    z, dx, dy, B, T, pe, pl = (int(v) for v in g["cfg"])
    m = UML(Linear(dx, z), Linear(dy, z), Transformer(z, z, nhead=5, num_layers=5, conv1d=True, out_last=False,
                                                       pos_embd=bool(pe), pos_learnable=bool(pl), max_len=128),
            [Linear(z, dx), Linear(z, dy)], modality="xy")
    m.load_state_dict({k[4:]: torch.as_tensor(g[k]) for k in g.files if k.startswith("sd::")})
    return m.to(DEV)


def _config(g, freq=2):
    bs, cfg = int(g["batch_size"]), {"freq": freq}
    for t in ("train", "val", "test"):
        x, y, lx, ly, lab = (torch.from_numpy(g[f"{k}_{t}"]) for k in ("x", "y", "lx", "ly", "labels"))
        cfg[t] = [([x[s:s + bs], None, y[s:s + bs]], [lx[s:s + bs], None, ly[s:s + bs]], torch.arange(s, min(s + bs, len(x))),
                   lab[s:s + bs].reshape(-1, 1)) for s in range(0, len(x), bs)]
    return cfg


@pytest.mark.parametrize("tag", ["mosi", "humor"])
def test_evaluate_with_the_knn_classifier(tag):
    from multibench.train import evaluate
    g = load_golden("probe_e2e_" + tag)
    ds, cfg = str(g["ds_name"]), _config(g)
    model = _model(str(g["model"]))
    plain = evaluate(model, cfg, ds, device=DEV)
    assert evaluate(model, cfg, ds, device=DEV, classifier_types=("logistic",)) == pytest.approx(plain, nan_ok=True, abs=0)
    res, emb, clfs = evaluate(model, cfg, ds, device=DEV, return_embeddings=True, classifier_types=("knn",))
    assert set(res) == set(plain) and len(clfs) == 6
    for k in plain:                                                              # everything but the six scores is untouched
        if "score_x" not in k and "score_y" not in k:
            assert res[k] == pytest.approx(plain[k], nan_ok=True, abs=0), k
    e = {t: emb[t].cpu().numpy() for t in ("train", "val", "test")}
    z = e["train"].shape[1] // 2
    for name, cols in (("x", slice(0, z)), ("y", slice(z, 2 * z)), ("xy", slice(0, 2 * z))):
        for t in ("val", "test"):
            xt, xh, yh = e["train"][:, cols], e[t][:, cols], g["y01_" + t]
            want = float((R.predict(xh, xt, g["y01_train"], 5) == yh).mean())
            blunt = int((~R.sharp(xh, xt, 5)).sum())
            key = f"{t}/score_{name}"
            print(f"{tag} {key}: knn {res[key]:.4f} float64 {want:.4f} (non-sharp {blunt} of {len(yh)}), logistic {plain[key]:.4f}")
            assert abs(res[key] - want) <= blunt / len(yh) + 1e-12
    # a later type overwrites an earlier one's keys; the fitted probes of both are returned
    both, _, clfs2 = evaluate(model, cfg, ds, device=DEV, return_embeddings=True, classifier_types=("logistic", "knn"))
    assert both == pytest.approx(res, nan_ok=True, abs=0) and len(clfs2) == 9
    with pytest.raises(ValueError, match="Unsupported classifier type: svm"):
        evaluate(model, cfg, ds, device=DEV, classifier_types=("svm",))
