"""No-GPU checks of the k-nearest-neighbour probe: the entry points exist at ABI v11 and reject every envelope violation before
any HIP call; the float64 restatement tests/_knn_ref.py reproduces what scikit-learn recorded in tests/golden/knn_probe*.npz on
every row; five deliberately wrong restatements are told apart; the sharpness constant and the non-sharp cap hold from the
reference side alone."""
import ctypes as C
import math

import numpy as np
import pytest

import _knn_ref as R
from conftest import load_golden

E_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


@pytest.fixture(scope="module")
def golden():
    g = load_golden("knn_probe")
    return {str(tag): {k.split("::", 1)[1]: v for k, v in g.items() if k.startswith(str(tag) + "::")} for tag in g["cases"]}


def test_symbols_exist_and_the_version_stays(lib):
    from umlh import _lib
    assert lib.umlh_version() == 11
    for name in ("umlh_knn_scratch_bytes", "umlh_knn_search", "umlh_knn_vote"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    import umlh
    assert umlh.KNeighborsProbe is umlh.probe.KNeighborsProbe


def test_envelope_violations_are_invalid_before_any_hip_call(lib):
    fake = C.c_void_p(256)                                   # never dereferenced: every check comes first
    big = 1 << 40

    def search(nt=100, ldt=8, nq=10, ldq=8, d=8, k=5, splits=0, train=fake, query=fake, idx=fake, scratch=fake, nbytes=big):
        return lib.umlh_knn_search(train, nt, ldt, query, nq, ldq, d, k, splits, idx, None, scratch, nbytes, None)

    for kw in (dict(k=0), dict(k=25), dict(k=5, nt=4), dict(d=0), dict(ldt=7), dict(ldq=7), dict(splits=-1), dict(nq=0),
               dict(nt=1 << 31), dict(nq=1 << 31), dict(train=None), dict(query=None), dict(idx=None), dict(scratch=None),
               dict(nbytes=16)):
        assert search(**kw) == E_INVALID, kw
        assert b"umlh_knn_search" in lib.umlh_last_error(), kw

    def vote(nq=10, k=5, nt=100, idx=fake, labels=fake, y=fake, pred=fake, votes=None, correct=None):
        return lib.umlh_knn_vote(idx, nq, k, labels, nt, y, pred, votes, correct, None)

    for kw in (dict(k=0), dict(k=25), dict(nq=0), dict(nt=0), dict(idx=None), dict(labels=None), dict(pred=None),
               dict(y=None, correct=fake), dict(nt=1 << 31)):
        assert vote(**kw) == E_INVALID, kw
        assert b"umlh_knn_vote" in lib.umlh_last_error(), kw


def test_scratch_queries(lib):
    q = lib.umlh_knn_scratch_bytes
    for args in ((100, 10, 8, 0, 0), (100, 10, 8, 25, 0), (4, 10, 8, 5, 0), (100, 10, 0, 5, 0), (100, 10, 8, 5, -1), (100, 0, 8, 5, 0),
                 (1 << 31, 10, 8, 5, 0), (0, 10, 8, 5, 0)):
        assert q(*args) == 0, args
    assert q(5, 1, 1, 5, 0) > 0                                                  # n_train == k
    assert q(4096, 64, 8, 5, 1) < q(4096, 64, 8, 5, 2) < q(4096, 64, 8, 5, 4)    # grows with splits
    assert q(4096, 64, 8, 5, 16) == q(4096, 64, 8, 5, 1000)                      # (at most one chunk per 256-column tile)
    # no n_query * n_train term: a million by a million is the lists (kc <= 32 entries of two words per chunk and query, plus the
    # candidates) and one float per train row
    n = 10 ** 6
    for splits in (0, 1, 8):
        got = q(n, n, 1024, 24, splits)
        assert 0 < got <= n * 32 * 4 * (2 * max(splits, 1) + 1) + n * 4 + 4 * 256, (splits, got)
    assert q(n, n, 1024, 24, 8) > q(n, n, 1024, 24, 1) >= n * 32 * 4 * 3


def test_restatement_reproduces_sklearn_on_every_row(golden):
    for tag, g in golden.items():
        k = int(g["k"])
        d2, idx = R.kneighbors(g["query"], g["train"], k)
        assert np.array_equal(idx, g["idx"]), tag
        np.testing.assert_allclose(np.sqrt(d2), g["dist"], rtol=1e-6, atol=0, err_msg=tag)
        pred, _ = R.vote(g["train_labels"][idx])
        assert np.array_equal(pred, g["pred"]), tag
        assert float((pred == g["query_labels"]).mean()) == float(g["score"]), tag
        assert 0.5 <= float(g["score"]) <= 0.8, tag                              # overlapping classes: the vote matters


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_wrong_variants_are_told_apart(golden, variant):
    if variant in ("tie_larger_index", "vote_larger_label"):
        # ties are certain only on integer-valued data; there the restatement itself is the record
        t, yt, q, _ = R.integer_case()
        changed = False
        for k in (5, 24):
            _, want = R.kneighbors(q, t, k)
            _, got = R.kneighbors(q, t, k, variant)
            changed |= not np.array_equal(want, got)
            changed |= not np.array_equal(R.predict(q, t, yt, k), R.predict(q, t, yt, k, variant))
        assert changed
        if variant == "vote_larger_label":                                       # and on the recorded votes of the two-class cases
            g = golden["e513x7_k8"]
            assert not np.array_equal(R.vote(g["train_labels"][g["idx"]], larger_label=True)[0], g["pred"])
        return
    differs = 0
    for tag, g in golden.items():
        k = int(g["k"])
        _, idx = R.kneighbors(g["query"], g["train"], k, variant)
        differs += (not np.array_equal(idx, g["idx"])) or (not np.array_equal(R.predict(g["query"], g["train"], g["train_labels"], k, variant), g["pred"]))
    # the self exclusion shows only where query i's own list holds train row i; the other two change every case
    assert differs >= 1 if variant == "self_exclusion" else differs == len(golden)


def test_sharpness_constant_and_cap(golden):
    worst = 0.0
    for tag, g in golden.items():
        err = R.stage1_error(g["query"], g["train"])
        blunt = int((~R.sharp(g["query"], g["train"], int(g["k"]))).sum())
        print(f"{tag}: fp32 stage-1 error 2^{math.log2(err):.2f} of the scale, non-sharp {blunt} of {len(g['query'])}")
        assert blunt <= R.CAP * len(g["query"]), tag
        worst = max(worst, err)
    assert 2.0 ** math.ceil(math.log2(8 * worst)) == R.TAU
    t, _, q, _ = R.integer_case()
    assert R.sharp(q[:4], t[:5], 5).all()                                        # n_train == k: every query is sharp
