"""The scratch sizes of the metric entry points, value for value: tests/golden/scratch_bytes.json holds what the fourteen public
*_scratch_bytes queries of include/umlh.h answered for a grid of shapes (smallest and largest legal, both sides of every threshold
of the plan code, a few illegal tuples that answer 0).  Each launcher forms its pointers from the plan its query returns the total
of, so the file lets a layout be restated and checked against what callers have allocated so far.
(scripts/make_golden_scratch_bytes.py records the file.)  Host arithmetic only: no GPU is touched."""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scratch_bytes.json")
QUERIES = ["umlh_align_scratch_bytes", "umlh_align_ext_scratch_bytes", "umlh_probe_scratch_bytes", "umlh_softmax_probe_scratch_bytes",
           "umlh_knn_scratch_bytes", "umlh_spectral_scratch_bytes", "umlh_subspace_scratch_bytes", "umlh_paired_cosine_scratch_bytes",
           "umlh_seq_step_stats_scratch_bytes", "umlh_seq_spectrum_scratch_bytes", "umlh_class_index_scratch_bytes",
           "umlh_class_stats_scratch_bytes", "umlh_eval_topk_scratch_bytes", "umlh_outlier_scratch_bytes"]


@pytest.fixture(scope="module")
def rows():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_the_file_covers_every_public_size_query(rows):
    from umlh import _lib
    assert QUERIES == [n for n in _lib.PROTOTYPES if n.endswith("_scratch_bytes")]
    for name in QUERIES:
        mine = [r for r in rows if r[0] == name]
        assert len(mine) >= 40, name
        assert all(len(r[1]) == len(_lib.PROTOTYPES[name][1]) for r in mine), name
        assert any(r[2] == 0 for r in mine), (name, "no refused tuple")
        assert all(r[2] % 256 == 0 for r in mine), (name, "a size that is no multiple of 256")
        assert len({tuple(r[1]) for r in mine}) == len(mine), (name, "a tuple recorded twice")
    assert len(rows) == sum(1 for r in rows if r[0] in QUERIES)


def test_every_size_is_the_recorded_one(rows, lib):
    bad = []
    for name, args, want in rows:
        got = int(getattr(lib, name)(*args))
        if got != want:
            bad.append((name, args, got, want))
    print(f"{len(rows)} rows replayed, {len(bad)} differ")
    assert not bad, bad[:10]
