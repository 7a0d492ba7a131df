"""No GPU: the grouped alignment entry points (umlh_align_pairs and its size query): their place in the ABI, the size query against
the single-call sizes, every refusal with pointers that are never dereferenced, and the refusals of umlh.align.measure_pairs."""
import ctypes as C

import pytest
import torch

E_INVALID = -1
NEW = ("umlh_align_pairs_scratch", "umlh_align_pairs")
WHO = "umlh_align_pairs"
FAKE = 4096          # never dereferenced: every check comes before the first HIP call
_KEEP = []


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def _pair(i=0, n=100, d_a=8, d_b=12, topk=10, cka=1, lists=False, **over):
    """Member i with distinct fake output pointers (inputs are shared: every member names the same fake table)."""
    from umlh._lib import AlignPair
    base = (1 << 24) * (i + 1)
    it = AlignPair(a=FAKE, lda=d_a, d_a=d_a, b=FAKE, ldb=d_b, d_b=d_b, n=n, cka=cka, topk=topk, out5=base,
                   knn_a=base + (1 << 20) if lists else None, knn_b=base + (2 << 20) if lists else None,
                   scores_a=base + (3 << 20) if lists else None, scores_b=base + (4 << 20) if lists else None)
    for k, v in over.items():
        setattr(it, k, v)
    return it


def _array(items):
    arr = (type(items[0]) * len(items))(*items)
    _KEEP.append(arr)
    return arr


def _call(lib, items, splits=0, scratch=FAKE, nbytes=1 << 40, n=None):
    rc = lib.umlh_align_pairs(_array(items) if items else None, len(items) if n is None else n, splits, scratch, nbytes, None)
    return rc, lib.umlh_last_error().decode()


def _query(lib, items, splits=0):
    return lib.umlh_align_pairs_scratch(_array(items), len(items), splits)


# ---------------------------------------------------------------------------------------------------------------------------- #
# ABI
# ---------------------------------------------------------------------------------------------------------------------------- #
def test_abi_placement_and_prototypes(lib):
    from test_abi_cpu import prototype_mismatches
    from umlh import _lib
    assert prototype_mismatches(_lib.PROTOTYPES) == []
    assert lib.umlh_version() == 11
    names = list(_lib.PROTOTYPES)
    at = names.index("umlh_align_list_stats")
    assert tuple(names[at + 1:at + 3]) == NEW and names[at + 3] == "umlh_masked_mean"
    for n in NEW:
        fn = getattr(lib, n)
        assert fn.restype is _lib.PROTOTYPES[n][0] and list(fn.argtypes) == list(_lib.PROTOTYPES[n][1])
        assert not n.endswith("_scratch_bytes")
    assert lib.umlh_align_pairs_scratch.restype is C.c_uint64
    hdr = open(_lib._INCLUDE + "/umlh.h").read()
    pos = [hdr.index(w) for w in ("int  umlh_align_list_stats(", "#define UMLH_ALIGN_MAX_PAIRS 64", "} umlh_align_pair_t;",
                                  "uint64_t umlh_align_pairs_scratch(", "int  umlh_align_pairs(", "int  umlh_masked_mean(")]
    assert pos == sorted(pos)
    assert _lib.ALIGN_MAX_PAIRS == 64
    # the ctypes struct follows the header's field order and the C layout: 8-byte pointers and n, 4-byte ints, no padding holes
    assert [f[0] for f in _lib.AlignPair._fields_] == ["a", "lda", "d_a", "b", "ldb", "d_b", "n", "cka", "topk", "out5", "knn_a", "knn_b",
                                                        "scores_a", "scores_b"]
    assert C.sizeof(_lib.AlignPair) == 88 and _lib.AlignPair.out5.offset == 48
    import umlh
    assert callable(umlh.align.measure_pairs)


# ---------------------------------------------------------------------------------------------------------------------------- #
# the size query
# ---------------------------------------------------------------------------------------------------------------------------- #
SHAPES = [(6, 1, 1, 1, 1), (33, 5, 33, 10, 1), (255, 32, 32, 32, 1), (256, 33, 100, 10, 1), (257, 128, 128, 0, 1), (2000, 35, 300, 10, 1)]


def _single(lib, n, d_a, d_b, topk, splits):
    return lib.umlh_align_scratch_bytes(n, d_a, d_b, topk, splits)


def test_size_query_against_the_single_calls(lib):
    """With splits > 0 both forms use the chunk counts asked for, and the group's plan holds everything the single calls' scratch
    holds (they take the maximum of their stages, the group the sum) plus the descriptor tables.  With splits = 0 the group picks
    its k-NN chunk count from the strips of the whole group, which is smaller than a lone member's by design; for one member it
    is at least half the single call's for each of the two views, so the bound holds there as well."""
    items = [_pair(i, n, da, db, k, c) for i, (n, da, db, k, c) in enumerate(SHAPES)]
    for splits in (1, 2, 7):
        total = _query(lib, items, splits)
        assert total % 256 == 0
        assert total >= sum(_single(lib, n, da, db, k, splits) for n, da, db, k, c in SHAPES)
        # monotone: every prefix is smaller than the next one
        sizes = [_query(lib, items[:g], splits) for g in range(1, len(items) + 1)]
        assert all(s % 256 == 0 for s in sizes) and sizes == sorted(set(sizes)) and sizes[-1] == total
    for i, (n, da, db, k, c) in enumerate(SHAPES):                      # one member, automatic chunk counts
        alone = _query(lib, [items[i]], 0)
        assert alone % 256 == 0 and alone >= _single(lib, n, da, db, k, 0), (n, da, db, k)
    sizes = [_query(lib, items[:g], 0) for g in range(1, len(items) + 1)]
    assert all(s % 256 == 0 for s in sizes)
    # monotone with automatic chunk counts too when the added member is the same shape: the chunk count can only shrink, and
    # never below one chunk, which a group of 16 Gaussian-eval pairs has reached
    same = [_pair(i, 2000, 10, 10, 10, 1) for i in range(20)]
    s16, s17, s20 = (_query(lib, same[:g], 0) for g in (16, 17, 20))
    assert s16 < s17 < s20
    # lists the caller supplies are not carved from scratch
    assert _query(lib, [_pair(0, 2000, 10, 10, 10, 1, lists=True)], 1) == _query(lib, [_pair(0, 2000, 10, 10, 10, 1)], 1) - 2 * 80128


def test_size_query_is_zero_on_invalid_arguments(lib):
    ok = _array([_pair(0), _pair(1)])
    assert lib.umlh_align_pairs_scratch(ok, 2, 0) > 0
    for bad in ((None, 1, 0), (ok, 0, 0), (ok, -1, 0), (ok, 65, 0), (ok, 2, -1)):
        assert lib.umlh_align_pairs_scratch(*bad) == 0, bad
    for kw in (dict(d_a=0), dict(d_b=0), dict(lda=7), dict(ldb=11), dict(n=0), dict(n=(1 << 30) + 1), dict(topk=-1), dict(topk=33),
               dict(topk=100), dict(topk=0, cka=0)):
        assert _query(lib, [_pair(0), _pair(1, **kw)]) == 0, kw


# ---------------------------------------------------------------------------------------------------------------------------- #
# refusals, all before the first HIP call
# ---------------------------------------------------------------------------------------------------------------------------- #
needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: only where no call can reach a device")


@needs_no_gpu
def test_group_count_and_null_items(lib):
    rc, msg = _call(lib, [], n=1)
    assert rc == E_INVALID and WHO in msg and "items is NULL" in msg, msg
    for n in (0, -1, 65):
        rc, msg = _call(lib, [_pair(i) for i in range(2)], n=n)
        assert rc == E_INVALID and WHO in msg and "n_items" in msg, msg
    rc, msg = _call(lib, [_pair(0)], splits=-1)
    assert rc == E_INVALID and WHO in msg and "splits=-1" in msg, msg


BAD = [  # what is wrong with member 1, the words the message must carry
    (dict(a=None), "null pointer (a "), (dict(b=None), "null pointer (b "), (dict(out5=None), "null pointer (out5 "),
    (dict(lda=7), "lda=7"), (dict(ldb=11), "ldb=11"), (dict(d_a=0), "d_a=0"), (dict(d_b=-3), "d_b=-3"),
    (dict(topk=-1), "topk=-1"), (dict(topk=33), "topk=33"), (dict(topk=100), "topk=100"), (dict(n=10), "n=10"), (dict(n=0, topk=0), "n=0"),
    (dict(n=(1 << 30) + 1), "2^30"), (dict(topk=0, cka=0), "ask for nothing")]


@needs_no_gpu
@pytest.mark.parametrize("bad,word", BAD, ids=[w[1].strip(" (") + str(i) for i, w in enumerate(BAD)])
def test_a_member_outside_the_single_pair_envelope_is_named(lib, bad, word):
    rc, msg = _call(lib, [_pair(0), _pair(1, **bad), _pair(2)])
    assert rc == E_INVALID and WHO in msg and "member 1" in msg and word in msg, msg


@needs_no_gpu
def test_member_messages_are_the_single_calls(lib):
    """The shape and list checks are the code of umlh_align_cka / umlh_align_knn: the same sentence behind another prefix."""
    f, big = C.c_void_p(FAKE), 1 << 40
    rc = lib.umlh_align_cka(f, 7, 8, f, 12, 12, 100, 0, f, f, big, None)
    single = lib.umlh_last_error().decode()
    rc2, msg = _call(lib, [_pair(0, lda=7)])
    assert rc == rc2 == E_INVALID and single.split(": ", 1)[1] == msg.split("member 0: ", 1)[1]
    rc = lib.umlh_align_knn(f, 100, 8, 8, 100, 0, f, None, f, big, None)
    single = lib.umlh_last_error().decode()
    rc2, msg = _call(lib, [_pair(0, topk=100)])
    assert rc == rc2 == E_INVALID and single.split(": ", 1)[1] == msg.split("member 0: ", 1)[1]


@needs_no_gpu
def test_a_doubled_output_pointer_names_both_members(lib):
    a, b, c = _pair(0, lists=True), _pair(1, lists=True), _pair(2, lists=True)
    c.out5 = a.out5
    rc, msg = _call(lib, [a, b, c])
    assert rc == E_INVALID and WHO in msg and "member 2" in msg and "member 0" in msg and "out5" in msg, msg
    for mine, theirs in (("knn_a", "knn_b"), ("scores_b", "scores_a"), ("knn_b", "scores_b"), ("scores_a", "out5")):
        a, b = _pair(0, lists=True), _pair(1, lists=True)
        setattr(b, mine, getattr(a, theirs))
        rc, msg = _call(lib, [a, b])
        assert rc == E_INVALID and "member 1" in msg and "member 0" in msg and mine in msg and theirs in msg, msg
    a = _pair(0, lists=True)
    a.knn_b = a.knn_a                                            # twice within one member
    rc, msg = _call(lib, [a])
    assert rc == E_INVALID and "member 0" in msg and "knn_a" in msg and "knn_b" in msg, msg
    # inputs may be shared (every member above names the same fake table), and the list pointers of a member without lists
    # are not looked at: the call gets as far as the scratch check, the last one before the device
    a, b = _pair(0, lists=True), _pair(1, lists=True, topk=0)
    b.knn_a = a.knn_a
    rc, msg = _call(lib, [a, b], nbytes=8)
    assert rc == E_INVALID and "scratch of 8 bytes" in msg, msg


@needs_no_gpu
def test_scratch_checks(lib):
    items = [_pair(0), _pair(1, topk=0), _pair(2, cka=0)]
    need = _query(lib, items, 2)
    for kw in (dict(scratch=None), dict(nbytes=need - 1), dict(nbytes=0), dict(scratch=FAKE + 4)):
        rc, msg = _call(lib, items, splits=2, **kw)
        assert rc == E_INVALID and WHO in msg and "scratch" in msg, (kw, msg)


# ---------------------------------------------------------------------------------------------------------------------------- #
# umlh.align.measure_pairs
# ---------------------------------------------------------------------------------------------------------------------------- #
def test_measure_pairs_refusals():
    from umlh import align
    a, b = torch.zeros(20, 4), torch.zeros(20, 6)
    cases = [([], "no pairs"), ([(a,)], "member 0"), ([(a, b), (a, b, 3)], "member 1"), ([(a, b, {"k": 3})], "unknown options"),
             ([(a, b), (a, torch.zeros(19, 6))], "member 1"), ([(a, torch.zeros(20))], "member 0"), ([(a, "b")], "member 0"),
             ([(a, b, {"topk": 20})], "topk=20"), ([(a, b, {"topk": 33})], "topk=33"), ([(a, b, {"topk": -1})], "topk=-1"),
             ([(a, b), (a, b, {"topk": 0, "cka": False})], "ask for nothing")]
    for pairs, word in cases:
        with pytest.raises(ValueError, match=word):
            align.measure_pairs(pairs)
    with pytest.raises(ValueError, match="splits=-1"):
        align.measure_pairs([(a, b)], splits=-1)
    with pytest.raises(ValueError, match="ask for nothing"):
        align.measure_pairs([(a, b)], topk=0, cka=False)
    if not torch.cuda.is_available():                       # every argument error comes first; then: no CPU compute path
        with pytest.raises(RuntimeError, match="needs a GPU"):
            align.measure_pairs([(a, b)])
