"""The refusals of the stateless entry points (csrc/umlh_ops.cpp), byte for byte: tests/golden/host_errors.json holds, for a legal
base call of each entry point, what the library answers when one argument or two are bad -- the return code and the whole
message.  A two-fault row records which check comes first.  The per-feature CPU tests pin fragments of these messages; this one
pins the text and the order, so the host layer can be moved or restated and checked against it.
(scripts/make_golden_host_errors.py records the file.)

Every pointer of a row is a fake address, which is safe only because each row is refused before the first HIP call.  A check
that regressed would turn a row into a kernel launch on that address, so the module does not run where a GPU is visible: the
property is the same on every machine."""
import pytest
import torch

import _host_errors as H

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: replayed only where no GPU is visible")


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_the_file_holds_refusals_of_every_entry_point():
    from umlh import _lib
    entries = H.golden()["entries"]
    names = [e["entry"] for e in entries]
    assert len(names) == len(set(names)) == 52
    assert names == [n for n in _lib.PROTOTYPES if n in set(names)]                 # the header's order
    for e in entries:
        argtypes = _lib.PROTOTYPES[e["entry"]][1]
        assert len(e["base"]) == len(argtypes), e["entry"]
        assert e["rows"] and all(r["rc"] == H.E_INVALID and r["msg"] for r in e["rows"]), e["entry"]
        assert any(len(r["set"]) == 1 and r["set"][0][1] is None for r in e["rows"]), (e["entry"], "no NULL row")
        assert any(len(r["set"]) > 1 for r in e["rows"]), (e["entry"], "no two-fault row")


def test_every_row_is_refused_with_the_recorded_code_and_message(lib):
    bad, rows = [], 0
    for e in H.golden()["entries"]:
        for r in e["rows"]:
            rows += 1
            got = H.call(lib, e["entry"], H.with_changes(e["base"], r["set"]))
            if got != (r["rc"], r["msg"]):
                bad.append((e["entry"], r["set"], got, (r["rc"], r["msg"])))
    print(f"{rows} rows replayed, {len(bad)} differ")
    assert not bad, bad[:10]
