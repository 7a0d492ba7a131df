"""No GPU: what the recorded bit checks of the head step stand on.  The committed tables cover exactly the cases and fields of
tests/_step_digests.py, the host inputs of every case are the ones the tables were recorded with, engine_env / child_env clear
what they say they clear, and the switch registry of tests/_switches.py is the set of switches the source reads and include/umlh.h
lists."""
import json
import os
import re

import pytest

import _step_digests as D
import _switches as S

CSRC = os.path.join(D.PKG, "csrc")


@pytest.mark.parametrize("suite", list(D.SUITES))
def test_table_covers_the_suite_cases(suite):
    table = D.load_table(suite)
    assert sorted(table) == sorted(D.PROCESS_ENVS[suite])
    for cases in table.values():
        assert sorted(cases) == sorted(c.name for c in D.SUITES[suite])
        assert all(sorted(cases[c.name]) == sorted(D.fields(c)) for c in D.SUITES[suite])


def test_suites_keep_their_sizes():
    assert {s: len(c) for s, c in D.SUITES.items()} == {"step_tails": 9, "fwd_prologue": 16, "f32_step": 22}


def test_f32_streamed_cases_differ_between_the_two_environments():
    table = D.load_table("f32_step")
    # MODE 3 and MODE 2 round differently: the streamed cases must not be the same bits under the two environments
    assert table["default"]["c1000_d96"] != table["x3_off"]["c1000_d96"]
    assert table["default"]["c100_d40"] == table["x3_off"]["c100_d40"]


@pytest.mark.parametrize("suite", list(D.SUITES))
def test_host_inputs_are_the_recorded_ones(suite):
    """tests/golden/step_digest_inputs.json was written from the inputs() of the three recorders this module replaced, on their
    last commit: a case named here has other inputs than the ones its digests were recorded with."""
    with open(os.path.join(D.TESTS, "golden", "step_digest_inputs.json")) as f:
        want = json.load(f)[suite]
    got = {c.name: D.inputs_digest(c) for c in D.SUITES[suite]}
    assert got == want, [n for n in want if got.get(n) != want[n]]


def test_engine_env_leaves_only_the_overrides(monkeypatch):
    for k in S.ENGINE_SWITCHES:
        monkeypatch.setenv(k, "5")
    monkeypatch.setenv("UMLH_F32_X3", "0")
    over = {"UMLH_BF16_FUSE": "0", "UMLH_STEP_GRID": "3"}
    S.engine_env(monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False), over)
    assert {k: os.environ[k] for k in S.ENGINE_SWITCHES if k in os.environ} == over
    assert os.environ["UMLH_F32_X3"] == "0"                      # (not an engine's to clear)
    restore = S.engine_env(over={"UMLH_MICRO": "0"})             # on os.environ itself, and back
    assert {k: os.environ[k] for k in S.ENGINE_SWITCHES if k in os.environ} == {"UMLH_MICRO": "0"}
    restore()
    assert {k: os.environ[k] for k in S.ENGINE_SWITCHES if k in os.environ} == over


@pytest.mark.parametrize("name", ["UMLH_F32_X3", "UMLH_WT", "UMLH_NO_SUCH_SWITCH"])
def test_engine_env_refuses_what_no_engine_reads(name):
    before = dict(os.environ)
    with pytest.raises(ValueError):
        S.engine_env(over={name: "0"})
    assert dict(os.environ) == before


def test_child_env_drops_every_registered_switch(monkeypatch):
    for k in S.SCOPE:
        monkeypatch.setenv(k, "5")
    env = S.child_env({"UMLH_F32_X3": "0"})
    assert {k: v for k, v in env.items() if k.startswith("UMLH_")} == {"UMLH_F32_X3": "0"}
    assert {k: v for k, v in env.items() if k not in S.SCOPE} == {k: v for k, v in os.environ.items() if k not in S.SCOPE}


def test_registry_is_the_set_of_switches_the_source_reads():
    reads = {}                                                   # name -> [(file, line text)]
    for fn in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, fn), errors="replace") as f:
            for line in f:
                for name in re.findall(r'(?:env_int|getenv)\("(UMLH_\w+)', line):
                    reads.setdefault(name, []).append(("csrc/" + fn, line))
    assert sorted(reads) == sorted(S.SCOPE)
    assert len(S.SWITCHES) == len(S.SCOPE)
    for name, scope, where in S.SWITCHES:
        assert where.rsplit(":", 1)[0] in [fn for fn, _ in reads[name]], (name, where)
        if any("static const" in line for _, line in reads[name]):
            assert scope == S.PROCESS, name                     # a function-local static is read once


def test_header_lists_every_switch_under_its_scope():
    with open(os.path.join(D.ROOT, "include", "umlh.h")) as f:
        comment = f.read().split("Environment switches read by the library", 1)[1].split("*/", 1)[0]
    engine, process = comment.split("read once per process", 1)
    listed = {S.ENGINE: set(re.findall(r"UMLH_\w+", engine)), S.PROCESS: set(re.findall(r"UMLH_\w+", process))}
    for name, scope, _ in S.SWITCHES:
        assert name in listed[scope], (name, scope)
    assert listed[S.ENGINE] | listed[S.PROCESS] == set(S.SCOPE)     # and nothing that no code reads
