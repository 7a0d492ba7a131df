"""No-GPU checks of ``multibench.data.LevelSequence``, the lazy sequence of loaders over noise levels that the affect families
(``robust_loaders``) and the MIMIC test sets (``multibench.mimic.get_dataloader``) share: length, indexing, and the cache that
keeps only the latest level and lets go of it before the next one is built.  Driven by a fake builder that records its calls."""
import gc
import weakref

import pytest


class _Table:
    def __init__(self, level):
        self.level = level


class _Builder:
    """``build`` of a sequence: records the levels it is asked for and, when it runs, whether the table it made before is
    still alive."""

    def __init__(self):
        self.calls, self.previous, self.previous_alive = [], None, []

    def __call__(self, level):
        if self.previous is not None:
            gc.collect()
            self.previous_alive.append(self.previous() is not None)
        table = _Table(level)
        self.calls.append(level)
        self.previous = weakref.ref(table)
        return table


def _sequence(n=5):
    from multibench.data import LevelSequence
    build = _Builder()
    return LevelSequence(n, build, lambda table: ("loader", table.level), base="clean"), build


def test_len_and_indexing():
    seq, build = _sequence()
    assert len(seq) == 5 and seq.base == "clean"
    assert seq[0] == ("loader", 0) and seq[-1] == seq[len(seq) - 1] == ("loader", 4) and seq[-5] == ("loader", 0)
    assert seq[1:4] == [("loader", 1), ("loader", 2), ("loader", 3)]           # a slice: the loaders in level order
    assert seq[::-2] == [("loader", 4), ("loader", 2), ("loader", 0)] and seq[5:] == []
    for bad in (5, -6, 100):
        with pytest.raises(IndexError):
            seq[bad]
    assert 5 not in build.calls and -6 not in build.calls                       # a refused index builds nothing
    assert [loader for loader in seq] == [("loader", k) for k in range(5)]      # the sequence protocol ends at IndexError


def test_only_the_latest_level_is_cached():
    seq, build = _sequence()
    first = seq.table(2)
    assert seq[2] == ("loader", 2) and seq.table(2) is first and seq.tables(2) is first and build.calls == [2]
    assert seq._last[0] == 2
    seq[3]
    assert build.calls == [2, 3] and seq._last[0] == 3
    seq[2]                                                                      # coming back builds again
    assert build.calls == [2, 3, 2] and seq.table(2) is not first
    seq[-3]                                                                     # the same level under its negative index
    assert build.calls == [2, 3, 2]


def test_the_previous_level_is_released_before_the_next_is_built():
    seq, build = _sequence()
    for k in (0, 1, 4, 1):
        seq[k]                                                                  # the loader is dropped at once: only the cache could hold the table
    assert build.calls == [0, 1, 4, 1] and build.previous_alive == [False, False, False]
    held = seq.table(1)                                                         # a caller's own reference does keep a table alive
    seq[2]
    assert build.previous_alive[-1] is True and held.level == 1
    assert build.previous() is seq._last[1]                                     # and the sequence holds the latest one
