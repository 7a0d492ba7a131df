"""Calls of the stateless entry points of libumlh.so from JSON-able argument lists, shared by
scripts/make_golden_host_errors.py (which records the refusals) and tests/test_host_errors_cpu.py (which replays them).

An argument is an int, a float ("nan" for NaN), None (NULL), or one of
    {"ptrs": [...]}   a host array of pointers        (umlh_rollout's P, the tensor lists of umlh_optimizer_step_multi)
    {"i64s": [...]}   a host array of int64           (the element counts of umlh_optimizer_step_multi)
    {"cfg": [...]}    a host umlh_rollout_cfg_t, its fields in order
-- the three kinds of argument the checks themselves read on the host.  Every other pointer is a fake address such as 256: a
check that let one through would hand it to a kernel, which is why neither file runs where a GPU is visible."""
import ctypes as C
import json
import os

from umlh import _lib

E_INVALID = -1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_errors.json")


def load(path=None):
    """The library at `path` (default: the in-tree build) with every prototype of include/umlh.h declared."""
    if path is None:
        return _lib.load_library()
    lib = C.CDLL(path)
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    return lib


def _num(v):
    return float("nan") if v == "nan" else v


def _arg(v, ctype):
    if isinstance(v, dict):
        (kind, xs), = v.items()
        if kind == "ptrs":
            return (C.c_void_p * len(xs))(*xs)
        if kind == "i64s":
            return (C.c_int64 * len(xs))(*xs)
        assert kind == "cfg", kind
        return C.byref(_lib.RolloutCfg(*[_num(x) for x in xs]))
    if v is not None and ctype in (C.c_float, C.c_double):
        return float(_num(v))
    return v


def call(lib, entry, args):
    """(return code, message of umlh_last_error) of one call."""
    argtypes = _lib.PROTOTYPES[entry][1]
    assert len(args) == len(argtypes), (entry, len(args), len(argtypes))
    rc = getattr(lib, entry)(*[_arg(v, t) for v, t in zip(args, argtypes)])
    return rc, lib.umlh_last_error().decode()


def with_changes(base, changes):
    args = list(base)
    for i, v in changes:
        args[i] = v
    return args


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
