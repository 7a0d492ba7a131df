"""CPU-side checks of the C-ABI shared library: it builds for gfx950, loads, and
exports every symbol include/umlh.h declares (no compute without a GPU); the ctypes
prototype table of umlh/_lib.py agrees with the header, declaration by declaration."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import umlh
    umlh.build_library()
    return umlh.load_library()


def test_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(ROOT, "include", "umlh.h")).read()
    declared = set(re.findall(r"\b(umlh_[a-z_]+)\s*\(", hdr))
    assert len(declared) >= 13
    for name in declared:
        assert hasattr(lib, name), name


def test_version_and_workspace_query(lib):
    from umlh._lib import Config
    assert lib.umlh_version() >= 1
    ok = Config(512, 512, 1000, 0, 0, 2, 0, 4096, 4096, 0.9, 0.999, 1e-8, 0.9, 0.01)
    assert lib.umlh_workspace_bytes(C.byref(ok)) > 1000 * 8192 * 4
    bad = Config(512, 256, 1000, 0, 0, 2, 0, 4096, 4096, 0.9, 0.999, 1e-8, 0.9, 0.01)   # dims differ w/o proj
    assert lib.umlh_workspace_bytes(C.byref(bad)) == 0
    too_many = Config(64, 64, 2000, 0, 0, 2, 0, 32, 32, 0.9, 0.999, 1e-8, 0.9, 0.0)
    assert lib.umlh_workspace_bytes(C.byref(too_many)) == 0


# umlh_workspace_bytes as the build before the region descriptions of csrc/umlh_api.cpp returned it (the partition must not
# move when a region's size is restated): (d_img, d_shared, C, has_proj, learnable_temp, optimizer, precision, rows img, rows txt).
# Together the configurations reach every optional region: both precisions, img_proj, the fp32 fragment-major shadow (d % 32 == 0)
# and its absence, the one-launch control words, the micro-step regions, the 2-D forward's exchange region.
WORKSPACE_BYTES = [
    ("fp32_lin_d512_c1000", (512, 512, 1000, 0, 0, 2, 0, 4096, 4096), {}, 56907776),
    ("bf16_lin_d512_c1000", (512, 512, 1000, 0, 0, 2, 1, 4096, 4096), {}, 38908160),
    ("bf16_mlp_1024_3200_c1000", (1024, 3200, 1000, 1, 0, 2, 1, 4096, 4096), {}, 244837376),
    ("fp32_mlp_40_56_c12", (40, 56, 12, 1, 1, 2, 0, 512, 128), {}, 1040896),
    ("fp32_lin_d30_c101", (30, 30, 101, 0, 1, 2, 0, 512, 128), {}, 1124864),
    ("bf16_lin_d512_c1000_fwd2d", (512, 512, 1000, 0, 0, 2, 1, 4096, 4096), {"UMLH_BF16_FWD2D": "1"}, 39989504),
    ("fp32_lin_d512_c1024", (512, 512, 1024, 0, 0, 2, 0, 4096, 4096), {}, 58191104),
    ("bf16_lin_d512_c1024", (512, 512, 1024, 0, 0, 2, 1, 4096, 4096), {}, 39405056),
    ("fp32_lin_d512_c1000_rows_1_0", (512, 512, 1000, 0, 0, 2, 0, 1, 0), {}, 25032704),
    ("bf16_lin_d512_c1000_rows_1_0", (512, 512, 1000, 0, 0, 2, 1, 1, 0), {}, 22496512),
]


@pytest.mark.parametrize("shape,env,expected", [c[1:] for c in WORKSPACE_BYTES], ids=[c[0] for c in WORKSPACE_BYTES])
def test_workspace_bytes_are_pinned(lib, monkeypatch, shape, env, expected):
    from umlh._lib import Config
    monkeypatch.delenv("UMLH_BF16_FWD2D", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = Config(*shape, 0.9, 0.999, 1e-8, 0.9, 0.01)
    assert lib.umlh_workspace_bytes(C.byref(cfg)) == expected


def test_null_and_unbound_calls_fail_with_message(lib):
    assert lib.umlh_create(None, None) < 0
    assert b"umlh_create" in lib.umlh_last_error()
    assert lib.umlh_train_step(None, None, None, None, None, None) < 0
    assert b"not bound" in lib.umlh_last_error()


def test_no_gpu_is_a_loud_error():
    import torch
    import umlh
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(umlh.UmlhError):
        umlh.HeadEngine(8, 8, 4, device="cpu")


def test_encoder_ops_validate_arguments_before_touching_the_gpu(lib):
    """The MultiBench encoder ops reject bad arguments with a message (no HIP call is made on these paths)."""
    fake = C.c_void_p(64)                                   # never dereferenced: the shape checks come first
    assert lib.umlh_gemm_f32(None, None, None, 4, 4, 4, 4, 4, 4, 0, 0, None, None, C.c_float(1.0), 1, None, None) != 0
    assert b"umlh_gemm_f32" in lib.umlh_last_error()
    assert lib.umlh_gemm_f32(fake, fake, fake, 4, 4, 4, 4, 4, 4, 0, 0, None, None, C.c_float(1.0), 3, None, None) != 0   # splits without slabs
    # (ta, tb) = (1, 0) has no kernel, and a stride shorter than the row it spans would read or write across rows: rejected up
    # front as UMLH_E_INVALID (not a HIP error from the launcher)
    E_INVALID = -1
    gemm = lambda M, N, K, lda, ldb, ldo, ta, tb: lib.umlh_gemm_f32(fake, fake, fake, M, N, K, lda, ldb, ldo, ta, tb, None, None,
                                                                     C.c_float(1.0), 1, None, None)
    for args, what in (((8, 6, 5, 8, 6, 6, 1, 0), b"(ta, tb) = (1, 0)"),
                       ((8, 6, 5, 5, 5, 5, 0, 0), b"ldo=5"),          # ldo < N
                       ((8, 6, 5, 4, 5, 6, 0, 0), b"lda=4"),          # ta = 0: lda < K
                       ((8, 6, 5, 7, 5, 6, 1, 1), b"lda=7"),          # ta = 1: lda < M
                       ((8, 6, 5, 5, 4, 6, 0, 0), b"ldb=4"),          # tb = 0: ldb < K
                       ((8, 6, 5, 5, 5, 6, 0, 1), b"ldb=5")):         # tb = 1: ldb < N
        assert gemm(*args) == E_INVALID, args
        msg = lib.umlh_last_error()
        assert b"umlh_gemm_f32" in msg and what in msg, (args, msg)
    rc = lib.umlh_attention_forward(fake, None, 200, 2, 20, 5, C.c_float(0.0), C.c_uint64(0), fake, fake, None)
    assert rc != 0 and b"envelope" in lib.umlh_last_error()
    rc = lib.umlh_attention_backward(fake, None, fake, fake, 16, 2, 330, 5, C.c_float(0.0), C.c_uint64(0), fake, None)   # head dim 66
    assert rc != 0 and b"envelope" in lib.umlh_last_error()
    assert lib.umlh_dropout(fake, 10, C.c_float(1.5), C.c_uint64(1), None) != 0
    assert lib.umlh_eval_rows(None, None, None, None) != 0


# ---- the ctypes prototype table against include/umlh.h (no GPU, no build) ----
_C_CLASSES = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint64_t": "u64", "float": "float", "double": "double",
              "void": "none", "umlh_handle_t": "pointer", "umlh_enc_plan_t": "pointer", "umlh_allreduce_fn": "pointer"}


def _c_class(ctype: str) -> str:
    if "*" in ctype or "[" in ctype:
        return "pointer"
    return _C_CLASSES[ctype.replace("const", "").strip()]


def _ctypes_class(t) -> str:
    if t is None:
        return "none"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C._CFuncPtr)):
        return "pointer"
    return {C.c_int32: "i32", C.c_int64: "i64", C.c_uint64: "u64", C.c_float: "float", C.c_double: "double"}[t]


def header_prototypes() -> dict:
    """name -> (return class, [argument classes]) of every umlh_* declaration of include/umlh.h."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umlh.h")).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^[ \t]*([A-Za-z_][\w \t]*?\**)[ \t]*\b(umlh_\w+)[ \t]*\(([^()]*)\)[ \t]*;", hdr, flags=re.M):
        args = [a.strip() for a in args.split(",")]
        if args == ["void"]:
            args = []
        # a parameter is `type name` or `type name[n]`: drop the name, keep what makes it a pointer
        out[name] = (_c_class(ret), [_c_class(re.sub(r"\b\w+[ \t]*(\[\w*\])?$", r"\1", a)) for a in args])
    return out


def prototype_mismatches(table: dict) -> list:
    """Every way ``table`` (name -> (restype, argtypes or None)) differs from the header, as sorted strings."""
    hdr, bad = header_prototypes(), []
    bad += [f"{n}: declared in umlh.h, missing from the table" for n in hdr.keys() - table.keys()]
    bad += [f"{n}: in the table, not declared in umlh.h" for n in table.keys() - hdr.keys()]
    for name in hdr.keys() & table.keys():
        restype, argtypes = table[name]
        if _ctypes_class(restype) != hdr[name][0]:
            bad.append(f"{name}: returns {hdr[name][0]}, restype {getattr(restype, '__name__', restype)}")
        if argtypes is None:
            bad.append(f"{name}: no argtypes")
        elif [_ctypes_class(t) for t in argtypes] != hdr[name][1]:
            bad.append(f"{name}: takes {hdr[name][1]}, argtypes {[_ctypes_class(t) for t in argtypes]}")
    return sorted(bad)


def test_header_parse_finds_every_declaration():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "umlh.h")).read(), flags=re.S)
    protos = header_prototypes()
    assert set(protos) == set(re.findall(r"\b(umlh_[a-z0-9_]+)\s*\(", hdr))     # every name that is followed by `(`
    assert protos["umlh_encoder_plan_offsets"] == ("i32", ["pointer", "pointer"])                      # uint64_t offsets[6]
    assert protos["umlh_last_error"] == ("pointer", []) and protos["umlh_encoder_plan_destroy"] == ("none", ["pointer"])
    assert protos["umlh_p2p_region_bytes"] == ("u64", ["i64", "i32"])
    assert protos["umlh_set_allreduce"] == ("i32", ["pointer", "pointer", "pointer", "i32"])


def test_prototype_table_matches_the_header():
    from umlh import _lib
    assert _lib.EXPORTS == list(_lib.PROTOTYPES)
    assert prototype_mismatches(_lib.PROTOTYPES) == []


def test_loaded_library_carries_the_table(lib):
    from umlh import _lib
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert lib.umlh_encoder_plan_destroy.restype is None
    assert lib.umlh_version.argtypes == []
    for name in ("umlh_p2p_region_bytes", "umlh_seq_mse_backward_scratch_floats", "umlh_encoder_plan_floats"):
        assert getattr(lib, name).restype is C.c_uint64, name


def test_size_queries_do_not_truncate_at_32_bits(lib):
    # a region for n floats cannot be smaller than n floats (csrc/umlh_p2p.hip: 2 * n_ranks slices of >= n / n_ranks floats)
    assert lib.umlh_p2p_region_bytes(1 << 31, 1) >= 4 * (1 << 31)
