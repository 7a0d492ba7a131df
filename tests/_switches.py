"""The environment switches the library reads (env_int / getenv in unpaired-multimodal-learning_amd/csrc), and the two ways a test
sets them.  tests/test_step_digests_cpu.py holds the table to the source and to the list in include/umlh.h.

  ENGINE   read when an engine is created (umlh_create, make_layout): set it in front of the engine, engine_env()
  PROCESS  read once per process (a function-local static): only a fresh child process sees another value, child_env().  The two
           GEMM stamp switches are read at every gemm_enc launch of an analysis build; they stand here so that no engine test
           sets them in its own process.

The third column is where the switch is read, as of the commit that last touched this table."""
import os

ENGINE, PROCESS = "engine", "process"

SWITCHES = (
    ("UMLH_BF16_FWD2D", ENGINE, "csrc/umlh_api.cpp:134"),
    ("UMLH_DBG_FWD", ENGINE, "csrc/umlh_api.cpp:280"),
    ("UMLH_DBG_DW", ENGINE, "csrc/umlh_api.cpp:281"),
    ("UMLH_BF16_STW", ENGINE, "csrc/umlh_api.cpp:285"),
    ("UMLH_DBG_STEP", ENGINE, "csrc/umlh_api.cpp:291"),
    ("UMLH_STEP_LAZY", ENGINE, "csrc/umlh_api.cpp:293"),
    ("UMLH_BF16_FUSE", ENGINE, "csrc/umlh_api.cpp:294"),
    ("UMLH_FORCE_DP", ENGINE, "csrc/umlh_api.cpp:304"),
    ("UMLH_MICRO", ENGINE, "csrc/umlh_api.cpp:306"),
    ("UMLH_STEP_GRID", ENGINE, "csrc/umlh_api.cpp:309"),
    ("UMLH_WT", PROCESS, "csrc/umlh_common.h:63"),
    ("UMLH_F32_X3", PROCESS, "csrc/umlh_common.h:75"),
    ("UMLH_ENC_SPLIT_WGS", PROCESS, "csrc/umlh_host.h:27"),
    ("UMLH_DBG_MICRO", PROCESS, "csrc/umlh_api.cpp:1111"),
    ("UMLH_ENC_GRAPH", PROCESS, "csrc/umlh_encoder.cpp:332"),
    ("UMLH_F32_FWD", PROCESS, "csrc/umlh_kernels_f32.hip:1719"),
    ("UMLH_F32_DW", PROCESS, "csrc/umlh_kernels_f32.hip:1726"),
    ("UMLH_F32_TM", PROCESS, "csrc/umlh_kernels_f32.hip:1751"),
    ("UMLH_DBG_GEMM_STAMPS", PROCESS, "csrc/umlh_kernels_f32.hip:1769"),
    ("UMLH_DBG_GEMM_CALL", PROCESS, "csrc/umlh_kernels_f32.hip:1772"),
)
SCOPE = {name: scope for name, scope, _ in SWITCHES}
ENGINE_SWITCHES = tuple(name for name, scope, _ in SWITCHES if scope == ENGINE)


def engine_env(setenv=None, delenv=None, over=()):
    """Delete every ENGINE switch, then set `over` ({name: value}); the next engine is created under exactly `over`.  In a test:
    setenv = monkeypatch.setenv, delenv = lambda k: monkeypatch.delenv(k, raising=False), and monkeypatch puts the environment
    back.  Without them os.environ is changed, and the function returned puts it back."""
    over = dict(over)
    wrong = [k for k in over if SCOPE.get(k) != ENGINE]
    if wrong:
        raise ValueError(f"{wrong}: not read at engine creation; a switch read once per process needs a child (child_env)")
    if (setenv is None) != (delenv is None):
        raise ValueError("setenv and delenv go together")
    saved = {k: os.environ.get(k) for k in ENGINE_SWITCHES} if setenv is None else {}
    setenv = setenv or os.environ.__setitem__
    delenv = delenv or (lambda k: os.environ.pop(k, None))
    for k in ENGINE_SWITCHES:
        delenv(k)
    for k, v in over.items():
        setenv(k, v)

    def restore():
        for k, v in saved.items():
            if v is None:
                delenv(k)
            else:
                setenv(k, v)
    return restore


def monkeypatch_engine_env(monkeypatch, over=()):
    """engine_env through a test's monkeypatch fixture: the next engine of the test is created under exactly `over`."""
    engine_env(monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False), over)


def child_env(over=()):
    """The environment of a child process: os.environ without any registered switch, plus `over`."""
    over = dict(over)
    wrong = [k for k in over if k not in SCOPE]
    if wrong:
        raise ValueError(f"{wrong}: not a switch the library reads")
    env = {k: v for k, v in os.environ.items() if k not in SCOPE}
    env.update(over)
    return env
