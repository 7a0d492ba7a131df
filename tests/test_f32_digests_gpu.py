"""GPU: the fp32 (parity mode) step computes bit for bit what the build recorded in tests/golden/f32_path_digests.json computed.

The yardstick is not the code under test: the table was written by scripts/make_f32_digests.py on a build of the commit named in
its "recorded_from" (the parent of the change that gave the kernels of csrc/umlh_kernels_f32.hip one copy of each shared piece),
after two runs of every child agreed.  It is compared for equality, as strings, with the same script's digests of the build under
test: SHA-256 of the raw bytes of the head weight, exp_avg and exp_avg_sq after 3 AdamW steps of HeadEngine.train_step, of the 3
scalar rows, and of the flat gradient of one grad_step.  The cases (the script's docstring lists what each one reaches) cover the
six (CTW, WC) pairs of fwd_ce_f32 in each of its four modes, both dW tiles, gemm_f32 with and without gathered rows, a learnable
scale and a step without text rows, all on ragged row counts.

The switches are read once per process: each environment (the default, UMLH_F32_X3=0) is one fresh child."""
import importlib.util
import os

import pytest

_SCRIPT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "make_f32_digests.py")


def _script():
    spec = importlib.util.spec_from_file_location("make_f32_digests", _SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_table_covers_the_script_cases():
    mod = _script()
    table = mod.load_table()["step"]
    assert sorted(table) == sorted(mod.STEP_ENVS)
    for env in mod.STEP_ENVS:
        assert sorted(table[env]) == sorted(mod.STEP_CASES)
    # MODE 3 and MODE 2 round differently: the streamed cases must not be the same bits under the two environments
    assert table["default"]["c1000_d96"] != table["x3_off"]["c1000_d96"]
    assert table["default"]["c100_d40"] == table["x3_off"]["c100_d40"]


@pytest.mark.gpu
@pytest.mark.parametrize("env", ["default", "x3_off"])
def test_f32_step_bit_identical_to_recorded_build(env):
    mod = _script()
    want = mod.load_table()["step"][env]
    got = mod.step_digests(env)
    for name in got:
        print(env, name, got[name])
    assert got == want, [(n, k) for n in want for k in want[n] if got.get(n, {}).get(k) != want[n][k]]
