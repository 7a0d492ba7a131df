"""GPU: the tails of the bf16 step's forward and dW tiles (everything after a tile's last MFMA: the softmax passes and the
wave exchange, dZ^T scaling, staging and stores, the slab epilogue, the publish) compute bit for bit what the parent of the
change that re-ordered them computed.

The yardstick is not the code under test: DIGESTS below was printed by scripts/make_step_tail_digests.py on a build of the
parent commit (PARENT) and is compared for equality with the same script's digests of the build under test -- SHA-256 of the
raw bytes of the head weight, exp_avg and exp_avg_sq after 3 AdamW steps, of the 3 scalar rows, and of the flat gradient of
one grad_step.  The cases are the smallest shapes at which a tail can go wrong (bf16, d = 128 unless stated, |scale| = 100):

  both_halves_c1000        C = 1000, rows 64 + 64: both wave halves live, padded last class tile
  wave4_one_class_c513     C = 513, rows 33 + 1: wave 4 with a single live class, waves 5-7 dead; partial and one-row sample tiles
  upper_half_padding_c512  C = 512, rows 32 + 32: waves 4-7 all padding
  wave0_only_c100          C = 100, rows 32 + 32: only wave 0 live
  learnable_scale_d512     C = 1000, d = 512, rows 96 + 40, learnable scale: the sum of exp * raw, cfg2's K
  negative_scale           C = 1000, rows 64 + 64, scale -100: the sign fold
  grid3 / lazy             the first case on 3 workgroups / with every fourth workgroup leaving its home tiles to others: the
                           cold path runs the same bodies, and a forward tile taken inside a dW tile's wait returns into it
  launch_per_kernel        the first case through the stand-alone kernels, which share the bodies

Every case runs with UMLH_MICRO=0: steps of at most four 16-row tiles (33 + 1, 32 + 32 rows) would otherwise run as the micro
step, which has none of these tiles.  Every row keeps its top logit clear of ties (the script's filter), so the hit counts in
the scalar rows are unambiguous."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

PARENT = "b30a579"
_SCRIPT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "make_step_tail_digests.py")

DIGESTS = {
    "both_halves_c1000": {
        "w_head": "64ca460d1ea4c56612fe8c18efdcd8b57e51bfe18e63667346d6060bd90560bc",
        "exp_avg": "8611885ed899e6347a9eab03e24e70a2c730414dca9a14cea6c66dee23d222c5",
        "exp_avg_sq": "6ba787eebdc80d3c7e48f1bc61b8a1600284e3780ea5bf3cf65763d0e76aa711",
        "scalars": "8089792642cb3b20b5df3dcb3726a27a3a3aa6c52b61a6e53e1bf49d467c065b",
        "grad": "4d4a6ba34760d751efe47f244f6b2b6d6028eb3350afaf531bb14a64618d0d81",
    },
    "wave4_one_class_c513": {
        "w_head": "87f73b3d4118175069546e1a4d4d73f0d12fbf92317486704fe518b00b0545ca",
        "exp_avg": "24c5503df1198b4c46528fa1dbbb9d1047498caf833067eb6fdad218aafbc789",
        "exp_avg_sq": "7ff38362a16c7e4d1b7b87b7eaa2928367362e90201e53f42e8339e827536133",
        "scalars": "d27877963b1ecebfbde8c64bf1eb560768b55f2029d76d5b793534834552854c",
        "grad": "a4cecb0ae32d79e78487a9bef63164b2e3ad6648f917d62ae9e50640823be938",
    },
    "upper_half_padding_c512": {
        "w_head": "2c44616da58e23cd48506b0b2ea9bc230c155a6f9592290e621267a24c911da9",
        "exp_avg": "f8571613d03b3a20a7b04dd5106268c51355dbc20a70182ea411f8dbfef2bd0a",
        "exp_avg_sq": "775c0b9076d1caa460e9fea72d4acc45256a2325e95ae95afd145c4d27a0aa0a",
        "scalars": "8c742008748857c126b5f2a3375b55f47db7af8500accdc41e2935cda3f9bb6a",
        "grad": "d03d6915ac2611843a8654211ad290fc50c45c9dcf97b89bfe887316220f4294",
    },
    "wave0_only_c100": {
        "w_head": "e4ef426ed9d04fb68a681d3837c44dda139d896c2e8a3718a8f46a906d464094",
        "exp_avg": "825c5331d4962393697f77fe11b5d69c682ba54d4975a586f0a051114f26f430",
        "exp_avg_sq": "547e9142a9c982bbfcda1512a59fedc6940577a55e67c85e403445d522b7f134",
        "scalars": "7706273648bbb0494ca8325a53423ca8906f95bce12726a8c3b9750c072f6374",
        "grad": "17a9c62e9ec341fffcfc17dfb65de6ff6625512f1d8ae5684dc758a805239b8a",
    },
    "learnable_scale_d512": {
        "w_head": "8914b7d3b148145a03a2680959b377a64091028a5ce7492407993f6f0f825a3b",
        "exp_avg": "4a88ece592aa249f39e149e63fde0dde01e60407d6ae580882603f26b3a2745c",
        "exp_avg_sq": "2fbf5e458912be8e27905878c301c683ec0bc69eb5a01da4efaf20e3aeae1903",
        "scalars": "ee42c68a627a12c51089de3573f31e40a3c130b0662b2967b383ce9fcf9eb374",
        "grad": "0efd5db04756c7756159e00f5b7bd474d5d6a418465ab58dcc2d3c126ba35d4b",
    },
    "negative_scale": {
        "w_head": "235753a7cee10888774a8552015c8c58dcf9bfbd9e22c6284b548df5b2406cb6",
        "exp_avg": "001fe9873dca6cbd849effcd6643a8f1fe1f8d69e68c782f57c22eeb5a9eca5f",
        "exp_avg_sq": "4f7eddd4ad44883bb1977852c99b3509996d0491b1516984b8b6e748e06ccc6c",
        "scalars": "62c41361f69b1d45d4016d22a3be33d96be71a579ef7dc14c1ed1287ea154b42",
        "grad": "fd2dcf3a857ffdbe44e9c0730fae6407588f0d5df3951fb277a371238dc4e5f2",
    },
    "grid3": {
        "w_head": "64ca460d1ea4c56612fe8c18efdcd8b57e51bfe18e63667346d6060bd90560bc",
        "exp_avg": "8611885ed899e6347a9eab03e24e70a2c730414dca9a14cea6c66dee23d222c5",
        "exp_avg_sq": "6ba787eebdc80d3c7e48f1bc61b8a1600284e3780ea5bf3cf65763d0e76aa711",
        "scalars": "8089792642cb3b20b5df3dcb3726a27a3a3aa6c52b61a6e53e1bf49d467c065b",
        "grad": "4d4a6ba34760d751efe47f244f6b2b6d6028eb3350afaf531bb14a64618d0d81",
    },
    "lazy": {
        "w_head": "64ca460d1ea4c56612fe8c18efdcd8b57e51bfe18e63667346d6060bd90560bc",
        "exp_avg": "8611885ed899e6347a9eab03e24e70a2c730414dca9a14cea6c66dee23d222c5",
        "exp_avg_sq": "6ba787eebdc80d3c7e48f1bc61b8a1600284e3780ea5bf3cf65763d0e76aa711",
        "scalars": "8089792642cb3b20b5df3dcb3726a27a3a3aa6c52b61a6e53e1bf49d467c065b",
        "grad": "4d4a6ba34760d751efe47f244f6b2b6d6028eb3350afaf531bb14a64618d0d81",
    },
    "launch_per_kernel": {
        "w_head": "64ca460d1ea4c56612fe8c18efdcd8b57e51bfe18e63667346d6060bd90560bc",
        "exp_avg": "8611885ed899e6347a9eab03e24e70a2c730414dca9a14cea6c66dee23d222c5",
        "exp_avg_sq": "6ba787eebdc80d3c7e48f1bc61b8a1600284e3780ea5bf3cf65763d0e76aa711",
        "scalars": "8089792642cb3b20b5df3dcb3726a27a3a3aa6c52b61a6e53e1bf49d467c065b",
        "grad": "4d4a6ba34760d751efe47f244f6b2b6d6028eb3350afaf531bb14a64618d0d81",
    },
}


def _script():
    spec = importlib.util.spec_from_file_location("make_step_tail_digests", _SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_table_covers_the_script_cases():
    mod = _script()
    assert list(DIGESTS) == list(mod.CASES)
    assert all(tuple(v) == mod.FIELDS for v in DIGESTS.values())


@pytest.mark.parametrize("name", list(DIGESTS))
def test_step_tails_bit_identical_to_parent(name, monkeypatch):
    got = _script().run_case(name, setenv=monkeypatch.setenv, delenv=lambda k: monkeypatch.delenv(k, raising=False))
    print(name, got)
    assert got == DIGESTS[name], [k for k in got if got[k] != DIGESTS[name][k]]
