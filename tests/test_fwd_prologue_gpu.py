"""GPU: the bf16 forward tile's prologue -- the row-id loads, the W ring prefetch, the X pieces of the first K block and the
take verdict in front of the first barrier -- may be re-ordered, but the step computes bit for bit what the parent of the change
that re-ordered it computed.

The yardstick is not the code under test: DIGESTS below was printed by scripts/make_fwd_prologue_digests.py on a build of the
parent commit (PARENT) and is compared for equality with the same script's digests of the build under test -- SHA-256 of the
raw bytes of the head weight, exp_avg and exp_avg_sq after 3 AdamW steps, of the 3 scalar rows, and of the flat gradient of
one grad_step.  Session: the parent's table was generated on an MI355X in the same GPU session as the first run of the change
(2026-10-21; parent library built from a clean export of PARENT next to the tree under test, both scripts run back to back in
one job, 16 cases x 5 arrays equal).

The cases are the smallest shapes at which the prologue can go wrong (bf16, UMLH_MICRO=0, scale 100, every row's top logit
clear of ties -- the script's filter):

  k128                 C = 1000, d = 128, rows 64 + 64: nks = PD, the prologue ring is the whole stream, the slot clamp
                       min(d, nks-1) is live and the only k-group is the one without refills
  k256                 the same with d = 256: one refill group, then the last
  k512_index_edges     C = 1000, d = 512, rows 96 + 40; the index vectors hold repeated ids and the table's first and last row:
                       cfg2's K with one X block, the X address arithmetic
  k1024_two_blocks     C = 1000, d = 1024, rows 32 + 32: the second X block is staged with refills in flight
  partial_dead_waves   C = 513, d = 256, rows 33 + 1: rows clamped to the segment's last row, waves 5-7 not live (they prefetch
                       all the same and use nothing of it)
  identity_rows        k256 without index vectors (RowBatch.index = None): the row-id loads read a dummy word
  narrow_c32 .. c512   d = 256, rows 40 + 24: the instantiations (CTW, WC) = (1,1), (1,2), (1,4), (1,8), (2,8) -- several rows
                       per wave-load, XK = 128 / 256 / 512
  stw2_c512 / c1000    k256 with UMLH_BF16_STW=2 through the stand-alone kernels: instantiations (2,8,2) and (4,8,2)
  grid3 / lazy         k256 on 3 workgroups / with every fourth workgroup leaving its home tiles to others: the cold path, a
                       forward tile that returns at the take verdict with loads in flight, a forward tile taken inside a dW wait
  launch_per_kernel    k256 through the stand-alone kernels (UMLH_BF16_FUSE=0), which share the body"""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

PARENT = "ee6b7c6"
_SCRIPT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "make_fwd_prologue_digests.py")

DIGESTS = {
    "k128": {
        "w_head": "f9dfaf3fe9bb34738b48b92a465f0af5d08ef0d28a6cb72b3eed6cfd0a5d63ab",
        "exp_avg": "3eec9dbf144ed4c8f27028304079b35a1710f427be71a8feb1d0ed72438b703f",
        "exp_avg_sq": "fe09a991d2e628b821c06f872b53c0372ccda8a4c296b51ec38b8574e5278640",
        "scalars": "093d69ae26296068b0d8177ba086eacf6549a54333613ae06074361e7d5f443b",
        "grad": "7491e0753865708299493ec1994cf70b654b6cc55cacb6095835dd8abf7288c5",
    },
    "k256": {
        "w_head": "e55c8b98098b5f9640736b4ec9966c392167d20c25b937901b83e797b4eee12b",
        "exp_avg": "100dba6a36fe0678b98edf1c3d78f43bf0aa75f7f0591fa337452a35d59e40a6",
        "exp_avg_sq": "937e0e2b877a099b2ecd34d8d5edc2b8937b26674b1617141dbfe56d3efd91d6",
        "scalars": "1e2fb93a86e1427fa23ab0f0bbe63c23651b304d6b10a5cbe9ba87d01d90acdb",
        "grad": "cc638c4aa4bf89ece5e9cf224636e71f5fa5c036e43523032de5e7675bb58dbc",
    },
    "k512_index_edges": {
        "w_head": "a4c31ed40d079ea76cb9fcf9ce5656b328950825876977da498028d5037bf27c",
        "exp_avg": "c832abaae0e7dcb5600b9b34e4e54ed6ceee1873ac8fef5ae46e49a01835ec5d",
        "exp_avg_sq": "091d1806ea62701dbc95933be4df46ff13f2d39a1d9c151210749e6f6f8f5fdc",
        "scalars": "216609ad84ca59a496ef231553aef0e3c94c70bc184c7a72cdf5e7440f827819",
        "grad": "7d62dc1047dba39074eeebd2a1aa5bb32f4d917ad440867655a44212be50f9cf",
    },
    "k1024_two_blocks": {
        "w_head": "24adc0b86af58ffc9c322d9aa56f63c2f8453ddfc0f0ec6f3bc4b61ffb5d072d",
        "exp_avg": "8d4d94cc88dc3f36fa6fb9f72505dd4745d4e49ab8f470764a15c65193ad2ea1",
        "exp_avg_sq": "759cc48578f2c0173c2710577bb8bf654bc5dd67106e5fabe5a18bfd9cbbecf1",
        "scalars": "7b42a67cf04c8f28ac336a13967e588e2fad59d88963cb079d0f8de26050f04e",
        "grad": "b8cd4b43809d6d1c13f440f9156cb01623a7ccdde5ca143815396b34e9020e4f",
    },
    "partial_dead_waves": {
        "w_head": "7b3bd75d81420fc5f03729fb33c73577a6a28c26be98b4e06a7bfd2f714bcace",
        "exp_avg": "0121c65affea1e27a4ed051a1b60a34d0561aad7962195362d5e210ff1c39016",
        "exp_avg_sq": "c96cc092ca2dfb5b1100460679e9def37099561e44c00214f38ab5826f624c54",
        "scalars": "46625664de25a9a3aae71a3b705c1535c4034ee768de832ac52fd33b38cb8b2a",
        "grad": "fbf1b9b3fe1c5e92ed687189afb0497da7383c1699f9cd0b96a667af981fcead",
    },
    "identity_rows": {
        "w_head": "e55c8b98098b5f9640736b4ec9966c392167d20c25b937901b83e797b4eee12b",
        "exp_avg": "100dba6a36fe0678b98edf1c3d78f43bf0aa75f7f0591fa337452a35d59e40a6",
        "exp_avg_sq": "937e0e2b877a099b2ecd34d8d5edc2b8937b26674b1617141dbfe56d3efd91d6",
        "scalars": "1e2fb93a86e1427fa23ab0f0bbe63c23651b304d6b10a5cbe9ba87d01d90acdb",
        "grad": "cc638c4aa4bf89ece5e9cf224636e71f5fa5c036e43523032de5e7675bb58dbc",
    },
    "narrow_c32": {
        "w_head": "5b82f9fb99b69c1997f32739ac6c43a5dab89d7716cf322f4c25b05cca74f980",
        "exp_avg": "aab8a5f2ba23c3790827d7e356a98bb63e2d41bfacba628bbe1ab958fbf8491e",
        "exp_avg_sq": "a8c4bbb9e962fbb7bd0a7ab27a83a3fed509713d3e80a3c43c0325092eb6115f",
        "scalars": "dcc514c8bff5db01fadd99adcfefc52a1f4583bb237b08030cf6a8331fe4119c",
        "grad": "c7307ee5dd59853544d8334077006a00cd59d0ae6f29636cc5f6a2b436054260",
    },
    "narrow_c64": {
        "w_head": "1e744ee6c1827e9d1b834092e2bb70355dc393c57755ec8b6fecf0cc135c9d25",
        "exp_avg": "b926b6e7427315db5cf98cc9f578ec9b1196272ac9fc573c367e6fd6a5b3da33",
        "exp_avg_sq": "89093248e0ae3e7b0054d7e30adf5013c1c7a27b11d1d0f7f591a24914d50997",
        "scalars": "826d508dfeb02720ad9c445d8fcd7192efe9cc1a0fc14c1c76004a30819f890d",
        "grad": "e81664fdb0be6b0deb1bda18fad9e5ac1b0c0a66ea76481c26cc70ddcf7a3b5b",
    },
    "narrow_c128": {
        "w_head": "d433c504190d09672f35dd48bf6669e40371dbd65b1a33d1d5f2b267a6b916cf",
        "exp_avg": "6a554149d7dcbb7c3ca9900395df455132db69f40b742e9fef24305f1bfce9fb",
        "exp_avg_sq": "e96a4af25dd72d7328b35ec314c5c504ad256c5ec79f1ef5ec44e5440d4eaa07",
        "scalars": "f1d41810435b3c1859c18c2fa016b9e0ca4dfccc7b5ce48a14bd33b56e56c618",
        "grad": "383f2c837a818624da8542f9545f60ae9e3b87fde2482bdd4145764d56678056",
    },
    "narrow_c256": {
        "w_head": "0de81de1b49416a519470c1cbbb733aa5ccbc382657ee4cc5849ba3b9983e808",
        "exp_avg": "ad104118f77e7ff81e45990c8c1f7213f83291599137ee5159694ad0bf82e61b",
        "exp_avg_sq": "62a69d62eec83d1b7f72d0bfa42b62a6c934dd1788e60bcb99d7121af5338f63",
        "scalars": "070fb2e6b3d5818ec0755933f01615e0d2c77e31166bafbfabffba96d60d4d76",
        "grad": "3d0690a96b0f36657af54b2423b93dc84a3a8c7798c78a5cc142d6c57f312c59",
    },
    "narrow_c512": {
        "w_head": "c84f96a2e2ed928a1c795d88a9a012afb9e3cb04ca48d358abd94a757987a3f6",
        "exp_avg": "9bdc4df7d7561c3adbb9ac4d582499aea2339de0725270b39e11b9d6fd6320fa",
        "exp_avg_sq": "b44e98b725ff71657878bd8a8ffe1852e1e16df3d484a0561f334cc80286620b",
        "scalars": "90d8dfba31a5e593f1933e441d1f562cd51ae76d948e4b271859de022d0cad99",
        "grad": "0a8627e17f1193082df947b662b2c49039f1883613f94a9cb9b3c18c4580e5eb",
    },
    "stw2_c512": {
        "w_head": "9066e0e3bd20ab1009ed69cbbcd35885b8988a2cb56a4bbe954d470d8e485e89",
        "exp_avg": "8b9850a08d309abc644f43c338a91f450f992b32b3656b74e98d41b6c465edb8",
        "exp_avg_sq": "4a803588affa8f44db2abe2bc5d450606e98d09ae83681c987a3b3c4aec3618f",
        "scalars": "cef7368b4ad05c12bc70e2b5bc0bf92994ceb9e9d68a1fd8b2a268b25e35cf31",
        "grad": "09de4075ff898af95ab74200cb9177db94f72492e3247accee97fd96ade27bdd",
    },
    "stw2_c1000": {
        "w_head": "e73182ee32a1cb2999c632c07c4e51571ff9613c73e626b9e5d058ee5f6b2cac",
        "exp_avg": "ac8eb5f28c446cf455ed2edd9aae63f282b8427989e1ea39ebc07a3771fa98e6",
        "exp_avg_sq": "2d64cae7f36273f07fc42057eefe7fd087c2d4f35b0571ad65daf50b53037269",
        "scalars": "c9ad186279646396a8bc642ec67f37f11a9879b6dad942c02af55468398465ab",
        "grad": "2b68b8d9ce14a98c7396f8ae7a7f11fc637ddb3cfec22013d0b72ac9edad755e",
    },
    "grid3": {
        "w_head": "e55c8b98098b5f9640736b4ec9966c392167d20c25b937901b83e797b4eee12b",
        "exp_avg": "100dba6a36fe0678b98edf1c3d78f43bf0aa75f7f0591fa337452a35d59e40a6",
        "exp_avg_sq": "937e0e2b877a099b2ecd34d8d5edc2b8937b26674b1617141dbfe56d3efd91d6",
        "scalars": "1e2fb93a86e1427fa23ab0f0bbe63c23651b304d6b10a5cbe9ba87d01d90acdb",
        "grad": "cc638c4aa4bf89ece5e9cf224636e71f5fa5c036e43523032de5e7675bb58dbc",
    },
    "lazy": {
        "w_head": "e55c8b98098b5f9640736b4ec9966c392167d20c25b937901b83e797b4eee12b",
        "exp_avg": "100dba6a36fe0678b98edf1c3d78f43bf0aa75f7f0591fa337452a35d59e40a6",
        "exp_avg_sq": "937e0e2b877a099b2ecd34d8d5edc2b8937b26674b1617141dbfe56d3efd91d6",
        "scalars": "1e2fb93a86e1427fa23ab0f0bbe63c23651b304d6b10a5cbe9ba87d01d90acdb",
        "grad": "cc638c4aa4bf89ece5e9cf224636e71f5fa5c036e43523032de5e7675bb58dbc",
    },
    "launch_per_kernel": {
        "w_head": "e55c8b98098b5f9640736b4ec9966c392167d20c25b937901b83e797b4eee12b",
        "exp_avg": "100dba6a36fe0678b98edf1c3d78f43bf0aa75f7f0591fa337452a35d59e40a6",
        "exp_avg_sq": "937e0e2b877a099b2ecd34d8d5edc2b8937b26674b1617141dbfe56d3efd91d6",
        "scalars": "1e2fb93a86e1427fa23ab0f0bbe63c23651b304d6b10a5cbe9ba87d01d90acdb",
        "grad": "cc638c4aa4bf89ece5e9cf224636e71f5fa5c036e43523032de5e7675bb58dbc",
    },
}


def _script():
    spec = importlib.util.spec_from_file_location("make_fwd_prologue_digests", _SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_table_covers_the_script_cases():
    mod = _script()
    assert list(DIGESTS) == list(mod.CASES)
    assert all(tuple(v) == mod.FIELDS for v in DIGESTS.values())


@pytest.mark.parametrize("name", list(DIGESTS))
def test_fwd_prologue_bit_identical_to_parent(name, monkeypatch):
    got = _script().run_case(name, setenv=monkeypatch.setenv, delenv=lambda k: monkeypatch.delenv(k, raising=False))
    print(name, got)
    assert got == DIGESTS[name], [k for k in got if got[k] != DIGESTS[name][k]]
