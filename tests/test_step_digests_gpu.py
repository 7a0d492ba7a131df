"""GPU: the head step computes bit for bit what the builds recorded under tests/golden/ computed.

The yardstick is not the code under test: the tables (bf16_step_digests.json, f32_path_digests.json) were written by the
recorder (now scripts/make_step_digests.py) on a build of the commit named in their "recorded_from" and are compared for
equality, as strings, with the digests tests/_step_digests.py computes on the build under test -- SHA-256 of the raw bytes of
the head weight, exp_avg and exp_avg_sq after 3 AdamW steps, of the 3 scalar rows, and of the flat gradient of one grad_step.

step_tails (recorded from the parent of the change that re-ordered them): the tails of the bf16 step's forward and dW tiles --
everything after a tile's last MFMA: the softmax passes and the wave exchange, dZ^T scaling, staging and stores, the slab
epilogue, the publish.  The smallest shapes at which a tail can go wrong (bf16, d = 128 unless stated, |scale| = 100):

  both_halves_c1000        C = 1000, rows 64 + 64: both wave halves live, padded last class tile
  wave4_one_class_c513     C = 513, rows 33 + 1: wave 4 with a single live class, waves 5-7 dead; partial and one-row sample tiles
  upper_half_padding_c512  C = 512, rows 32 + 32: waves 4-7 all padding
  wave0_only_c100          C = 100, rows 32 + 32: only wave 0 live
  learnable_scale_d512     C = 1000, d = 512, rows 96 + 40, learnable scale: the sum of exp * raw, cfg2's K
  negative_scale           C = 1000, rows 64 + 64, scale -100: the sign fold
  grid3 / lazy             the first case on 3 workgroups / with every fourth workgroup leaving its home tiles to others: the
                           cold path runs the same bodies, and a forward tile taken inside a dW tile's wait returns into it
  launch_per_kernel        the first case through the stand-alone kernels, which share the bodies

fwd_prologue (recorded from the parent of the change that re-ordered it, on an MI355X in the same GPU session as the first run
of the change, 2026-10-21): the bf16 forward tile's prologue -- the row-id loads, the W ring prefetch, the X pieces of the first
K block and the take verdict in front of the first barrier.  The smallest shapes at which it can go wrong (bf16, scale 100):

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
  launch_per_kernel    k256 through the stand-alone kernels (UMLH_BF16_FUSE=0), which share the body

Every bf16 case runs with UMLH_MICRO=0: steps of at most four 16-row tiles (33 + 1, 32 + 32 rows) would otherwise run as the micro
step, which has none of these tiles.  Every row keeps its top logit clear of ties (the runner's filter), so the hit counts in
the scalar rows are unambiguous.

f32_step (recorded from the parent of the change that gave the kernels of csrc/umlh_kernels_f32.hip one copy of each shared
piece, after two runs of every child agreed): the fp32 (parity mode) step through HeadEngine.train_step / grad_step, on the
smallest shapes that reach every instantiation of its kernels; the projected head adds its projection weight to the digests.

  fwd_ce_f32<CTW, WC, MODE>   C = 20, 64, 100, 200, 513, 1000 are the six (CTW, WC) pairs (1,1) (1,2) (1,4) (1,8) (2,8) (4,8);
                              d = 40 is MODE 0 (guarded loads), d = 48 MODE 1 (K % 16 == 0, K % 32 != 0), d = 96 MODE 3 and,
                              under UMLH_F32_X3=0, MODE 2.  At C = 20 (256-row block, X block of 64 columns) d = 96 is two X
                              blocks, the second one short; C = 1000, d = 544 is two X blocks at 32 rows per block.
  dw_f32x3 / dw_f32           C = 1000, d = 544: M N = 544 000 >= 8 * 128 * 128
  gemm_f32<0,1,*>             the dW GEMM of every other case
  gemm_f32<0,0,*>, <1,1,*>    the projected head (d_img 72, d 96, C 100): gathered rows, dH^T = W^T dZ^T
  learnable scale, a step without text rows: one case each
Rows are ragged (33 + 1, 70 + 31): rows past the segment and a class tile that straddles C are both present.  The fp32 switches
are read once per process: each environment (the default, UMLH_F32_X3=0) is one fresh child that computes all 22 cases."""
import pytest

import _step_digests as D

pytestmark = pytest.mark.gpu

BF16_CASES = [pytest.param(suite, case, id=f"{suite}-{case.name}")
              for suite in ("step_tails", "fwd_prologue") for case in D.SUITES[suite]]


@pytest.mark.parametrize("suite,case", BF16_CASES)
def test_bf16_step_bit_identical_to_recorded_build(suite, case, monkeypatch):
    want = D.load_table(suite)["default"][case.name]
    got = D.run_case(case, setenv=monkeypatch.setenv, delenv=lambda k: monkeypatch.delenv(k, raising=False))
    print(case.name, got)
    assert got == want, [k for k in got if got[k] != want[k]]


@pytest.mark.parametrize("env", list(D.PROCESS_ENVS["f32_step"]))
def test_f32_step_bit_identical_to_recorded_build(env):
    want = D.load_table("f32_step")[env]
    got = D.digests_in_child("f32_step", D.PROCESS_ENVS["f32_step"][env])
    for name in got:
        print(env, name, got[name])
    assert got == want, [(n, k) for n in want for k in want[n] if got.get(n, {}).get(k) != want[n][k]]
