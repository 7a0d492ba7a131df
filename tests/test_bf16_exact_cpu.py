"""CPU: the exactly representable operands of tests/_bf16_exact_ref.py.  (a) The construction holds, with every assertion of the
reference firing, at every shape the GPU file runs; (b) C' = 512 is rejected, and why; (c) the criterion the GPU file applies
-- bit equality of every element with the float64 result -- notices each one-row defect the looser bf16 tests let through:
every mutation below changes the reference's own inputs the way a kernel with that bug would and must be detected."""
import numpy as np
import pytest

import _bf16_exact_ref as R


@pytest.mark.parametrize("shape", R.ALL_SHAPES, ids=lambda s: s.id)
def test_construction_is_exact_at_every_gpu_shape(shape):
    case, ref = R.case_and_reference(shape)
    s = shape
    assert len(case.live) == s.live and case.live.min() >= s.live_from
    if s.C > 256:
        assert all(np.any((case.live >= lo) & (case.live < lo + 32)) for lo in range(0, s.C, 32))
    if not s.dense and s.ri >= 255:
        assert len(np.unique(case.ii)) < s.ri                                  # gathered with duplicates
    assert ref.g_head.dtype == np.float32 and ref.g_head.shape == (s.C, s.d) and np.abs(ref.g_head).max() > 0
    assert (ref.g_proj is not None) == s.two_layer
    if s.two_layer and s.ri:
        assert np.abs(ref.g_proj[s.d // 2:]).max() > 0
    live_labels = np.isin(case.yi, case.live).all() and np.isin(case.yt, case.live).all()
    assert live_labels == (s.live == s.C)                                      # dead labels wherever there are dead classes
    for rows, loss, acc in ((s.ri, ref.loss_img, ref.acc_img), (s.rt, ref.loss_txt, ref.acc_txt)):
        assert 0.0 <= float(acc) * R.G <= rows and float(acc) * R.G == round(float(acc) * R.G)
        assert (loss > 0) == (rows > 0)
    if min(s.ri, s.rt) >= 33:
        assert 0 < float(ref.acc_img) * R.G < s.ri                             # the tie rule decides rows both ways


def test_512_live_classes_are_rejected():
    with pytest.raises(ValueError):
        R.make_case(R.single(1024, 1000, 512, 64, 64))
    coef = R.ALPHA * 64.0 / R.G
    with pytest.raises(AssertionError):                                        # 511/512: nine significant bits, a rounding tie
        R.assert_bf16_exact("dZ", np.array([coef * (1.0 / 512 - 1.0)]))
    R.assert_bf16_exact("dZ", np.array([coef * (1.0 / 256 - 1.0), coef / 256, -coef, 0.0]))


def _detected(ref, mut):
    n_h, first = R.mismatches(mut.g_head, ref.g_head)
    n_p = R.mismatches(mut.g_proj, ref.g_proj)[0] if ref.g_proj is not None else 0
    return n_h + n_p, first


@pytest.mark.parametrize("mutation,shape", [
    ("drop_last_row", R.SINGLE_SHAPES[0]), ("drop_last_row", R.SINGLE_SHAPES[4]), ("drop_last_row", R.DOUBLE_SHAPES[2]),
    ("padded_row_dz", R.SINGLE_SHAPES[0]), ("padded_row_dz", R.SINGLE_SHAPES[6]), ("padded_row_dz", R.DOUBLE_SHAPES[0]),
    ("swap_across_seam", R.SINGLE_SHAPES[0]), ("swap_across_seam", R.SINGLE_SHAPES[5]),
    ("shift_k_chunk", R.SINGLE_SHAPES[0]), ("shift_k_chunk", R.SINGLE_SHAPES[6]), ("shift_k_chunk", R.DOUBLE_SHAPES[1]),
    ("dh_rounded_twice", R.DOUBLE_SHAPES[0]), ("dh_rounded_twice", R.DOUBLE_SHAPES[2]),
], ids=lambda v: v if isinstance(v, str) else v.id)
def test_gradient_defects_fail_bit_equality(mutation, shape):
    """One row's share of a gradient element is of the size of the older tests' tolerance (8e-3 of the largest element); under
    bit equality every such defect shows.  Printed: how many elements differ, the first of them, the largest deviation."""
    case, ref = R.case_and_reference(shape)
    mut = R.reference(case, mutation)
    n, first = _detected(ref, mut)
    # (for scale: the largest deviation in units of max|dW_head|, which the older tests bound by 8e-3 plus 2 % of the element)
    dev = np.abs(mut.g_head.astype(np.float64) - ref.g_head).max() / np.abs(ref.g_head).max()
    print(f"{mutation} at {shape.id}: {n} elements differ, first {first[:1]}, max deviation {dev:.2e} of max|dW_head|")
    assert n > 0, "the mutation went unnoticed"


@pytest.mark.parametrize("shape", [R.SINGLE_SHAPES[0], R.SINGLE_SHAPES[3], R.DOUBLE_SHAPES[2]], ids=lambda s: s.id)
def test_argmax_on_the_second_live_class_fails_accuracy_equality(shape):
    case, ref = R.case_and_reference(shape)
    mut = R.reference(case, "argmax_second_live")
    print(f"argmax_second_live at {shape.id}: acc_img {float(ref.acc_img) * R.G:.0f} -> {float(mut.acc_img) * R.G:.0f} hits")
    assert mut.acc_img != ref.acc_img and (shape.rt < 33 or mut.acc_txt != ref.acc_txt)
    assert R.mismatches(mut.g_head, ref.g_head)[0] == 0                        # only the accuracies can tell


def test_sgd_step_of_the_reference_is_the_optimizer_recurrence_in_fp32():
    """W - lr g of the reference equals the device's own recurrence (m = 0 * 0 + g, w = w - lr * m) evaluated in fp32."""
    case, ref = R.case_and_reference(R.SINGLE_SHAPES[0])
    m = np.float32(0.0) * np.float32(0.0) + ref.g_head
    w = case.w_head - np.float32(R.LR) * m
    assert w.dtype == np.float32 and R.mismatches(w, ref.w_head_new)[0] == 0
    assert R.mismatches(ref.w_head_new, case.w_head)[0] > 0
