"""The inputs of test_gpu_roi_rpn_edges.py hold what they claim (CPU: the oracle alone, no library loaded).

Each case of _roi_rpn_cases.py exists for one branch of rpn_loss_grad_kernel, detection_targets_kernel or the RoIAlign kernels; the claims
that put it on that branch -- a positive in every 256-wide pass, an exact float32 tie, an odd N, a sample that is a pixel -- are
asserted here, so a re-seeded or edited case that has left its branch is red wherever the suite runs."""
import numpy as np
import pytest

import _roi_rpn_cases as K
from oracle import np_oracle as O

F32 = np.float32


# ---- RPN losses ------------------------------------------------------------------------------------------------------------------

def test_rpn_three_passes_has_positives_in_every_pass_and_differing_counts_per_image():
    c = K.rpn_three_passes()
    assert sum(K.RPN_SIZES) == 1023 and c.B == 3
    assert [int((c.match[b] != 0).sum()) for b in range(3)] == [230, 256, 114] and c.n_sel == 600
    pos = [int((c.match[b] == 1).sum()) for b in range(3)]
    assert len(set(pos)) == 3 and sum(pos) == c.n_pos <= K.RPN_TARGET_CAPACITY
    assert len(c.pass_positives()) == 3 and min(c.pass_positives()) >= 1              # a rank counted within the pass only is wrong in passes 2, 3
    for b in (0, 2):                                                                  # first and last anchor of the first and last image
        assert c.match[b, 0] != 0 and c.match[b, 1022] != 0
    assert c.match[0, 0] == 1 and c.match[2, 1022] == 1
    # the selection is dense_model._rpn_selection's: anchor order inside an image, images in order, index b * h * w * A + i
    assert c.lvl[0] == 0 and c.idx[0] == 0 and c.lvl[-1] == 4 and c.idx[-1] == 2 * K.RPN_SIZES[4] + 2
    for b, (lo, hi) in enumerate(((0, 230), (230, 486), (486, 600))):
        size = np.asarray(K.RPN_SIZES)[c.lvl[lo:hi]]
        assert np.all(c.idx[lo:hi] // size == b)
        flat = np.cumsum([0] + K.RPN_SIZES)[c.lvl[lo:hi]] + c.idx[lo:hi] % size
        assert np.all(np.diff(flat) > 0) and np.array_equal(flat, np.nonzero(c.match[b])[0])
    # both means run over the batch's union: the image-major concatenation has the selected anchors in the same order
    m, logits, bbox = c.flat()
    assert m.shape == (3 * 1023,) and logits.shape == (3 * 1023, 2) and bbox.shape == (3 * 1023, 4)
    assert np.array_equal(m[m != 0], c.mt)
    assert np.array_equal(logits[1023 + 5], c.heads[0][1, 0, 1, 4:6]) and np.array_equal(bbox[2 * 1023 + 1022], c.heads[4][2, 0, 0, 14:18])
    l_cls, l_box, d_cls, d_box = c.oracle()
    assert l_cls > 0 and l_box > 0 and int((np.abs(d_cls).sum(-1) > 0).sum()) == 600 and int((np.abs(d_box).sum(-1) > 0).sum()) == c.n_pos


def test_rpn_slack_entries_are_valid_unselected_anchors_that_would_change_the_result():
    c = K.rpn_three_passes()
    lvl, idx, mt, target, slack = c.padded()
    assert lvl.shape == idx.shape == mt.shape == (K.RPN_SEL_CAPACITY,) and target.shape == (K.RPN_TARGET_CAPACITY, 4)
    assert np.array_equal(lvl[:600], c.lvl) and np.array_equal(idx[:600], c.idx) and np.array_equal(mt[:600], c.mt)
    assert np.array_equal(target[:c.n_pos], c.target) and np.all(target[c.n_pos:] == 1e3) and np.all(mt[600:] == 1)
    selected = set(zip(c.lvl.tolist(), c.idx.tolist()))
    assert len(slack) == 168 and len(set(slack)) == 168 and not (set(slack) & selected)
    for l, i in slack:
        assert 0 <= l < 5 and 0 <= i < c.B * K.RPN_SIZES[l]
    # read as selected, the slack changes both losses by far more than the test's tolerance
    match = c.match.copy()
    bounds = np.cumsum([0] + K.RPN_SIZES)
    for l, i in slack:
        match[i // K.RPN_SIZES[l], bounds[l] + i % K.RPN_SIZES[l]] = 1
    _, logits, bbox = c.flat()
    l_cls, l_box = c.oracle()[:2]
    assert abs(O.rpn_class_loss(match.reshape(-1), logits)[0] - l_cls) > 1e-3
    assert abs(O.rpn_bbox_loss(target, match.reshape(-1), bbox)[0] - l_box) > 1.0


def test_rpn_all_negative_has_no_positive():
    c = K.rpn_all_negative()
    assert c.n_sel == 600 and c.n_pos == 0 and set(c.mt.tolist()) == {-1}
    l_cls, l_box, _, d_box = c.oracle()
    assert l_cls > 0 and l_box == 0.0 and not d_box.any()


def test_rpn_knee_targets_are_exact_and_straddle_the_knee():
    c = K.rpn_knee()
    assert c.B == 1 and c.n_pos == 3 and c.n_sel == 43
    assert np.array_equal(c.target.astype(np.float64), K.KNEE_TARGETS)                # exactly representable in float32
    _, _, bbox = c.flat()
    assert np.array_equal(np.nonzero(c.match[0] == 1)[0], K.KNEE_ANCHORS) and not bbox[list(K.KNEE_ANCHORS)].any()     # diff = target
    ad = np.abs(K.KNEE_TARGETS).ravel()
    one = F32(1)
    assert {float(one), float(np.nextafter(one, F32(0))), float(np.nextafter(one, F32(2))), 0.5, 0.0, 3.0} == set(ad.tolist())
    for v in (1.0, float(np.nextafter(one, F32(0))), float(np.nextafter(one, F32(2))), 0.5, 3.0):
        assert v in K.KNEE_TARGETS and -v in K.KNEE_TARGETS                           # both signs
    # at |diff| = 1 the loss is 0.5 either way, but the gradient is the outer branch's sign
    l_box, d_box = c.oracle()[1], c.oracle()[3]
    assert abs(d_box[0, 0, 0] + 1 / 12) < 1e-15 and abs(d_box[0, 0, 1] - 1 / 12) < 1e-15 and l_box > 0


# ---- detection targets -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(K.DT_ODD))
def test_dt_odd_counts_and_parities(name):
    c = K.dt_odd(name)
    N = len(c.props)
    assert N % 2 == 1 and N == int(name[1:].split("_")[0]) and N <= 4096
    assert c.nonzero_rows % 2 == K.DT_ODD[name][5]
    _, _, npos, nneg = c.oracle()
    assert npos >= 1                                                                  # something is selected in every case
    if N >= 255:
        assert (npos, nneg) == (66, 134) and c.nonzero_rows < N                       # both lists above their quota; a zero row shifts the compaction
    print(name, N, c.nonzero_rows, npos, nneg)


def test_dt_the_two_257_cases_differ_in_the_parity_of_their_non_zero_rows():
    a, b = K.dt_odd("n257_odd_rows"), K.dt_odd("n257_even_rows")
    assert len(a.props) == len(b.props) == 257 and a.nonzero_rows == 255 and b.nonzero_rows == 256
    assert np.abs(b.props[256]).sum() > 0                                             # the second workgroup's one proposal is a real row


@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("kind", ["identical", "equal_iou"])
def test_dt_tie_is_an_exact_float32_tie_and_the_first_row_wins(kind, swapped):
    c, tied, (g0, g1) = K.dt_first_maximum(kind, swapped)
    ov = O.overlaps_f32(c.props, c.gt)
    with np.errstate(invalid="ignore"):
        for i in tied:
            assert ov[i, g0] == ov[i, g1] and ov[i, g0] >= 0.5 and ov[i, g0] == np.nanmax(ov[i])
    if kind == "identical":
        assert np.array_equal(c.gt[g0], c.gt[g1]) and float(ov[tied[0], g0]) == 1.0
    else:
        assert not np.array_equal(c.gt[g0], c.gt[g1]) and float(ov[tied[0], g0]) == float(F32(0.25) / F32(0.3125))
    assert not np.array_equal(c.caps[g0], c.caps[g1])
    rois, caps, npos, _ = c.oracle()
    rows = [r for r in range(npos) if any(np.array_equal(rois[r], c.props[i]) for i in tied)]
    assert len(rows) == len(tied)
    for r in rows:
        assert np.array_equal(caps[r], c.caps[g0])                                    # the first maximum; `>=` in the argmax would give caps[g1]
    plain, sw = K.dt_first_maximum(kind, False)[0], K.dt_first_maximum(kind, True)[0]
    assert np.array_equal(plain.caps[1], sw.caps[3]) and np.array_equal(plain.gt[1], sw.gt[3])


def test_dt_threshold_sides():
    c = K.dt_threshold()
    iou = c.best_iou()
    assert float(iou[1]) == 0.5 and float(iou[0]) == K.HALF_BELOW and abs(K.HALF_BELOW - 0.49999997) < 1e-8 and iou[2] < 0.1
    rois, _, npos, nneg = c.oracle()
    assert (npos, nneg) == (1, 2) and np.array_equal(rois[0], c.props[1]) and np.array_equal(rois[1], c.props[0])


def test_dt_nan_row_is_present_and_in_neither_list():
    c = K.dt_nan_row()
    ov = O.overlaps_f32(c.props, c.gt)
    assert np.isnan(ov[1, 1]) and int(np.isnan(ov).sum()) == 1 and np.isnan(c.best_iou()[1])
    assert np.abs(c.props[1]).sum() > 0 and np.abs(c.gt[1]).sum() > 0                  # neither is a padding row
    rois, _, npos, nneg = c.oracle()
    assert (npos, nneg) == (2, 3) and int(1 / c.ratio * npos) - npos > nneg           # the quota had room for the NaN row
    assert not any(np.array_equal(r, c.props[1]) for r in rois)
    assert np.array_equal(rois[:5], c.props[[2, 4, 0, 3, 5]])


def test_dt_saturated_lists():
    c = K.dt_all_positive()
    assert len(c.props) == 101 and np.all(c.best_iou() == 1.0)
    assert c.oracle()[2:] == (int(c.n_rois * c.ratio), 0) == (16, 0)
    c = K.dt_no_positive()
    assert len(c.props) == 75 and np.all(c.best_iou() < 0.5)
    rois, caps, npos, nneg = c.oracle()
    assert (npos, nneg) == (0, 0) and not rois.any() and not caps.any()


def test_philox_known_answer():
    """philox2x32 moved here from test_gpu_kernels.py: counter 0, key 0 of Philox-2x32-10 (Random123's known-answer vector, word 0)."""
    assert int(K.philox2x32(np.array([0]), 0, 0)[0]) == 0xFF1DAE59


# ---- RoIAlign --------------------------------------------------------------------------------------------------------------------

def test_roi_boxes_reach_every_level_with_a_margin():
    boxes = K.roi_boxes()
    assert boxes.shape == (2, 70, 4) and boxes.dtype == F32
    assert all(h != w for h, w in K.ROI_HW)
    lv = O.roi_levels(boxes, K.ROI_IMAGE)
    rnd = K.roi_random_mask()
    assert int(rnd.sum()) == 2 * 70 - len(K.ROI_LITERALS)
    for level in (2, 3, 4, 5):
        assert int(((lv == level) & rnd).sum()) >= 8, level
    f = K.roi_float_level(boxes)[rnd].astype(np.float64)
    assert np.all(np.isfinite(f)) and float(np.abs(f - np.floor(f) - 0.5).min()) >= K.ROI_MARGIN
    b = boxes[rnd]
    assert np.all(b[:, 2] > b[:, 0]) and np.all(b[:, 3] > b[:, 1]) and b.min() >= 0 and b.max() <= 1
    ar = (b[:, 2] - b[:, 0]) / (b[:, 3] - b[:, 1])
    assert ar.min() < 0.7 and ar.max() > 1.4                                          # not square: h and w differ as well as H and W


def test_roi_literal_boxes_are_what_their_names_say():
    boxes = K.roi_boxes()
    lv = O.roi_levels(boxes, K.ROI_IMAGE)
    at = {n: (boxes[i, j], int(lv[i, j])) for n, (i, j, _) in K.ROI_LITERALS.items()}
    for n in ("zero_a", "zero_b", "zero_c"):
        assert not at[n][0].any() and at[n][1] == 2
    b, level = at["flipped_both"]
    assert b[2] < b[0] and b[3] < b[1] and level == 3
    b, level = at["flipped_y"]
    assert b[2] < b[0] and b[3] > b[1] and (b[2] - b[0]) * (b[3] - b[1]) < 0 and level == 2
    assert at["full"][0].tolist() == [0, 0, 1, 1] and at["full"][1] == 5
    b, level = at["overrun"]
    assert b[0] < 0 and b[1] < 0 and b[2] > 1 and b[3] > 1 and level == 5
    assert np.isnan(at["nan"][0]).any() and at["nan"][1] == 2
    for n in ("flipped_both", "full", "overrun"):                                      # the literal boxes keep the routing margin too
        f = float(K.roi_float_level(at[n][0]))
        assert abs(f - np.floor(f) - 0.5) >= K.ROI_MARGIN
    assert sum(j >= 64 for _, j, _ in K.ROI_LITERALS.values()) >= 4                    # the ragged second round of 64 boxes sees special cases


@pytest.mark.parametrize("pool", [1, 2, 7, 16])
def test_roi_oracle_rows_of_the_special_boxes(pool):
    """The NaN box's forward rows are zero and it adds nothing in the backward; the overrunning box has zero rows and rows inside; the
    flipped boxes read the map (their rows are not zero)."""
    boxes, C = K.roi_boxes(), 4
    maps = [m + 3.0 for m in K.roi_maps(C, 1)]                                        # far from 0: a sample that was read shows
    out = O.pyramid_roi_align(boxes, maps, K.ROI_IMAGE, pool)
    i, j, _ = K.ROI_LITERALS["nan"]
    assert not out[i, j].any()
    one = np.zeros((2, 70, pool, pool, C))
    one[i, j] = 1.0
    assert not any(g.any() for g in O.pyramid_roi_align_backward(boxes, [m.shape for m in maps], K.ROI_IMAGE, one))
    i, j, _ = K.ROI_LITERALS["overrun"]
    zero = ~out[i, j].any(axis=-1)
    assert {1: not zero.any(), 2: zero.all()}.get(pool, zero[0].all() and zero[:, -1].all() and not zero[3:-3, 3:-3].any())
    for n in ("flipped_both", "flipped_y", "full", "zero_a"):
        i, j, _ = K.ROI_LITERALS[n]
        assert out[i, j].all()


def test_roi_sweep_reaches_every_accumulator_and_tail():
    assert {p for p, _ in K.ROI_SWEEP} == {1, 2, 7, 16} and {c for _, c in K.ROI_SWEEP} == {4, 260, 512, 1024}
    assert all(p <= 7 for p, c in K.ROI_SWEEP if c >= 512)
    assert all(c % 4 == 0 and c <= 1024 for _, c in K.ROI_SWEEP)
    assert (260 // 4) % 64 == 1 and 260 > 256 and (1024 // 4 + 63) // 64 == 4           # a one-lane second chunk; all four accumulators


def test_integral_samples_are_pixels_in_float32():
    boxes, rows, cols = K.integral_boxes()
    assert boxes.shape == (1, 10, 4) and np.all(O.roi_levels(boxes, K.INTEGRAL_IMAGE) == 2)
    H, W = K.INTEGRAL_HW[0]
    assert (H, W) == (13, 25)
    in_y, in_x = K.integral_sample_coordinates(boxes)
    assert in_y.dtype == F32 and np.array_equal(in_y, rows) and np.array_equal(in_x, cols)      # integers, the stated ones
    assert rows.min() >= 0 and rows.max() <= H - 1 and cols.min() >= 0 and cols.max() <= W - 1
    assert int((boxes[0, :, 2] < boxes[0, :, 0]).sum()) == 2 and int((boxes[0, :, 3] < boxes[0, :, 1]).sum()) == 1
    assert any(float(v) * 12 != round(float(v) * 12) for v in boxes[0, :, 0])                   # not only corners exact in binary
    # the oracle agrees: every forward row is a map row
    maps = K.roi_maps(8, 3, B=1, hw=K.INTEGRAL_HW)
    out = O.pyramid_roi_align(boxes, maps, K.INTEGRAL_IMAGE, 7)
    for r in range(10):
        np.testing.assert_array_equal(out[0, r], maps[0][0][rows[r]][:, cols[r]])
