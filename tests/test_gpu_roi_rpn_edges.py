"""The three kernels between the encoder and the decoder of the joint train step on the branches their other direct tests do not take
(-m gpu): dc_rpn_loss_grad_f32 in the train step's call form (batched heads, device counts, fixed capacities, three passes of the
one-block loop), dc_detection_targets_f32 at odd proposal counts, exact ties, the 0.5 threshold, a NaN row and saturated lists, and
dc_roi_align_pyramid_f32 / _bwd_f32 on non-square maps over pool 1..16 and C 4..1024.  The reference is oracle/np_oracle.py throughout;
the inputs are _roi_rpn_cases.py's, and test_roi_rpn_cases.py (CPU) proves that they hold what the tests below rely on.

What a wrong kernel would show, case by case: a loop that stops after one pass leaves the gradients of selected anchors 256.. zero
and both losses short (three_passes); a rank counted within the pass regresses pass 2's positives to pass 1's target rows (three_passes:
positives in every pass); ignored device counts read the slack (capacity_clamp: other finite numbers); `iou >= best` takes the second
tied GT row's caption (first_maximum, both orders); `best > 0.5f` loses the one positive (threshold); without the odd-N entry the
last pair's second word is whatever the LDS held, and every rank may be one too high (odd counts, bit-exact rows); H and W swapped in
one roi_sample call moves every sample of a 24 x 40 map (sweep, integral samples); accumulators k >= 1 not stored leave channels
256.. of the gradient maps at their old value (C = 260, 512, 1024)."""
import numpy as np
import pytest
import torch

from image_captioning_amd._lib import DcapError

import _roi_rpn_cases as K
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def close(got, want, tol=2e-5):
    got = (got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)).astype(np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    assert err < tol, "max err %.3e (scaled) exceeds %.1e" % (err, tol)


# ---------------------------------------------------------------------------------------------
# 1. RPN losses in the train step's call form
# ---------------------------------------------------------------------------------------------
FILL = 7.0            # what dheads hold before a launch that must not write them


def _rpn_run(ops, case, lvl, idx, mt, target, n_pos, counts=None, fill=0.0):
    """One launch over the batched heads; returns (losses [2], dheads as NumPy arrays)."""
    heads = [dev(h) for h in case.heads]
    dh = [torch.full(h.shape, fill, device="cuda") for h in heads]
    losses = torch.full((2,), 9.0, device="cuda")
    i32 = lambda a: dev(a, torch.int32)
    ops.rpn_loss_grad(heads, dh, i32(lvl), i32(idx), i32(mt), dev(target), n_pos, losses, anchors_per_loc=K.RPN_A,
                      counts_dev=None if counts is None else i32(counts), batched=True)
    return losses.cpu().numpy(), [d.cpu().numpy() for d in dh]


def _rpn_check(case, losses, dh, tol=1e-5):
    """Both losses and every level's gradient at every image against the oracle; what no selected anchor owns stays exactly zero."""
    A = K.RPN_A
    l_cls, l_box, d_cls, d_box = case.oracle()
    print("rpn losses: device %r oracle (%.9g, %.9g)" % (losses.tolist(), l_cls, l_box))
    close(losses, np.array([l_cls, l_box]), tol)
    bounds = np.cumsum([0] + K.RPN_SIZES)
    for l, (h, w) in enumerate(K.RPN_SHAPES):
        got = dh[l]
        assert got.shape == (case.B, h, w, K.RPN_STRIDE)
        assert not got[..., 6 * A:].any()                                               # the padding columns
        for b in range(case.B):
            want_c, want_b = d_cls[b, bounds[l]:bounds[l + 1]], d_box[b, bounds[l]:bounds[l + 1]]
            got_c, got_b = got[b, :, :, :2 * A].reshape(-1, 2), got[b, :, :, 2 * A:6 * A].reshape(-1, 4)
            close(got_c, want_c, tol)
            close(got_b, want_b, tol)
            m = case.match[b, bounds[l]:bounds[l + 1]]
            assert not got_c[m == 0].any() and not got_b[m != 1].any()                  # every non-selected anchor, exactly
            assert np.all(np.abs(got_c[m != 0]).sum(1) > 0)                             # every selected one was visited


@pytest.fixture(scope="module")
def three_passes(ops):
    """The three-pass batch with exact-size buffers and host counts: (case, losses, dheads)."""
    case = K.rpn_three_passes()
    return (case,) + _rpn_run(ops, case, case.lvl, case.idx, case.mt, case.target, case.n_pos)


def test_rpn_three_passes_of_the_one_block_loop(three_passes):
    """B = 3, 230 + 256 + 114 = 600 selected anchors, positives in each pass of 256 and in each image: losses and all five dheads at
    every image at the existing test's 1e-5 (the 600-term sums need no more room: per-thread partials of at most three terms and an
    8-level tree keep the float32 error near 1e-7)."""
    case, losses, dh = three_passes
    _rpn_check(case, losses, dh)


def test_rpn_capacity_clamp_equals_the_exact_size_call_bit_for_bit(ops, three_passes):
    """sel_* of capacity 768, target rows of capacity 384, counts_dev = {600, n_pos}, the host n_pos argument the capacity: the slack
    (valid unselected anchors with match 1, target rows 1e3) must not be read."""
    case, want_losses, want_dh = three_passes
    lvl, idx, mt, target, _ = case.padded()
    losses, dh = _rpn_run(ops, case, lvl, idx, mt, target, K.RPN_TARGET_CAPACITY, counts=[case.n_sel, case.n_pos])
    assert np.array_equal(losses, want_losses)
    for got, want in zip(dh, want_dh):
        assert np.array_equal(got, want)
    _rpn_check(case, losses, dh)


def test_rpn_empty_forms_through_the_device_counts(ops):
    """{n_sel, 0} with every match -1: the bbox loss is exactly 0 and no bbox column is written; {0, 0}: both losses exactly 0, dheads
    untouched.  The buffers keep their capacities, their slack says otherwise."""
    case = K.rpn_all_negative()
    lvl, idx, mt, target, _ = case.padded()
    assert np.all(target == 1e3)
    losses, dh = _rpn_run(ops, case, lvl, idx, mt, target, K.RPN_TARGET_CAPACITY, counts=[case.n_sel, 0], fill=FILL)
    l_cls, _, d_cls, _ = case.oracle()
    close(losses[:1], np.array([l_cls]), 1e-5)
    assert losses[1] == 0.0
    A = K.RPN_A
    bounds = np.cumsum([0] + K.RPN_SIZES)
    for l, got in enumerate(dh):
        assert np.all(got[..., 2 * A:] == FILL)                                        # no bbox column, no padding column
        for b in range(case.B):
            m = case.match[b, bounds[l]:bounds[l + 1]]
            got_c = got[b, :, :, :2 * A].reshape(-1, 2)
            assert np.all(got_c[m == 0] == FILL)
            close(np.where((m != 0)[:, None], got_c, 0.0), d_cls[b, bounds[l]:bounds[l + 1]], 1e-5)
    full = K.rpn_three_passes()
    lvl, idx, mt, target, _ = full.padded()
    losses, dh = _rpn_run(ops, full, lvl, idx, mt, target, K.RPN_TARGET_CAPACITY, counts=[0, 0], fill=FILL)
    assert losses.tolist() == [0.0, 0.0]
    assert all(np.all(got == FILL) for got in dh)


def test_rpn_smooth_l1_around_the_knee(ops):
    """|diff| = 1, 1 -+ one ulp, 0.5, 0 and 3 with both signs, every diff exact in float32 (the bbox outputs are 0): the loss and
    every gradient against the oracle; at |diff| = 1 the gradient is the linear branch's -+1 / 12 like the reference's `< 1.0`."""
    case = K.rpn_knee()
    for counts in (None, [case.n_sel, case.n_pos]):
        losses, dh = _rpn_run(ops, case, case.lvl, case.idx, case.mt, case.target, case.n_pos, counts=counts)
        _rpn_check(case, losses, dh)
        g = dh[0][0, 0, 0, 2 * K.RPN_A:2 * K.RPN_A + 4]                                  # anchor 0: targets 1, -1, 1 - ulp, -(1 - ulp)
        assert g[0] == -g[1] == np.float32(-1.0) * (np.float32(1) / np.float32(12)) and g[2] == -g[3]


# ---------------------------------------------------------------------------------------------
# 2. detection targets: parity, ties, thresholds (bit-exact)
# ---------------------------------------------------------------------------------------------
DT_SEEDS = [None, 1234]


def _dt_check(ops, case, seed, offset=81):
    """The device against O.detection_targets: RoIs, captions and counts bit-exact (test_gpu_kernels.py's check)."""
    step = torch.tensor([5], dtype=torch.int32, device="cuda")
    rois, oc, counts = ops.detection_targets(dev(case.props), dev(case.gt), dev(case.caps, torch.int32), case.n_rois, case.ratio, seed=seed,
                                             offset=offset, offset_dev=step if seed is not None else None)
    shuffle = None
    if seed is not None:
        keys = K.philox2x32(np.arange(len(case.props)), offset + 5, seed)
        shuffle = lambda idx: idx[np.lexsort((idx, keys[idx]))]
    want_rois, want_caps, npos, nneg = case.oracle(shuffle)
    rois, oc = rois.cpu().numpy(), oc.cpu().numpy()
    assert counts.cpu().numpy().tolist() == [npos, nneg]
    assert np.array_equal(rois, want_rois)
    assert np.array_equal(oc, want_caps)
    return rois, oc, npos, nneg


@pytest.mark.parametrize("seed", DT_SEEDS)
@pytest.mark.parametrize("name", sorted(K.DT_ODD))
def test_detection_targets_odd_proposal_counts(ops, name, seed):
    """N = 1, 3, 255, 257 (odd and even number of non-zero rows: the second workgroup ranks one proposal), 1023, 4095: the odd-N pair
    list with its closing entry above every real one."""
    _dt_check(ops, K.dt_odd(name), seed)


@pytest.mark.parametrize("seed", DT_SEEDS)
@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("kind", ["identical", "equal_iou"])
def test_detection_targets_take_the_first_maximum(ops, kind, swapped, seed):
    case, tied, (g0, _) = K.dt_first_maximum(kind, swapped)
    rois, caps, npos, _ = _dt_check(ops, case, seed)
    rows = [r for r in range(npos) if any(np.array_equal(rois[r], case.props[i]) for i in tied)]
    assert len(rows) == len(tied) and all(np.array_equal(caps[r], case.caps[g0]) for r in rows)


@pytest.mark.parametrize("seed", DT_SEEDS)
def test_detection_targets_threshold_is_inclusive_at_exactly_one_half(ops, seed):
    case = K.dt_threshold()
    rois, _, npos, nneg = _dt_check(ops, case, seed)
    assert (npos, nneg) == (1, 2) and np.array_equal(rois[0], case.props[1])
    assert sorted(rois[1:3, 2].tolist()) == sorted(case.props[[0, 2], 2].tolist())       # the float32 below 0.5 is a negative


@pytest.mark.parametrize("seed", DT_SEEDS)
def test_detection_targets_nan_row_is_in_neither_list(ops, seed):
    case = K.dt_nan_row()
    rois, _, npos, nneg = _dt_check(ops, case, seed)
    assert (npos, nneg) == (2, 3) and not any(np.array_equal(r, case.props[1]) for r in rois)


@pytest.mark.parametrize("seed", DT_SEEDS)
def test_detection_targets_saturated_lists(ops, seed):
    _, _, npos, nneg = _dt_check(ops, K.dt_all_positive(), seed)
    assert (npos, nneg) == (16, 0)
    rois, caps, npos, nneg = _dt_check(ops, K.dt_no_positive(), seed)
    assert (npos, nneg) == (0, 0) and not rois.any() and not caps.any()


# ---------------------------------------------------------------------------------------------
# 3. RoIAlign forward and backward off the square 7 x 7 x 256 path
# ---------------------------------------------------------------------------------------------

def _roi_check(ops, boxes, pool, C, image=K.ROI_IMAGE, hw=K.ROI_HW):
    """Forward (1e-5), routing (bit-exact), backward into non-zero maps (3e-5) and the adjoint identity, all against the oracle."""
    B, R = boxes.shape[:2]
    area = float(image[0] * image[1])
    maps, base, g = K.roi_maps(C, 1, B, hw), K.roi_maps(C, 2, B, hw), K.roi_grad(R, pool, C, 3, B)
    lv = torch.full((B * R,), -1, dtype=torch.int32, device="cuda")
    bx = dev(boxes)
    fwd = ops.roi_align_pyramid([dev(m) for m in maps], bx, area, pool, levels_out=lv).cpu().numpy()
    np.testing.assert_array_equal(lv.cpu().numpy().reshape(B, R), O.roi_levels(boxes, image))
    close(fwd, O.pyramid_roi_align(boxes, maps, image, pool), 1e-5)
    dm = [dev(b) for b in base]
    ops.roi_align_pyramid_bwd(dm, bx, area, dev(g), pool)
    got = [d.cpu().numpy() for d in dm]
    want = O.pyramid_roi_align_backward(boxes, [m.shape for m in maps], image, g)
    for d, w, b in zip(got, want, base):
        close(d, w + b, 3e-5)
    lhs = float((fwd.astype(np.float64) * g).sum())
    rhs = sum(float(((d.astype(np.float64) - b) * m).sum()) for d, b, m in zip(got, base, maps))
    print("adjoint: <fwd, g> %.9g <maps, bwd> %.9g" % (lhs, rhs))
    assert abs(lhs - rhs) < 1e-4 * max(1.0, abs(lhs))
    return fwd, got, base


@pytest.mark.parametrize("pool,C", K.ROI_SWEEP)
def test_roi_align_on_non_square_maps(ops, pool, C):
    """B = 2, R = 70 (a ragged second round of the backward's 64-box ballot), maps 24 x 40 .. 3 x 5, every level populated, zero,
    flipped, full-image, overrunning and NaN boxes among them."""
    boxes = K.roi_boxes()
    fwd, _, _ = _roi_check(ops, boxes, pool, C)
    i, j, _ = K.ROI_LITERALS["nan"]
    assert not fwd[i, j].any()


@pytest.mark.parametrize("R", [1, 64, 65])
def test_roi_align_box_counts_around_one_ballot_round(ops, R):
    boxes = K.roi_boxes()
    _roi_check(ops, boxes[:, 5:6] if R == 1 else boxes[:, :R], 7, 260)


def test_roi_align_integral_samples_copy_and_add_whole_rows(ops):
    """Level-2 maps of 13 x 25 and boxes whose 7 x 7 samples are pixels: the forward rows ARE the map rows (bit for bit: both
    interpolation weights are 0) and the backward adds each g row once to one pixel -- with integer-valued g and maps, exactly."""
    boxes, rows, cols = K.integral_boxes()
    C, hw, image = 8, K.INTEGRAL_HW, K.INTEGRAL_IMAGE
    area = float(image[0] * image[1])
    maps = K.roi_maps(C, 4, 1, hw)
    fwd = ops.roi_align_pyramid([dev(m) for m in maps], dev(boxes), area, 7).cpu().numpy()
    for r in range(boxes.shape[1]):
        np.testing.assert_array_equal(fwd[0, r], maps[0][0][rows[r]][:, cols[r]])
    rng = np.random.default_rng(9)
    g = rng.integers(-8, 9, (1, boxes.shape[1], 7, 7, C)).astype(np.float32)
    base = [rng.integers(-8, 9, (1, h, w, C)).astype(np.float32) for h, w in hw]
    dm = [dev(b) for b in base]
    ops.roi_align_pyramid_bwd(dm, dev(boxes), area, dev(g), 7)
    want = [b.astype(np.float64) for b in base]
    for r in range(boxes.shape[1]):
        for py in range(7):
            for px in range(7):
                want[0][0, rows[r, py], cols[r, px]] += g[0, r, py, px]
    for w, o, b in zip(want, O.pyramid_roi_align_backward(boxes, [b.shape for b in base], image, g), base):
        np.testing.assert_array_equal(w, o + b)                                         # the oracle says the same
    for d, w in zip(dm, want):
        np.testing.assert_array_equal(d.cpu().numpy(), w)
    _roi_check(ops, boxes, 7, C, image, hw)


def test_roi_align_backward_refuses_pool_17_and_1028_channels(ops):
    """Above RA_MAX_POOL and above four accumulators of 256 channels the backward raises and launches nothing."""
    boxes = dev(K.roi_boxes()[:, :4])
    for pool, C in ((17, 8), (7, 1028)):
        dm = [torch.full((2, h, w, C), FILL, device="cuda") for h, w in K.ROI_HW]
        with pytest.raises(DcapError):
            ops.roi_align_pyramid_bwd(dm, boxes, 512.0 * 512.0, torch.ones(2, 4, pool, pool, C, device="cuda"), pool)
        torch.cuda.synchronize()
        assert all(bool((d == FILL).all()) for d in dm)
