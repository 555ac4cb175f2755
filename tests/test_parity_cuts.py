"""The parity-cut checkers of tests/_parity_cuts.py shown failing (no GPU, no library load): a checker that cannot fail is worth
nothing, so each one passes its clean case and fails on a planted error, for the stated reason.  The arrays are tiny and built with the
oracle itself; the 'device' side is the oracle's result rounded to float32."""
import types

import numpy as np
import pytest

from oracle import np_models as M
from oracle import np_oracle as O

import _parity_cuts as PC

R = 6


@pytest.fixture(scope="module")
def head():
    """Six RoIs through the oracle's head: weights, cache (with the magnitude sums), an upstream gradient of dyadic values (its column
    sums are exact in float64) and the float32 'device' buffers."""
    rng = np.random.default_rng(11)
    W = {'mrcnn_class_conv1/kernel': (0.01 * rng.standard_normal((7, 7, 256, 1024))).astype(np.float32),
         'mrcnn_class_conv2/kernel': (0.05 * rng.standard_normal((1, 1, 1024, 1024))).astype(np.float32)}
    for conv, bn in PC.HEAD:
        W[conv + '/bias'] = (0.01 * rng.standard_normal(1024)).astype(np.float32)
        W[bn + '/gamma'] = rng.uniform(0.5, 1.5, 1024).astype(np.float32)
        W[bn + '/beta'] = (0.1 * rng.standard_normal(1024)).astype(np.float32)
        W[bn + '/moving_mean'] = (0.1 * rng.standard_normal(1024)).astype(np.float32)
        W[bn + '/moving_variance'] = rng.uniform(0.5, 1.5, 1024).astype(np.float32)
    feat = rng.standard_normal((R, 7, 7, 256)).astype(np.float32)
    f, cache = M.roi_head_forward(feat, W, mag=True)
    df = rng.integers(-64, 65, f.shape).astype(np.float64) / 64.0
    df[df == 0] = 1.0
    return types.SimpleNamespace(W=W, cache=cache, df=df)


def _device_side(h):
    """(dev_acc, dev_hact, oracle_cache) of the clean case; all arrays are fresh copies."""
    c = h.cache
    aux = dict(head_z=(c['z1'].copy(), c['z2'].copy()), head_mag=(c['mag1'], c['mag2']), head_acc=(c['acc1'], c['acc2']))
    acc = [c['acc1'].astype(np.float32), c['acc2'].astype(np.float32)]
    hact = [np.maximum(c['z1'], 0).astype(np.float32), np.maximum(c['z2'], 0).astype(np.float32)]
    return acc, hact, PC.oracle_head_cache(aux)


def test_head_cache_carries_the_preactivations_and_the_magnitude_sums(head):
    c = head.cache
    assert np.array_equal(c['a1'], np.maximum(c['z1'], 0)) and np.array_equal(c['f'], np.maximum(c['z2'], 0))
    np.testing.assert_allclose(c['mag1'], np.abs(c['x']) @ np.abs(c['K1']), rtol=1e-14)
    np.testing.assert_allclose(c['mag2'], np.abs(c['a1']) @ np.abs(c['K2']), rtol=1e-14)
    assert np.all(np.abs(c['acc1']) <= c['mag1']) and np.all(np.abs(c['acc2']) <= c['mag2'])
    assert 'mag1' not in M.roi_head_forward(c['x'].reshape(R, 7, 7, 256), head.W)[1]          # the sums are computed on request only


def test_head_backward_with_its_own_masks_is_bit_identical(head):
    c = head.cache
    a = M.roi_head_backward(head.df, c)
    b = M.roi_head_backward(head.df, c, masks=(c['a1'] > 0, c['f'] > 0))
    assert set(a) == set(b)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_one_flipped_layer2_mask_entry_moves_exactly_its_channel(head):
    """Layer-2 mask entry (r, c) switched on: bn2/beta[c] moves by df[r, c] (exactly: the terms are dyadic), bn2/gamma[c] by
    df[r, c] n2[r, c], conv2/bias[c] by df[r, c] g2[c] / s2[c]; every other channel of the three keeps its bits."""
    c, df = head.cache, head.df
    m1, m2 = c['a1'] > 0, c['f'] > 0
    r, ch = (int(v) for v in np.argwhere(~m2)[7])
    flipped = m2.copy()
    flipped[r, ch] = True
    a = M.roi_head_backward(df, c, masks=(m1, m2))
    b = M.roi_head_backward(df, c, masks=(m1, flipped))
    others = np.arange(1024) != ch
    d = df[r, ch]
    assert b['mrcnn_class_bn2/beta'][ch] - a['mrcnn_class_bn2/beta'][ch] == d and d != 0
    for key, step in (('mrcnn_class_bn2/gamma', d * c['n2'][r, ch]), ('mrcnn_class_conv2/bias', d * c['g2'][ch] / c['s2'][ch])):
        scale = np.abs(a[key][ch]) + np.abs(step) + R * np.abs(c['n2'][:, ch]).max()
        assert abs((b[key][ch] - a[key][ch]) - step) <= 1e-13 * scale, key
        assert abs(step) > 1e-6, key                                                   # a move a 5e-4 tolerance on the tensor would see
    for key in ('mrcnn_class_bn2/beta', 'mrcnn_class_bn2/gamma', 'mrcnn_class_conv2/bias'):
        assert np.array_equal(a[key][others], b[key][others]), key
    # (the kernel gradient: only column ch of conv2/kernel moves)
    ka, kb = a['mrcnn_class_conv2/kernel'].reshape(1024, 1024), b['mrcnn_class_conv2/kernel'].reshape(1024, 1024)
    assert np.array_equal(ka[:, others], kb[:, others]) and not np.array_equal(ka[:, ch], kb[:, ch])


def test_head_kinks_threshold():
    z = np.array([[1e-9, -2e-6, 3e-6, 0.5]])
    mag, gamma, sd, extra = np.full((1, 4), 100.0), np.array([1.0, -2.0, 1.0, 1.0]), np.array([1.0, 1.0, 2.0, 1.0]), np.full((1, 4), 2.0)
    C, t = PC.head_kinks(z, mag, gamma, sd, extra, 4.0)
    u = 2.0 ** -24
    np.testing.assert_allclose(t, [[4 * u * 100 + 16 * u, 8 * u * 100 + 16 * u, 2 * u * 100 + 16 * u, 4 * u * 100 + 16 * u]], rtol=1e-15)
    assert C.tolist() == [[True, True, True, False]]
    assert PC.head_kinks(z, mag, gamma, sd, extra, 0.25)[0].tolist() == [[True, True, False, False]]            # 66 u and 28.5 u


def test_check_head_decisions_clean_case_passes_and_reports(head):
    acc, hact, oc = _device_side(head)
    masks, report = PC.check_head_decisions(acc, hact, oc, head.W, c_acc=(4.0, 4.0))
    assert np.array_equal(masks[0], head.cache['a1'] > 0) and np.array_equal(masks[1], head.cache['f'] > 0)
    for li in (1, 2):
        rep = report["layer%d" % li]
        assert rep["disagreements"] == [] and rep["acc_ratio"] <= 0.5 and rep["close_set"] <= 2       # float32 rounding of acc: u / 2 of |acc| <= mag


@pytest.mark.parametrize("layer", [0, 1])
def test_check_head_decisions_fails_on_a_flipped_entry_far_from_zero(head, layer):
    acc, hact, oc = _device_side(head)
    r, c = np.unravel_index(int(np.abs(oc['z'][layer]).argmax()), oc['z'][layer].shape)
    hact[layer][r, c] = 0.0 if hact[layer][r, c] > 0 else 1.0
    with pytest.raises(AssertionError, match=r"head layer %d: 1 ReLU decision\(s\) differ outside the close set; first at \(row %d, channel %d\)" % (layer + 1, r, c)):
        PC.check_head_decisions(acc, hact, oc, head.W, c_acc=(4.0, 4.0))


def test_check_head_decisions_accepts_and_reports_a_flip_inside_the_close_set(head):
    acc, hact, oc = _device_side(head)
    r, c = 2, 300
    oc['z'][1][r, c] = 1e-12                                   # the oracle: just positive; the device: zero
    hact[1][r, c] = 0.0
    masks, report = PC.check_head_decisions(acc, hact, oc, head.W, c_acc=(4.0, 4.0))
    assert not masks[1][r, c]
    assert [(d["row"], d["channel"], d["z64"]) for d in report["layer2"]["disagreements"]] == [(r, c, 1e-12)]
    assert report["layer2"]["close_set"] >= 1 and report["layer1"]["disagreements"] == []


def test_check_head_decisions_fails_when_the_close_set_exceeds_the_cap(head):
    acc, hact, oc = _device_side(head)
    oc['z'][0][0, :PC.CLOSE_SET_CAP + 1] = 1e-12
    hact[0][0, :PC.CLOSE_SET_CAP + 1] = 1e-12
    with pytest.raises(AssertionError, match="head layer 1: .* pre-activations within rounding of zero .cap 64.: choose another image seed"):
        PC.check_head_decisions(acc, hact, oc, head.W, c_acc=(4.0, 4.0))


def test_check_head_decisions_fails_on_a_gemm_output_off_by_more_than_the_bound(head):
    acc, hact, oc = _device_side(head)
    acc[0][3, 17] += np.float32(40 * PC.U32 * oc['mag'][0][3, 17])
    with pytest.raises(AssertionError, match=r"head layer 1: acc at \(3, 17\)"):
        PC.check_head_decisions(acc, hact, oc, head.W, c_acc=(4.0, 4.0))


def test_the_stated_constant_is_below_the_worst_case_bound():
    assert len(PC.C_ACC) == 2 and all(0 < c <= k for c, k in zip(PC.C_ACC, PC.HEAD_K))
    assert all(np.log2(c) == int(np.log2(c)) for c in PC.C_ACC)


# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sample():
    """Two images: 40 proposals each, GT boxes = some of the image's own proposals (so positive RoIs exist), different GT counts and captions."""
    rng = np.random.default_rng(5)
    H = W = 128
    cfg = types.SimpleNamespace(TRAIN_ROIS_PER_IMAGE=12, ROI_POSITIVE_RATIO=0.33)
    props = np.zeros((2, 48, 4), np.float32)
    for b in range(2):
        y, x = rng.uniform(0, 0.6, 40), rng.uniform(0, 0.6, 40)
        props[b, :40] = np.stack([y, x, y + rng.uniform(0.2, 0.4, 40), x + rng.uniform(0.2, 0.4, 40)], axis=1)
    gt_boxes = np.zeros((2, 6, 4), np.int32)
    gt_boxes[0, :3] = np.rint(props[0, [1, 5, 9]] * 128)
    gt_boxes[1, :2] = np.rint(props[1, [0, 7]] * 128)
    gt_caps = np.zeros((2, 6, 5), np.int32)
    gt_caps[0, :3] = [[1, 5, 2, 0, 0], [1, 6, 7, 2, 0], [1, 8, 2, 0, 0]]
    gt_caps[1, :2] = [[1, 9, 10, 11, 2], [1, 12, 2, 0, 0]]
    gt_norm = (gt_boxes.astype(np.float32) / np.float32(128)).astype(np.float32)
    out = [O.detection_targets(props[b], gt_caps[b], gt_norm[b], 12, 0.33, None) for b in range(2)]
    tg = dict(rois=np.stack([o[0] for o in out]), caps=np.stack([o[1] for o in out]), npos=np.array([o[2] for o in out]), nneg=np.array([o[3] for o in out]))
    assert np.all(tg['npos'] > 0) and np.all(tg['nneg'] > 0)
    return types.SimpleNamespace(tg=tg, props=props, gt_caps=gt_caps, gt_boxes=gt_boxes, H=H, W=W, cfg=cfg)


def test_check_sample_clean_case_passes(sample):
    s = sample
    PC.check_sample(s.tg, s.props, s.gt_caps, s.gt_boxes, s.H, s.W, s.cfg)
    one = dict(rois=s.tg['rois'][1], caps=s.tg['caps'][1], npos=int(s.tg['npos'][1]), nneg=int(s.tg['nneg'][1]))      # IMAGES_PER_GPU = 1: no image axis
    PC.check_sample(one, s.props[1:], s.gt_caps[1:], s.gt_boxes[1:], s.H, s.W, s.cfg)
    for b in range(2):
        PC.assert_rois_are_proposals(s.tg['rois'][b], s.tg['npos'][b] + s.tg['nneg'][b], s.props[b])


def test_check_sample_fails_when_the_images_gt_captions_are_swapped(sample):
    s = sample
    with pytest.raises(AssertionError, match="sampled target row.s. differ from the GT rows"):
        PC.check_sample(s.tg, s.props, s.gt_caps[::-1], s.gt_boxes, s.H, s.W, s.cfg)


def test_check_sample_fails_when_the_images_gt_boxes_are_swapped(sample):
    s = sample
    with pytest.raises(AssertionError, match="image 0: "):
        PC.check_sample(s.tg, s.props, s.gt_caps, s.gt_boxes[::-1], s.H, s.W, s.cfg)


def test_check_sample_fails_when_one_roi_row_is_moved(sample):
    s = sample
    tg = {k: np.array(v) for k, v in s.tg.items()}
    n = int(tg['npos'][1])
    tg['rois'][1, [n, n + 1]] = tg['rois'][1, [n + 1, n]]                  # two negatives out of proposal order
    with pytest.raises(AssertionError, match="image 1: 2 sampled RoI row.s. differ"):
        PC.check_sample(tg, s.props, s.gt_caps, s.gt_boxes, s.H, s.W, s.cfg)
    with pytest.raises(AssertionError, match="none of the device's proposals"):
        PC.assert_rois_are_proposals(tg['rois'][0] + np.float32(1e-6), 3, s.props[0])


def test_compare_proposals_fails_on_two_swapped_entries_of_the_order():
    rng = np.random.default_rng(3)
    S, strides, scales, ratios = 64, [4, 8, 16, 32, 64], (32, 64, 128, 256, 512), [0.5, 1, 2]
    shapes = [[S // s, S // s] for s in strides]
    anchors = O.generate_pyramid_anchors(scales, ratios, shapes, strides, 1).astype(np.float32)
    n = anchors.shape[0]
    scores = rng.random(n).astype(np.float32)
    deltas = (0.5 * rng.standard_normal((n, 4))).astype(np.float32)
    want, ix, kp = O.proposal_layer(scores, deltas, anchors, (S, S), n, 0.7)
    keep = np.full(n, -1, np.int32)
    keep[:len(kp)] = kp
    assert 50 < len(kp) < n                                   # NMS suppressed some: there is padding to check
    PC.compare_proposals(want, ix, keep, want, ix, kp)
    swapped = ix.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    with pytest.raises(AssertionError):
        PC.compare_proposals(want, swapped, keep, want, ix, kp)
    moved = want.copy()
    moved[[0, 1]] = moved[[1, 0]]
    with pytest.raises(AssertionError):
        PC.compare_proposals(moved, ix, keep, want, ix, kp)
    padded = want.copy()
    padded[-1] = 0.25
    with pytest.raises(AssertionError):
        PC.compare_proposals(padded, ix, keep, want, ix, kp)


def test_check_rpn_heads_compares_per_level_and_per_image():
    """A stand-in plan of two images and two levels (fused heads: 6 class logits, 12 deltas, 2 padding channels): the clean case passes
    whatever the padding holds; the two images' heads swapped on one level fail."""
    rng = np.random.default_rng(9)
    A, shapes = 3, [(4, 4), (2, 2)]
    auxes = [dict(rpn_cls={2 + i: rng.standard_normal((1, h, w, 2 * A)) for i, (h, w) in enumerate(shapes)},
                  rpn_box={2 + i: rng.standard_normal((1, h, w, 4 * A)) for i, (h, w) in enumerate(shapes)}) for _ in range(2)]
    heads = []
    for i, (h, w) in enumerate(shapes):
        hd = np.full((2, h, w, 20), np.nan, np.float32)
        for b in range(2):
            hd[b, ..., :6], hd[b, ..., 6:18] = auxes[b]['rpn_cls'][2 + i][0], auxes[b]['rpn_box'][2 + i][0]
        heads.append(hd)
    errs = PC.check_rpn_heads(types.SimpleNamespace(rpn_heads=heads), auxes, A)
    assert len(errs) == 2 * 2 * 2 and max(errs.values()) < 1e-6
    heads[1] = heads[1][::-1].copy()
    with pytest.raises(AssertionError, match="RPN head of image 0, P3"):
        PC.check_rpn_heads(types.SimpleNamespace(rpn_heads=heads), auxes, A)
