"""detection_eval.compute_ap against the vectors the REFERENCE's own compute_ap produced (tests/golden/detection_ap_reference.npz, written
by tests/golden/make_detection_ap_vectors.py from the reference tree): mAP, precisions, recalls and overlaps bit for bit.  Then the rules
the reference leaves open or that its vectors cannot hold (its argsort is unstable under ties), on planted inputs: score ties, IoU
ties, an IoU exactly equal to the threshold, a best-IoU ground truth of the wrong class, no ground truth.  CPU only."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detection_ap_reference.npz")


@pytest.fixture(scope="module")
def vectors():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def ev():
    from image_captioning_amd import detection_eval
    return detection_eval


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def test_compute_ap_equals_the_reference_bit_for_bit(vectors, ev):
    v = vectors
    seen = 0
    for D in v["d_sizes"]:
        for G in v["g_sizes"]:
            key = "D%d_G%d_" % (D, G)
            args = [v[key + n] for n in ("gt_boxes", "gt_class_ids", "pred_boxes", "pred_class_ids", "pred_scores")]
            for t, thr in enumerate(v["thresholds"]):
                m_ap, precisions, recalls, overlaps = ev.compute_ap(*args, iou_threshold=float(thr))
                assert precisions.dtype == np.float64 and recalls.dtype == np.float64 and overlaps.dtype == np.float64
                assert overlaps.shape == (D, G) and precisions.shape == (D + 2,)
                assert np.array_equal(_bits(overlaps), _bits(v[key + "t%d_overlaps" % t])), (key, t)
                assert np.array_equal(_bits(precisions), _bits(v[key + "t%d_precisions" % t])), (key, t)
                assert np.array_equal(_bits(recalls), _bits(v[key + "t%d_recalls" % t])), (key, t)
                assert _bits(m_ap) == _bits(v[key + "t%d_mAP" % t]), (key, t, m_ap, v[key + "t%d_mAP" % t])
                seen += 1
    assert seen == 6 * 3 * 2


def test_the_vectors_hold_what_they_claim(vectors):
    v = vectors
    assert v["d_sizes"].tolist() == [0, 1, 7, 8, 9, 100] and v["g_sizes"].tolist() == [1, 5, 60] and v["thresholds"].tolist() == [0.5, 0.75]
    assert (v["D100_G60_gt_boxes"][-3:] == 0).all() and (v["D100_G60_pred_boxes"][-3:] == 0).all()       # the zero padding
    aps = [float(v["D%d_G%d_t%d_mAP" % (D, G, t)]) for D in (7, 8, 9, 100) for G in (5, 60) for t in (0, 1)]
    assert min(aps) < max(aps) and 0 < max(aps) <= 1                                                        # matches and misses both occur
    terms = v["D100_G60_t0_recalls"]
    assert (np.diff(terms) != 0).sum() >= 8                                                                 # the eight-accumulator branch of the sum
    assert float(v["D7_G5_t0_mAP"]) > float(v["D7_G5_t1_mAP"])                                              # the thresholds differ in effect
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_ordered_sum_is_numpy_s_order(ev):
    rng = np.random.default_rng(3)
    for n in (0, 1, 7, 8, 9, 15, 16, 17, 64, 100, 127):
        x = rng.random(n) * 10.0 ** rng.integers(-8, 8, n)
        assert _bits(ev.ordered_sum(x)) == _bits(np.sum(x)), n


def test_equal_scores_rank_the_higher_index_first(ev):
    # two predictions of equal score on one ground truth: the higher index is ranked first and takes it
    overlaps = np.array([[0.9], [0.8], [0.7]])
    ap, pred_match, gt_match, order = ev.ap_from_overlaps(overlaps, [1], [1, 1, 1], np.array([0.5, 0.5, 0.9], np.float32), [0.5])
    assert order.tolist() == [2, 1, 0] and pred_match.tolist() == [[0, -1, -1]] and gt_match.tolist() == [[0]] and ap[0] == 1.0
    ap, pred_match, _, order = ev.ap_from_overlaps(overlaps, [1], [1, 1, 1], np.array([0.5, 0.5, 0.1], np.float32), [0.75])
    assert order.tolist() == [1, 0, 2] and pred_match.tolist() == [[0, -1, -1]]
    assert np.array_equal(order, np.argsort(np.array([0.5, 0.5, 0.1], np.float32), kind="stable")[::-1])


def test_equal_ious_match_the_higher_index(ev):
    overlaps = np.array([[0.6, 0.6, 0.6], [0.6, 0.6, 0.6]])
    _, pred_match, gt_match, _ = ev.ap_from_overlaps(overlaps, [1, 1, 1], [1, 1], np.array([0.9, 0.8], np.float32), [0.5])
    assert pred_match.tolist() == [[2, 1]] and gt_match.tolist() == [[-1, 1, 0]]


def test_an_iou_equal_to_the_threshold_matches(ev):
    # areas chosen so that the IoU is exactly 1/2 and exactly 3/4
    gt = np.array([[0, 0, 4, 4], [10, 10, 14, 14]], np.int32)
    pred = np.array([[0, 0, 4, 2], [10, 10, 14, 13]], np.int32)               # 8 of 16 pixels; 12 of 16
    ids = np.array([1, 1], np.int32)
    scores = np.array([0.9, 0.8], np.float32)
    m_ap, _, _, overlaps = ev.compute_ap(gt, ids, pred, ids, scores, iou_threshold=0.5)
    assert overlaps[0, 0] == 0.5 and overlaps[1, 1] == 0.75 and m_ap == 1.0
    ap, pred_match, _, _ = ev.ap_from_overlaps(overlaps, ids, ids, scores, [0.5, 0.75, np.nextafter(0.75, 1.0)])
    assert pred_match.tolist() == [[0, 1], [-1, 1], [-1, -1]]
    assert ap.tolist() == [1.0, 0.25, 0.0]                                     # at 0.75: one of two found, at rank 2: (1/2) * (1/2)


def test_a_best_iou_of_the_wrong_class_lets_the_second_best_match(ev):
    overlaps = np.array([[0.9, 0.6, 0.2]])
    _, pred_match, gt_match, _ = ev.ap_from_overlaps(overlaps, [2, 1, 1], [1], np.array([0.9], np.float32), [0.5, 0.7])
    assert pred_match.tolist() == [[1], [-1]] and gt_match.tolist() == [[-1, 0, -1], [-1, -1, -1]]


def test_a_matched_ground_truth_is_skipped_and_a_nan_is_never_eligible(ev):
    overlaps = np.array([[0.9, 0.6], [0.8, 0.7], [np.nan, np.nan]])
    ap, pred_match, _, _ = ev.ap_from_overlaps(overlaps, [1, 1, 1][:2], [1, 1, 1], np.array([0.9, 0.8, 0.99], np.float32), [0.5])
    assert pred_match.tolist() == [[-1, 0, 1]]                                 # rank 0 is the NaN row
    assert ap[0] == (0.5 - 0.0) * (2 / 3) + (1.0 - 0.5) * (2 / 3)


def test_no_ground_truth_gives_nan(ev):
    ap, pred_match, gt_match, order = ev.ap_from_overlaps(np.zeros((3, 0)), [], [1, 1, 1], np.array([0.3, 0.2, 0.1], np.float32), [0.5, 0.75])
    assert np.isnan(ap).all() and pred_match.tolist() == [[-1, -1, -1]] * 2 and gt_match.shape == (2, 0) and order.tolist() == [0, 1, 2]
    ap, _, _, _ = ev.ap_from_overlaps(np.zeros((0, 0)), [], [], np.zeros(0, np.float32), [0.5])
    assert np.isnan(ap).all()                                                  # (the reference returns 0 there)
    ap, pred_match, _, _ = ev.ap_from_overlaps(np.zeros((0, 2)), [1, 1], [], np.zeros(0, np.float32), [0.5])
    assert ap.tolist() == [0.0] and pred_match.shape == (1, 0)
    m_ap, precisions, recalls, overlaps = ev.compute_ap(np.zeros((2, 4), np.int32), np.zeros(2, np.int32), np.array([[0, 0, 4, 4]], np.int32),
                                                        np.array([1], np.int32), np.array([0.5], np.float32))
    assert np.isnan(m_ap) and overlaps.shape == (1, 0)


def test_default_thresholds_are_used_as_computed(ev):
    assert np.array_equal(ev.DEFAULT_THRESHOLDS, np.arange(0.5, 1.0, 0.05)) and len(ev.DEFAULT_THRESHOLDS) == 10
    assert ev.DEFAULT_THRESHOLDS[4] != 0.7                                      # 0.7000000000000002: not rounded


def test_the_shapes_are_checked(ev):
    with pytest.raises(ValueError, match="overlaps"):
        ev.ap_from_overlaps(np.zeros(3), [1], [1], [0.5], [0.5])
    with pytest.raises(ValueError, match="predictions"):
        ev.ap_from_overlaps(np.zeros((2, 1)), [1], [1], np.array([0.5], np.float32), [0.5])
