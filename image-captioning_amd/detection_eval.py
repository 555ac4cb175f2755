"""Average precision of one image's detections against its ground truth: the reference's utils.compute_ap (mask_rcnn/utils.py
:568-633), restated operation for operation, and the same rule on a given IoU matrix (box IoU or mask_rle.iou's mask IoU) for
several thresholds.  ops.detection_ap (dc_detection_ap_f64, include/dcap.h) is held to ap_from_overlaps bit for bit.

Two rules the reference's unstable np.argsort(...)[::-1] leaves open are fixed here:
  - equal scores are ordered higher index first, as np.argsort(kind="stable")[::-1] orders them (the rule of refine="device");
  - a prediction takes, among the still unmatched ground truths of its class with IoU >= threshold, the one of the highest IoU, and on
    equal IoU the higher index.  The reference walks the descending IoU order, skips matched ground truths, continues past a class
    mismatch and breaks below the threshold: without ties that is this argmax.
A NaN IoU is never eligible.  The final sum runs in a fixed order (ordered_sum), so host and device agree whatever NumPy does.
With no ground truth the AP is NaN (the reference divides by zero there; with no prediction either it returns 0, here NaN too).

Out of scope: COCO's 101-point interpolation, area ranges, maxDets and crowd regions as "ignore" in the matching."""
import numpy as np

from . import utils

DEFAULT_THRESHOLDS = np.arange(0.5, 1.0, 0.05)            # used as computed: 0.7000000000000002 and its like are not rounded
MAX_THRESHOLDS = 16


def ordered_sum(values):
    """The sum of float64 values in NumPy's order for fewer than 128 terms, at any length: below 8 terms a plain loop; otherwise eight
    running accumulators over the whole groups of 8, combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder in sequence."""
    v = [np.float64(x) for x in values]
    n = len(v)
    if n < 8:
        res = np.float64(0.0)
        for x in v:
            res = res + x
        return res
    r = v[:8]
    i = 8
    while i < n - n % 8:
        for k in range(8):
            r[k] = r[k] + v[i + k]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for x in v[i:]:
        res = res + x
    return res


def rank_order(pred_scores):
    """Prediction indices best first; equal scores: the higher index first."""
    return np.argsort(np.asarray(pred_scores), kind="stable")[::-1]


def precision_recall(matched, n_gt):
    """(precisions, recalls) as the reference pads them, from the 0/1 flags of the predictions in rank order: precisions float64 with
    the right-to-left maximum applied; recalls a float32 quotient, widened to float64 by the concatenation."""
    hits = np.cumsum(np.asarray(matched, np.float64))
    precisions = hits / (np.arange(len(hits)) + 1)
    with np.errstate(divide="ignore", invalid="ignore"):  # (no ground truth: the reference's division by zero)
        recalls = hits.astype(np.float32) / np.float32(n_gt)
    precisions = np.concatenate([[0], precisions, [0]])
    recalls = np.concatenate([[0], recalls, [1]])
    for i in range(len(precisions) - 2, -1, -1):
        precisions[i] = np.maximum(precisions[i], precisions[i + 1])
    return precisions, recalls


def average_precision(precisions, recalls):
    indices = np.where(recalls[:-1] != recalls[1:])[0] + 1
    return ordered_sum((recalls[indices] - recalls[indices - 1]) * precisions[indices])


def ap_from_overlaps(overlaps, gt_class_ids, pred_class_ids, pred_scores, iou_thresholds):
    """overlaps float64 [D,G] (row d: prediction d, in the caller's order) -> (ap float64 [T], pred_match int32 [T,D]: per prediction
    IN RANK ORDER the matched ground truth or -1, gt_match int32 [T,G]: the rank of the prediction matched to it or -1, order int64 [D]:
    the prediction at each rank)."""
    overlaps = np.asarray(overlaps, np.float64)
    if overlaps.ndim != 2:
        raise ValueError("ap_from_overlaps: overlaps must be [D,G], got shape %s" % (overlaps.shape,))
    D, G = overlaps.shape
    thresholds = np.asarray(iou_thresholds, np.float64).reshape(-1)
    gt_class_ids, pred_class_ids = np.asarray(gt_class_ids).reshape(-1)[:G], np.asarray(pred_class_ids).reshape(-1)
    pred_scores = np.asarray(pred_scores).reshape(-1)
    if len(gt_class_ids) != G or len(pred_class_ids) != D or len(pred_scores) != D:
        raise ValueError("ap_from_overlaps: %d x %d overlaps need %d predictions' ids and scores and %d ground-truth ids, got %d, %d and %d"
                         % (D, G, D, G, len(pred_class_ids), len(pred_scores), len(gt_class_ids)))
    order = rank_order(pred_scores)
    T = len(thresholds)
    ap = np.full(T, np.nan)
    pred_match, gt_match = np.full((T, D), -1, np.int32), np.full((T, G), -1, np.int32)
    same_class = pred_class_ids[:, None] == gt_class_ids[None, :]
    for t, thr in enumerate(thresholds):
        for rank, d in enumerate(order):
            row = overlaps[d]
            eligible = (gt_match[t] < 0) & (row >= thr) & same_class[d]        # (a NaN fails row >= thr)
            if eligible.any():
                best = np.flatnonzero(eligible & (row == row[eligible].max()))[-1]
                pred_match[t, rank], gt_match[t, best] = best, rank
        if G:
            ap[t] = average_precision(*precision_recall(pred_match[t] >= 0, G))
    return ap, pred_match, gt_match, order


def compute_ap(gt_boxes, gt_class_ids, pred_boxes, pred_class_ids, pred_scores, iou_threshold=0.5):
    """utils.compute_ap of the reference: (mAP, precisions, recalls, overlaps [predictions best first, gt])."""
    gt_boxes = utils.trim_zeros(np.asarray(gt_boxes))
    pred_boxes = utils.trim_zeros(np.asarray(pred_boxes))
    n = pred_boxes.shape[0]
    pred_scores, pred_class_ids = np.asarray(pred_scores)[:n], np.asarray(pred_class_ids)
    overlaps = utils.compute_overlaps(pred_boxes, gt_boxes)
    ap, pred_match, _, order = ap_from_overlaps(overlaps, np.asarray(gt_class_ids)[:gt_boxes.shape[0]], pred_class_ids[:n], pred_scores,
                                                [iou_threshold])
    precisions, recalls = precision_recall(pred_match[0] >= 0, gt_boxes.shape[0])
    return ap[0], precisions, recalls, overlaps[order]
