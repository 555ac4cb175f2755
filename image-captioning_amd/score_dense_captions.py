"""The scoring half of the reference's evaluation script (evaluate_models/test_score_dense_captions.py :131-156, :347-384, :448-520):
ground truth, the text score of every record, and the DenseCap mAP sweep.  test_score_dense_captions.py holds the caption-generation
half and stops at assign_detections_to_ground_truth; DenseCaptioningEvaluator here extends that class, so one object does both:

    from image_captioning_amd.score_dense_captions import DenseCaptioningEvaluator

BLEU / ROUGE / CIDEr (pure Python in the reference) are scored by caption_metrics.py on token ids, on the host or on the device;
METEOR and SPICE (Java jars under eval/) are refused by name.
"""
import numpy as np

from . import caption_metrics as cm
from . import test_score_dense_captions as _generation

MIN_OVERLAPS = (0.3, 0.4, 0.5, 0.6, 0.7)                      # :71-72, the thresholds of the mAP sweep
MIN_SCORES = (-1, 0, 0.05, 0.1, 0.15, 0.2, 0.25)              # -1: the detection-only ("det") rows


class DenseCaptioningEvaluator(_generation.DenseCaptioningEvaluator):
    """The generation-side evaluator plus get_gt_captions, score_captions, evaluate and evaluate_from."""

    def __init__(self, *args, **kwargs):
        super(DenseCaptioningEvaluator, self).__init__(*args, **kwargs)
        self.min_overlaps = list(MIN_OVERLAPS)
        self.min_scores = list(MIN_SCORES)

    def get_gt_captions(self, image_ids):
        """:131-156 -- per image (image, merged ground-truth boxes, their caption lists): boxes overlapping by more than 0.7 are one box."""
        images, gt_boxes, gt_captions = [], [], []
        for image_id in image_ids:
            boxes, captions = self.dataset.load_original_captions_and_rois(image_id)
            merged_boxes, merged_captions = self.merge_boxes(boxes, captions, 0.7)
            images.append(self.dataset.load_image(image_id))
            gt_boxes.append(merged_boxes)
            gt_captions.append(merged_captions)
        return images, gt_boxes, gt_captions

    def score_captions(self, records, method, backend="host", tokenizer=None):
        """:347-384 on token ids (caption_metrics.py): the text score of every record of `records` (a list of per-image record lists, as
        assign_detections_to_ground_truth returns it), the records that have references forming ONE corpus (one group).  method "BLEU",
        "ROUGE" or "CIDER"; "METEOR" and "SPICE" raise (they need the reference's Java jars).  Returns float64 scores ALIGNED WITH THE
        FLATTENED RECORDS -- [n] for ROUGE / CIDER, [4, n] for BLEU-1..4 -- with NaN where a record has no references.  (The reference
        drops those records and later indexes the shorter list by record position; the two agree whenever the reference-less records
        come last -- INTEGRATION.md.)  backend="device" scores on the GPU and makes one device-to-host copy of the scores.  A reference
        is a string or, as merge_boxes leaves it, a sequence whose first entry is the string."""
        cm.check_metric(method)
        flat = [r for image in records for r in image]
        have = [i for i, r in enumerate(flat) if len(r['references']) > 0]
        gens = {i: [flat[i]['candidate']] for i in have}
        refs = {i: [s if isinstance(s, str) else s[0] for s in flat[i]['references']] for i in have}
        _, cands, rlists, _ = cm.encode_strings(gens, refs, tokenizer)
        res = cm.score(cm.pack_captions(cands, rlists), metrics=(method,), backend=backend)[method]
        res = res.cpu().numpy() if backend == "device" else res
        out = np.full(res.shape[:-1] + (len(flat),), np.nan)
        out[..., have] = res
        return out

    @staticmethod
    def evaluate_from(records, scores, npos, min_overlaps=MIN_OVERLAPS, min_scores=MIN_SCORES):
        """The sweep of :466-520 alone: records (per-image lists or one flat list, kept in that order -- image after image, not
        re-sorted globally), scores [n] aligned with the flattened records, npos the number of ground-truth boxes.  For every
        (min_overlap, min_score): a record is a true positive when it has references, ov >= min_overlap, ok == 1 and score > min_score,
        else a false positive; cumulative sums; the 101-point max-interpolated average precision.  min_score -1 fills 'det_breakdown'
        (keys 'ov<o>'), the others 'ap_breakdown' (keys 'ov<o>_score<s>'); 'map' and 'detmap' are their means.  float64 NumPy."""
        flat = [r for image in records for r in image] if len(records) and isinstance(records[0], (list, tuple)) else list(records)
        n = len(flat)
        scores = np.asarray(scores, np.float64).reshape(-1)
        assert scores.shape[0] == n, "evaluate_from: %d scores for %d records" % (scores.shape[0], n)
        has_ref = np.array([len(r['references']) > 0 for r in flat], bool)
        ov = np.array([r['ov'] for r in flat], np.float64)
        ok = np.array([r['ok'] == 1 for r in flat], bool)
        thresholds = np.array([t / 100 for t in range(0, 101)])
        ap_results, det_results = {}, {}
        for min_overlap in min_overlaps:
            for min_score in min_scores:
                with np.errstate(invalid="ignore"):
                    hit = has_ref & (ov >= min_overlap) & ok & (scores > min_score)
                tp = np.cumsum(hit.astype(np.float64))
                fp = np.cumsum((~hit).astype(np.float64))
                rec, prec = tp / npos, tp / (tp + fp)
                best_after = np.maximum.accumulate(prec[::-1])[::-1]              # max of prec[i:]: rec never decreases
                first = np.searchsorted(rec, thresholds, side="left")
                ap = 0
                for i in first:
                    ap = ap + (best_after[i] if i < n else 0)
                ap = ap / len(thresholds)
                if min_score == -1:
                    det_results['ov{}'.format(min_overlap)] = ap
                else:
                    ap_results['ov{}_score{}'.format(min_overlap, min_score)] = ap
        return {'map': np.mean(list(ap_results.values())), 'ap_breakdown': ap_results,
                'detmap': np.mean(list(det_results.values())), 'det_breakdown': det_results}

    def evaluate(self, method=None, backend="host"):
        """:448-520 -- {'map', 'ap_breakdown', 'detmap', 'det_breakdown'} of the dataset: ground truth, generated captions, the
        assignment, the text scores (method: default the evaluator's text_metrics; BLEU scores a record by its BLEU-4) and the sweep
        above.  The reference scores with METEOR, which needs its Java jar: "METEOR" and "SPICE" raise here."""
        method = cm.check_metric(method or self.text_metrics)
        num_images, image_ids = self.dataset.num_images, self.dataset._image_ids
        images, gt_boxes, gt_captions = self.get_gt_captions(image_ids)
        boxes, captions, log_probs = self.get_generated_captions(num_images, images)
        records = self.assign_detections_to_ground_truth(num_images, gt_boxes, gt_captions, boxes, captions, log_probs)
        scores = self.score_captions(records, method, backend=backend)
        npos = np.sum([box.shape[0] for box in gt_boxes])
        return self.evaluate_from(records, scores[3] if method == "BLEU" else scores, npos, self.min_overlaps, self.min_scores)
