"""Golden vectors for detection_eval.compute_ap, produced by RUNNING THE REFERENCE'S OWN compute_ap (not a restatement).

As make_maskrcnn_vectors.py does: compute_iou, compute_overlaps, trim_zeros and compute_ap are taken out of the reference's
mask_rcnn/utils.py with `ast` at run time and compiled into a namespace that holds numpy alone; no reference text is stored.  Seeded
inputs: D in {0, 1, 7, 8, 9, 100} predictions x G in {1, 5, 60} ground truths, int32 boxes with zero-padded rows behind both, class
mismatches planted, thresholds 0.5 and 0.75.  Before anything is written the scores are checked to be pairwise distinct and no
prediction to have two eligible ground truths of equal IoU: the reference's order is unspecified under ties.

Run:  python tests/golden/make_detection_ap_vectors.py        (needs the reference tree; the GPU box never runs this)
"""
import ast
import os
import types

import numpy as np

REF = os.path.join(os.environ.get("DCAP_REFERENCE", "/root/reference"), "mask_rcnn")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "detection_ap_reference.npz")
D_SIZES, G_SIZES, THRESHOLDS, PAD, N_CLASSES, SIDE = (0, 1, 7, 8, 9, 100), (1, 5, 60), (0.5, 0.75), 3, 4, 512


def functions_from(path, names, ns):
    """Compile the named function definitions of a reference file into `ns`, and nothing else."""
    with open(path, "r", encoding="utf-8") as f:
        tree = ast.parse(f.read(), filename=path)
    defs = {n.name: n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
    for name in names:
        exec(compile(ast.Module(body=[defs[name]], type_ignores=[]), path, "exec"), ns)
    return types.SimpleNamespace(**{n: ns[n] for n in names})


def make_case(rng, D, G):
    """G ground-truth boxes on a jittered grid; predictions are shifted copies of ground truths (so that IoUs fall on both sides of the
    thresholds) and a few boxes of their own; every fifth prediction carries another class than the box it was copied from."""
    side = int(np.ceil(np.sqrt(G)))
    cell = SIDE // side
    gy, gx = np.divmod(np.arange(G), side)
    h, w = rng.integers(cell // 2, cell, G), rng.integers(cell // 2, cell, G)
    y1, x1 = gy * cell + rng.integers(0, cell // 4, G), gx * cell + rng.integers(0, cell // 4, G)
    gt = np.stack([y1, x1, y1 + h, x1 + w], 1).astype(np.int32)
    gt_ids = rng.integers(1, N_CLASSES, G).astype(np.int32)
    src = rng.integers(0, G, D)
    shift = rng.integers(-cell // 6, cell // 6 + 1, (D, 4))
    pred = (gt[src] + shift).astype(np.int32)
    pred[:, 2:] = np.maximum(pred[:, 2:], pred[:, :2] + 1)
    ids = gt_ids[src].copy()
    ids[::5] = ids[::5] % (N_CLASSES - 1) + 1                                  # another class in 1..N_CLASSES-1
    scores = rng.permutation(D + 7)[:D].astype(np.float32) / np.float32(D + 7) + np.float32(0.01)
    pad = np.zeros((PAD, 4), np.int32)
    return (np.concatenate([gt, pad]), np.concatenate([gt_ids, np.zeros(PAD, np.int32)]), np.concatenate([pred, pad]),
            np.concatenate([ids, np.zeros(PAD, np.int32)]), np.concatenate([scores, np.zeros(PAD, np.float32)]))


def main():
    ref = functions_from(os.path.join(REF, "utils.py"), ["compute_iou", "compute_overlaps", "trim_zeros", "compute_ap"], {"np": np})
    rng = np.random.default_rng(20261021)
    out = {"d_sizes": np.array(D_SIZES), "g_sizes": np.array(G_SIZES), "thresholds": np.array(THRESHOLDS, np.float64)}
    for D in D_SIZES:
        for G in G_SIZES:
            gt, gt_ids, pred, ids, scores = make_case(rng, D, G)
            assert len(np.unique(scores[:D])) == D, "two predictions share a score: the reference's argsort may order them either way"
            key = "D%d_G%d_" % (D, G)
            out.update({key + "gt_boxes": gt, key + "gt_class_ids": gt_ids, key + "pred_boxes": pred, key + "pred_class_ids": ids,
                        key + "pred_scores": scores})
            matched = 0
            for t, thr in enumerate(THRESHOLDS):
                with np.errstate(divide="ignore", invalid="ignore"):
                    m_ap, precisions, recalls, overlaps = ref.compute_ap(gt, gt_ids, pred, ids, scores, iou_threshold=thr)
                for row in overlaps:
                    eligible = row[row >= thr]
                    assert len(np.unique(eligible)) == len(eligible), "a prediction has two eligible ground truths of equal IoU"
                matched += int(round(float(recalls[-2]) * G)) if D else 0
                out.update({key + "t%d_mAP" % t: np.float64(m_ap), key + "t%d_precisions" % t: precisions, key + "t%d_recalls" % t: recalls,
                            key + "t%d_overlaps" % t: overlaps})
            print("D %3d G %2d: mAP %.4f at %.2f, %d matches over both thresholds" % (D, G, out[key + "t0_mAP"], THRESHOLDS[0], matched))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
