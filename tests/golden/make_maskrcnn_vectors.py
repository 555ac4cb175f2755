"""Golden vectors for Mask R-CNN's host-side post-processing, produced by RUNNING THE REFERENCE'S OWN CODE (not a restatement).

As make_reference_vectors.py does: mask_rcnn/config.py is imported as a module (it only needs numpy), and the pure-NumPy functions
refine_detections and clip_to_window (mask_rcnn/mask_rcnn_model.py) and apply_box_deltas, non_max_suppression and compute_iou
(mask_rcnn/utils.py) are taken out of their files with `ast` at run time and compiled into a namespace that holds `np` -- the
modules' top-level `import tensorflow / keras / scipy.misc` lines are never executed, no stand-in for a missing library is written
and no reference source text is stored in this repository.  Of the METHOD unmold_detections only the statements in front of the mask
loop are compiled (the box part: count, scale and shift, truncation, the deletion of empty boxes); the loop behind them calls
scipy.misc.imresize, which no longer exists.

Inputs (seeded): 200 RoIs x 9 classes.  Planted: RoI 0 is a confident detection whose box loses its height in np.rint (zero area after
unmolding), RoI 1 is the only RoI class 8 wins, rows where the background wins, rows under DETECTION_MIN_CONFIDENCE.  The winners'
probabilities are checked to be pairwise distinct: the reference orders them with an unstable argsort.  Two runs: the reference's
DETECTION_MIN_CONFIDENCE (0.7) with room for 30 detections (the cut is active), and 0 with room for 100.

Run:  python tests/golden/make_maskrcnn_vectors.py        (needs the reference tree; the GPU box never runs this)
"""
import ast
import importlib.util
import os
import types

import numpy as np

REF = os.path.join(os.environ.get("DCAP_REFERENCE", "/root/reference"), "mask_rcnn")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "maskrcnn_reference.npz")
N_ROIS, N_CLASSES, SIDE = 200, 9, 256
WINDOW = (0, 32, 256, 224)                       # a portrait image padded left and right
IMAGE_SHAPE = (300, 225, 3)


def _definitions(path):
    with open(path, "r", encoding="utf-8") as f:
        tree = ast.parse(f.read(), filename=path)
    return {n.name: n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}


def functions_from(path, names, ns):
    """Compile the named function definitions of a reference file into `ns`, and nothing else."""
    defs = _definitions(path)
    for name in names:
        exec(compile(ast.Module(body=[defs[name]], type_ignores=[]), path, "exec"), ns)
    return types.SimpleNamespace(**{n: ns[n] for n in names})


def box_part_of_unmold_detections(path, ns):
    """unmold_detections' statements up to the mask loop as a function of their own, returning (boxes, class_ids, scores)."""
    fn = _definitions(path)["unmold_detections"]
    stop = min(st.lineno for st in fn.body if isinstance(st, ast.Assign) and getattr(st.targets[0], "id", None) == "full_masks")
    body = [st for st in fn.body if st.lineno < stop and not (isinstance(st, ast.Expr) and isinstance(st.value, ast.Constant))]
    body.append(ast.parse("return boxes, class_ids, scores").body[0])
    part = ast.FunctionDef(name="unmold_boxes_part", args=fn.args, body=body, decorator_list=[], returns=None, type_comment=None)
    mod = ast.fix_missing_locations(ast.Module(body=[part], type_ignores=[]))
    exec(compile(mod, path, "exec"), ns)
    return ns["unmold_boxes_part"]


def inputs(seed=20):
    rng = np.random.RandomState(seed)
    logits = rng.randn(N_ROIS, N_CLASSES) * 1.5
    logits[:, 8] -= 50.0                                                  # class 8 wins nowhere ...
    sharp = rng.rand(N_ROIS) < 0.6
    win = rng.randint(0, 8, N_ROIS)
    logits[np.flatnonzero(sharp), win[sharp]] += rng.uniform(3.0, 7.0, sharp.sum())
    logits[0] = -4.0
    logits[0, 3] = 3.0
    logits[1] = -4.0
    logits[1, 8] = 2.5                                                    # ... but in RoI 1
    z = logits - logits.max(axis=1, keepdims=True)
    probs = (np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)).astype(np.float32)
    cy, cx = rng.uniform(0.1, 0.9, N_ROIS), rng.uniform(0.2, 0.8, N_ROIS)
    hh, ww = rng.uniform(0.03, 0.5, N_ROIS), rng.uniform(0.03, 0.4, N_ROIS)
    rois = np.stack([cy - hh / 2, cx - ww / 2, cy + hh / 2, cx + ww / 2], axis=1).astype(np.float32)
    deltas = (rng.randn(N_ROIS, N_CLASSES, 4) * np.array([1.0, 1.0, 1.5, 1.5])).astype(np.float32)
    rois[0] = [0.5, 0.4, 0.5005, 0.6]                                     # 0.13 pixels high: np.rint closes it
    deltas[0] = 0.0
    rois[1] = [0.05, 0.3, 0.2, 0.5]
    deltas[1] = 0.0
    return rois, probs, deltas


def main():
    spec = importlib.util.spec_from_file_location("ref_maskrcnn_config", os.path.join(REF, "config.py"))
    ref_config = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_config)
    utils = functions_from(os.path.join(REF, "utils.py"), ["compute_iou", "non_max_suppression", "apply_box_deltas"], {"np": np})
    ns = {"np": np, "utils": utils}
    model_py = os.path.join(REF, "mask_rcnn_model.py")
    model = functions_from(model_py, ["clip_to_window", "refine_detections"], ns)
    unmold_boxes_part = box_part_of_unmold_detections(model_py, ns)

    rois, probs, deltas = inputs()
    ids = probs.argmax(axis=1)
    top = probs[np.arange(N_ROIS), ids]
    assert len(np.unique(top)) == N_ROIS, "two RoIs share a winning probability: the reference's argsort may order them either way"
    assert (ids == 8).sum() == 1 and ids[1] == 8 and (ids == 0).sum() >= 5 and ((ids > 0) & (top < 0.7)).sum() >= 5
    out = dict(rois=rois, probs=probs, deltas=deltas, window=np.array(WINDOW, np.float32), image_shape=np.array(IMAGE_SHAPE),
               num_classes=np.array(N_CLASSES), side=np.array(SIDE))
    for tag, conf, cap in (("conf", 0.7, 30), ("all", 0.0, 100)):
        class Cfg(ref_config.Config):
            NAME = "golden"
            NUM_CLASSES = N_CLASSES
            IMAGE_MIN_DIM = SIDE
            IMAGE_MAX_DIM = SIDE
            DETECTION_MAX_INSTANCES = cap
            DETECTION_MIN_CONFIDENCE = conf
        cfg = Cfg()
        det = model.refine_detections(rois.copy(), probs.copy(), deltas.copy(), np.array(WINDOW, np.float32), cfg)
        assert det.shape[1] == 6 and 0 < det.shape[0] <= cap
        det32 = np.zeros((cfg.DETECTION_MAX_INSTANCES, 6), np.float32)    # as the DetectionLayer hands them on: padded, float32
        det32[:det.shape[0]] = det
        dummy = np.zeros((cfg.DETECTION_MAX_INSTANCES, 1, 1, N_CLASSES), np.float32)
        boxes, class_ids, scores = unmold_boxes_part(None, det32, dummy, IMAGE_SHAPE, np.array(WINDOW))
        area = (det[:, 2] - det[:, 0]) * (det[:, 3] - det[:, 1])
        assert (area == 0).any() and len(boxes) < det.shape[0], "the planted zero-area detection did not survive to unmold_detections"
        assert (class_ids == 8).sum() == 1
        out.update({"det_" + tag: det, "final_boxes_" + tag: boxes, "final_ids_" + tag: class_ids, "final_scores_" + tag: scores,
                    "max_instances_" + tag: np.array(cfg.DETECTION_MAX_INSTANCES), "min_confidence_" + tag: np.array(conf),
                    "nms_threshold_" + tag: np.array(cfg.DETECTION_NMS_THRESHOLD), "bbox_std_" + tag: np.asarray(cfg.BBOX_STD_DEV)})
        print(tag, "detections", det.shape[0], "after unmolding", len(boxes), "classes", sorted(set(class_ids.tolist())))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
