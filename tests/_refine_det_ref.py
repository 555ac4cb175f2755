"""A NumPy restatement of dc_refine_detections_f32's contract (include/dcap.h), the case table the CPU and GPU tests share, and
`decided`: whether a case's result survives a float64 exp that is one ulp off either way.

The restatement is written from the contract, not from mask_rcnn_model.refine_detections: one global greedy scan in
np.argsort(kind="stable")[::-1] order with suppression inside a class only, every operation in the number format the contract names,
the exp function handed in.  tests/test_refine_det_ref.py holds it equal to the host path (refine_detections + unmold_boxes) wherever
the scores are pairwise distinct -- with ties the host path's default sort promises no order and the contract's rule stands alone.
`plant` names one deliberate error; the CPU test shows that each moves the result on the table.

A plain module, no fixtures; the package is imported inside the functions, as in the test files."""
import numpy as np

F32, F64, I32 = np.float32, np.float64, np.int32
STD = (0.1, 0.1, 0.2, 0.2)
PLANTS = ("cross_class", "ge", "f64_iou", "no_conf", "low_index_first")
OUTPUTS = ("count", "boxes", "rois", "norm", "class_ids", "scores", "keep")


def refined_boxes(rois, deltas, window, std, hw, exp):
    """apply_box_deltas, the scaling to pixels, the clip and np.rint: rois, deltas float32 [N,4] -> int32 [N,4]."""
    r = np.asarray(rois, F32)
    d = np.asarray(deltas, F32).astype(F64) * np.asarray(std, F64)
    with np.errstate(all="ignore"):
        height, width = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
        cy, cx = r[:, 0] + F32(0.5) * height, r[:, 1] + F32(0.5) * width
        cy = (cy.astype(F64) + d[:, 0] * height.astype(F64)).astype(F32)
        cx = (cx.astype(F64) + d[:, 1] * width.astype(F64)).astype(F32)
        height = (height.astype(F64) * exp(d[:, 2])).astype(F32)
        width = (width.astype(F64) * exp(d[:, 3])).astype(F32)
        y1, x1 = cy - F32(0.5) * height, cx - F32(0.5) * width
        box = np.stack([y1, x1, y1 + height, x1 + width], axis=1)
        box = (box.astype(F64) * np.array([hw[0], hw[1], hw[0], hw[1]], F64)).astype(F32)
        w = np.asarray(window, F64).astype(F32)
        for col, lo, hi in ((0, 0, 2), (1, 1, 3), (2, 0, 2), (3, 1, 3)):
            box[:, col] = np.maximum(np.minimum(box[:, col], w[hi]), w[lo])
        return np.rint(box).astype(I32)


def exceeds(box, boxes, thr, plant=None):
    """The float32 IoU of one int32 box with others (taken as float32) against (float) thr; a 0/0 NaN exceeds nothing."""
    T = F64 if plant == "f64_iou" else F32
    a, b = box.astype(T), boxes.astype(T)
    with np.errstate(all="ignore"):
        area_a, area_b = (a[2] - a[0]) * (a[3] - a[1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        ih = np.maximum(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]), T(0))
        iw = np.maximum(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), T(0))
        inter = iw * ih
        iou = inter / (area_a + area_b - inter)
        t = T(thr) if plant == "f64_iou" else F32(thr)
        return iou >= t if plant == "ge" else iou > t


def refine_image(rois, class_ids, scores, deltas, consts, std, min_confidence, threshold, max_instances, hw, exp=np.exp, plant=None):
    """One image -> the seven outputs as a dict (OUTPUTS), max_instances rows each, padded as the contract pads them."""
    ids, sc, M = np.asarray(class_ids, I32), np.asarray(scores, F32), int(max_instances)
    consts = np.asarray(consts, F64)
    boxes = refined_boxes(rois, deltas, consts[:4], std, hw, exp)
    cand = ids > 0
    if min_confidence != 0 and plant != "no_conf":
        cand &= sc >= F32(min_confidence)
    idx = np.nonzero(cand)[0]
    if plant == "low_index_first":
        order = idx[np.argsort(-sc[idx].astype(F64), kind="stable")]
    else:
        order = idx[np.argsort(sc[idx], kind="stable")[::-1]]
    alive, kept = np.ones(len(order), bool), []
    for a, i in enumerate(order):
        if not alive[a]:
            continue
        kept.append(i)
        if len(kept) == M:
            break
        rest = order[a + 1:]
        hit = exceeds(boxes[i], boxes[rest], threshold, plant)
        if plant != "cross_class":
            hit &= ids[rest] == ids[i]
        alive[a + 1:] &= ~hit
    kept = np.array(kept, np.int64)
    shift = np.array([consts[6], consts[7], consts[6], consts[7]], F64)
    final = ((boxes[kept].astype(F64) - shift) * consts[8]).astype(I32)
    ok = (final[:, 2] - final[:, 0]) * (final[:, 3] - final[:, 1]) > 0
    kept, final = kept[ok], final[ok]
    n = len(kept)
    out = dict(count=np.array(n, I32), boxes=np.zeros((M, 4), I32), rois=np.zeros((M, 4), I32), norm=np.zeros((M, 4), F32),
               class_ids=np.full((M,), -1, I32), scores=np.zeros((M,), F32), keep=np.full((M,), -1, I32))
    out["boxes"][:n], out["rois"][:n], out["class_ids"][:n], out["scores"][:n], out["keep"][:n] = boxes[kept], final, ids[kept], sc[kept], kept
    out["norm"][:n] = (boxes[kept].astype(F32).astype(F64) / np.array([hw[0], hw[1], hw[0], hw[1]], F64)).astype(F32)
    return out


def refine(case, exp=np.exp, plant=None):
    """A case of B images -> the seven outputs stacked over the images ([B], [B,M,4], ...)."""
    per = [refine_image(case["rois"][b], case["class_ids"][b], case["scores"][b], case["deltas"][b], case["consts"][b], case["std"],
                        case["min_confidence"], case["threshold"], case["max_instances"], case["hw"], exp=exp, plant=plant)
           for b in range(len(case["rois"]))]
    return {k: np.stack([p[k] for p in per]) for k in OUTPUTS}


def same(a, b):
    """All seven outputs equal, tails included (scores by their bits)."""
    return all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k].view(I32) if a[k].dtype == F32 else a[k],
                                                                                        b[k].view(I32) if b[k].dtype == F32 else b[k])
               for k in OUTPUTS)


def decided(case):
    """True when the result does not hang on the last bit of exp: np.exp, one ulp above and one ulp below give the same outputs."""
    up = lambda x: np.nextafter(np.exp(x), np.inf)
    down = lambda x: np.nextafter(np.exp(x), -np.inf)
    base = refine(case)
    return same(base, refine(case, exp=up)) and same(base, refine(case, exp=down))


def host_path(case):
    """mask_rcnn_model.refine_detections + unmold_boxes on every image of the case, padded into the seven outputs."""
    from image_captioning_amd import mask_rcnn_model as MR

    class Cfg(object):
        BBOX_STD_DEV = np.array(case["std"])
        IMAGE_SHAPE = np.array([case["hw"][0], case["hw"][1], 3])
        DETECTION_MIN_CONFIDENCE = case["min_confidence"]
        DETECTION_NMS_THRESHOLD = case["threshold"]
        DETECTION_MAX_INSTANCES = case["max_instances"]
    M, hw, per = case["max_instances"], case["hw"], []
    for b in range(len(case["rois"])):
        window = case["windows"][b]
        boxes, cls, sc, keep = MR.refine_detections(case["rois"][b], case["class_ids"][b], case["scores"][b], case["deltas"][b],
                                                    np.asarray(window, F32), Cfg)
        final, ok = MR.unmold_boxes(boxes, case["image_shapes"][b], window)
        n = int(ok.sum())
        out = dict(count=np.array(n, I32), boxes=np.zeros((M, 4), I32), rois=np.zeros((M, 4), I32), norm=np.zeros((M, 4), F32),
                   class_ids=np.full((M,), -1, I32), scores=np.zeros((M,), F32), keep=np.full((M,), -1, I32))
        out["boxes"][:n], out["rois"][:n], out["class_ids"][:n], out["scores"][:n], out["keep"][:n] = boxes[ok], final[ok], cls[ok], sc[ok], keep[ok]
        out["norm"][:n] = (boxes[ok].astype(F32) / np.array([hw[0], hw[1], hw[0], hw[1]])).astype(F32)
        per.append(out)
    return {k: np.stack([p[k] for p in per]) for k in OUTPUTS}


def distinct_scores(case):
    """Pairwise distinct scores among each image's candidates-to-be (class id > 0): the host path's order is then defined."""
    return all(len(np.unique(s[i > 0])) == int((i > 0).sum()) for s, i in zip(case["scores"], case["class_ids"]))


# ------------------------------------------------------------------------------------------------ cases
def consts_row(window, hw, image_shape):
    """dense_model.refine_constants' row, computed here from its description (window, h, w, shift y x, scale, one unused word)."""
    scale = min(image_shape[0] / (window[2] - window[0]), image_shape[1] / (window[3] - window[1]))
    return np.array([window[0], window[1], window[2], window[3], hw[0], hw[1], window[0], window[1], scale, 0.0], F64)


def make_case(name, seed, N, C, B=1, min_confidence=0.0, max_instances=100, hw=(256, 256), geometry=None, classes=None, ties=0,
              clusters=None, tiny=0, outside=0, inverted=0, zero_padded=0, edit=None):
    """Random RoIs around a few centres (so that the NMS bites), deltas of the head's size, distinct scores (a permutation of a grid,
    ties > 0: quantised to that many values), class ids uniform in [0, C) (classes: that list instead).  geometry: per image
    (window, image_shape); the last rows become, in turn, tiny boxes, boxes outside the window, boxes with negative extent and all-zero
    proposals.  edit(case) may adjust the arrays."""
    rng = np.random.RandomState(seed)
    geometry = geometry or [((0, 32, 256, 224), (300, 225, 3))] * B
    rois, ids, scores, deltas = [], [], [], []
    for b in range(B):
        k = clusters or max(1, min(N, 2 + N // 12))
        centre = rng.uniform(0.15, 0.85, (k, 2))[rng.randint(0, k, N)] + rng.normal(0, 0.02, (N, 2))
        size = rng.uniform(0.05, 0.35, (N, 2))
        r = np.concatenate([centre - size / 2, centre + size / 2], axis=1)
        at = N
        for count, kind in ((zero_padded, "zero"), (inverted, "inverted"), (outside, "outside"), (tiny, "tiny")):
            lo = max(0, at - count)
            if kind == "zero":
                r[lo:at] = 0
            elif kind == "inverted":
                r[lo:at] = r[lo:at][:, [2, 3, 0, 1]]
            elif kind == "outside":
                r[lo:at, 1], r[lo:at, 3] = rng.uniform(0.0, 0.05, at - lo), rng.uniform(0.06, 0.11, at - lo)    # left of the window's x1
            else:
                r[lo:at, 2:] = r[lo:at, :2] + rng.uniform(0.001, 0.012, (at - lo, 2))
            at = lo
        rois.append(r.astype(F32))
        ids.append((rng.randint(0, C, N) if classes is None else np.asarray(classes)[rng.randint(0, len(classes), N)]).astype(I32))
        s = (rng.permutation(N) + 1.0) / (N + 1.0)
        if ties:
            s = np.floor(s * ties) / ties
        scores.append(s.astype(F32))
        deltas.append((rng.normal(0, 1.0, (N, 4)) * [1.0, 1.0, 1.5, 1.5]).astype(F32))
    case = dict(name=name, rois=np.stack(rois), class_ids=np.stack(ids), scores=np.stack(scores), deltas=np.stack(deltas), std=STD,
                min_confidence=min_confidence, threshold=0.3, max_instances=max_instances, hw=hw, windows=[g[0] for g in geometry],
                image_shapes=[g[1] for g in geometry], consts=np.stack([consts_row(g[0], hw, g[1]) for g in geometry]))
    if edit:
        edit(case)
    return case


def _twins(case):
    """Rows 0-3: one box four times -- classes 1 and 2 once each with the best scores, then class 1 twice more: the two leaders must
    both survive (different classes), the other two fall to the first."""
    for a in ("rois", "deltas"):
        case[a][0, 1:4] = case[a][0, 0]
    case["rois"][0, 0:4] = np.array([0.3, 0.3, 0.6, 0.6], F32)
    case["deltas"][0, 0:4] = 0
    case["class_ids"][0, :4] = [1, 2, 1, 1]
    case["scores"][0, :4] = np.array([0.999, 0.998, 0.997, 0.996], F32)


def _at_the_floor(case):
    """Scores exactly at (float32) 0.7 -- kept, NumPy compares in float32 -- and one float32 below it -- dropped; the two rows have
    class 80 to themselves and distant boxes, so that only the floor decides about them."""
    case["scores"][0, 0], case["scores"][0, 1] = F32(0.7), np.nextafter(F32(0.7), F32(0))
    case["class_ids"][0][case["class_ids"][0] == 80] = 79
    case["class_ids"][0, :2] = 80
    case["rois"][0, 0], case["rois"][0, 1] = np.array([0.2, 0.2, 0.4, 0.4], F32), np.array([0.6, 0.6, 0.8, 0.8], F32)
    case["deltas"][0, :2] = 0


def _iou_between_the_thresholds(case):
    """Two boxes of one class in a 4096-pixel image, the second inside the first: 947 x 1238 in 2001 x 1953 is an IoU of 0.3 + 1 / (10 x
    3907953) -- above the float64 0.3, and rounded to float32 exactly (float) 0.3, which exceeds nothing: both survive.  Zero deltas and
    coordinates that are multiples of 1/4096 keep every step of the refinement exact."""
    case["rois"][0] = np.array([[0, 0, 2001, 1953], [0, 0, 947, 1238]], F32) / F32(4096)
    case["deltas"][0] = 0
    case["class_ids"][0] = 1
    case["scores"][0] = np.array([0.9, 0.8], F32)


BIG = [((0, 0, 4096, 4096), (4096, 4096, 3))]
THREE = [((0, 32, 256, 224), (300, 225, 3)), ((0, 0, 256, 256), (512, 512, 3)), ((43, 0, 213, 256), (100, 150, 3))]
LIMIT = 2048          # _lib.REFINE_DET_MAX_ROIS (the GPU test holds the two equal)
_CASES = []


def cases():
    """The table, built once: name -> case.  Sizes 1, 63, 64, 65, 1000, 1025 and the limit; B = 1 and 3; C = 2 and 81."""
    if not _CASES:
        _CASES.extend([
            make_case("n1", 1, 1, 2, classes=[1], max_instances=3),
            make_case("n2-iou-between-thresholds", 14, 2, 2, hw=(4096, 4096), geometry=BIG, edit=_iou_between_the_thresholds),
            make_case("n63-m3-more-survivors", 2, 63, 81, max_instances=3),
            make_case("n64-single-class", 3, 64, 2, classes=[1]),
            make_case("n65-all-background", 4, 65, 81, classes=[0]),
            make_case("n65-ties", 5, 65, 2, ties=4, clusters=3),
            make_case("n64-twins", 6, 64, 81, edit=_twins),
            make_case("n65-floor-0.7", 7, 65, 81, min_confidence=0.7, edit=_at_the_floor),
            make_case("n200-edges-b3", 8, 200, 9, B=3, geometry=THREE, tiny=30, outside=20, inverted=20, zero_padded=30, max_instances=100),
            make_case("n1000-b3-conf", 9, 1000, 81, B=3, geometry=THREE, min_confidence=0.7),
            make_case("n1000-c81", 10, 1000, 81, zero_padded=100),
            make_case("n1025-c81", 11, 1025, 81),
            make_case("limit-c2", 12, LIMIT, 2, clusters=40, max_instances=100),
            make_case("limit-ties-c81", 13, LIMIT, 81, ties=64),
        ])
    return {c["name"]: c for c in _CASES}


def golden_case(golden, tag):
    """tests/golden/maskrcnn_reference.npz (the reference's own refine_detections / unmold_detections) -> (case, expected detections
    [K,6] float64 as the DetectionLayer pads them: y1, x1, y2, x2, class id, score; final boxes, ids, scores)."""
    probs, deltas = golden["probs"], golden["deltas"]
    ids = probs.argmax(axis=1).astype(I32)
    n = np.arange(len(ids))
    side = int(golden["side"])
    window, shape = tuple(float(v) for v in golden["window"]), tuple(int(v) for v in golden["image_shape"])
    case = dict(name="golden-" + tag, rois=golden["rois"][None].astype(F32), class_ids=ids[None], scores=probs[n, ids][None].astype(F32),
                deltas=deltas[n, ids][None].astype(F32), std=tuple(float(v) for v in golden["bbox_std_" + tag]),
                min_confidence=float(golden["min_confidence_" + tag]), threshold=float(golden["nms_threshold_" + tag]),
                max_instances=int(golden["max_instances_" + tag]), hw=(side, side), windows=[window], image_shapes=[shape],
                consts=consts_row(window, (side, side), shape)[None])
    return case, golden["det_" + tag], golden["final_boxes_" + tag], golden["final_ids_" + tag], golden["final_scores_" + tag]
