"""What Mask R-CNN inference costs on the device, and what the fused mask-head tail buys.

1. detect() per image at the reference's inference shape -- 1024 x 1024 molded image (a 768 x 1024 original), ResNet-101, 1000 proposals,
   81 classes, up to 100 detections, synthetic weights (mrcnn_class_logits spread so that foreground classes win; the count of
   detections that results is reported) -- with postprocess="host", "device" and "device" with device_masks=True (the masks stay on the device), alternating call by call: wall clock around each call
   (detect ends in device-to-host copies, so the call is complete when it returns), median of the calls of a repeat, median of the repeats.
2. The three kernels alone at that shape: ops.class_select (1000 x 81), ops.mask_head_tail (100 RoIs), ops.mask_paste (100 detections
   into 768 x 1024): device events around each launch, median per repeat, median of the repeats.
3. The fused tail against the same mathematics composed from what existed before it: ops.gemm to [N 196, 1024] with the bias in its
   epilogue, torch ReLU, ops.gemm of the [N 784, 256] view (a quadrant's channels are contiguous, so no shuffle is needed in front) to
   all classes (81 padded to 84 columns), torch sigmoid, gather of each RoI's class, pixel shuffle of the small result.  The two
   alternate call by call in one process.  fused_wins: composed - fused > the run-to-run spread of the composition's repeats.

4. --refine (alone: --refine --no-kernels --no-detect): what detect(refine="device") buys.  The host stage it replaces --
   mask_rcnn_model.refine_detections + unmold_boxes in NumPy on the model's own selection (1000 RoIs x 81 classes) -- wall clock, alone;
   the one launch that replaces it (ops.refine_detections on that selection), device events; and detect() with refine="host" and
   "device" alternating call by call in one process, for postprocess="device" with and without device_masks.  device_refine_wins:
   host - device > the run-to-run spread of the host mode's repeats.  There is no threshold: the mode is opt-in.

5. --rle (alone: --rle --no-kernels --no-detect): what detect(mask_format="rle") buys a caller who wants the masks on the host.  detect()
   with postprocess="device" and the dense [N,H,W] bytes copied down against mask_format="rle" (the encodings built on the device, two
   small copies), for refine="host" and "device", the four alternating call by call in one process; the bytes each mode copies; the
   run counts of the detections and ops.mask_rle's default capacity; and ops.mask_rle's seven launches beside ops.mask_paste's four on
   the model's own detections.  rle_wins: dense - rle > the run-to-run spread of the dense mode's repeats.

6. --eval (alone: --eval --no-kernels --no-detect): MaskRCNN.evaluate(overlap="mask") with backend="host" -- detect(mask_format="rle"),
   then mask_rle.iou and detection_eval.ap_from_overlaps in NumPy -- against backend="device" -- the encodings stay on the device,
   ops.rle_iou and ops.detection_ap score them, one small copy comes down --, alternating call by call in one process, against 20
   synthetic ground truths made from the image's own detections (shifted masks); and ops.rle_iou and ops.detection_ap alone on those
   encodings.  device_eval_wins: host - device > the run-to-run spread of the noisier mode's repeats.

    python tools/maskrcnn_bench.py --out profiles/maskrcnn_bench.json
    python tools/maskrcnn_bench.py --refine --no-kernels --no-detect --out profiles/maskrcnn_refine_bench.json
    python tools/maskrcnn_bench.py --rle --no-kernels --no-detect --out profiles/maskrcnn_rle_bench.json
    python tools/maskrcnn_bench.py --eval --no-kernels --no-detect --out profiles/maskrcnn_eval_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(rows, **row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def timed_alternating(call, launches, repeats, warmup):
    """{name: per-repeat medians (ms)}: device events around every call, the variants alternating call by call."""
    for _ in range(warmup):
        for k in call:
            call[k]()
    torch.cuda.synchronize()
    per_repeat = {k: [] for k in call}
    for _ in range(repeats):
        ev = {k: [] for k in call}
        for _ in range(launches):
            for k in call:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call[k]()
                e1.record()
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        for k in call:
            per_repeat[k].append(float(np.median([a.elapsed_time(b) for a, b in ev[k]])))
    return per_repeat


def summary(v):
    return dict(ms=round(float(np.median(v)), 4), repeats_ms=[round(x, 4) for x in v], spread_ms=round(max(v) - min(v), 4))


def kernels(own, rows):
    from image_captioning_amd import ops
    from image_captioning_amd.packing import pack_mask_tail
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    t = lambda a, dt=torch.float32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    R, C, N, P, Cc = own.proposals, own.classes, own.detections, 14, 256
    note = "device events around each call, median of %d calls per repeat, variants alternating call by call, median of %d repeats" % (own.launches, own.repeats)
    # ---- class_select
    z, d = t(rng.randn(R, C) * 3.0), t(rng.randn(R, 4 * C))
    ids, sc, dl = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, device=dev), torch.empty(R, 4, device=dev)
    r = timed_alternating({"class_select": lambda: ops.class_select(z, d, class_ids=ids, scores=sc, deltas_out=dl)}, own.launches, own.repeats, own.warmup)
    emit(rows, what="kernel", kernel="dc_class_select_f32", R=R, C=C, bytes=R * C * 4 + R * 24, timing=note, **summary(r["class_select"]))
    # ---- the tail, fused and composed
    x = t(np.maximum(rng.randn(N, P, P, Cc), 0.0))
    wd, bd = t(rng.randn(2, 2, Cc, Cc) / np.sqrt(Cc)), t(0.1 * rng.randn(Cc))
    wm, bm = (rng.randn(Cc, C) * 2.0 / np.sqrt(Cc)).astype(np.float32), (0.1 * rng.randn(C)).astype(np.float32)
    cls = t(rng.randint(1, C, N), torch.int32)
    wm_t, bm_d = t(pack_mask_tail(wm)), t(bm)
    out = torch.empty(N, 2 * P, 2 * P, device=dev)
    Cp = (C + 3) // 4 * 4
    wm_pad, bm_pad = np.zeros((Cc, Cp), np.float32), np.zeros(Cp, np.float32)
    wm_pad[:, :C], bm_pad[:C] = wm, bm
    wm_pad, bm_pad = t(wm_pad), t(bm_pad)
    wd_flat, bd4 = wd.view(4 * Cc, Cc), bd.repeat(4)
    g1, g2 = torch.empty(N * P * P, 4 * Cc, device=dev), torch.empty(N * P * P * 4, Cp, device=dev)
    index = cls.long().view(N, 1, 1).expand(N, P * P * 4, 1)

    def composed():
        ops.gemm(x.view(N * P * P, Cc), wd_flat, b_trans=True, shift=bd4, out=g1)
        torch.relu_(g1)
        ops.gemm(g1.view(N * P * P * 4, Cc), wm_pad, shift=bm_pad, out=g2)
        torch.sigmoid_(g2)
        picked = g2.view(N, P * P * 4, Cp).gather(2, index)                      # [N, (y, x, dy, dx), 1]
        return picked.view(N, P, P, 2, 2).permute(0, 1, 3, 2, 4).reshape(N, 2 * P, 2 * P)

    fused = lambda: ops.mask_head_tail(x, wd, bd, wm_t, bm_d, cls, out=out)
    diff = float((fused() - composed()).abs().max().item())
    r = timed_alternating({"fused": fused, "composed": composed}, own.launches, own.repeats, own.warmup)
    f, c = summary(r["fused"]), summary(r["composed"])
    flop = 2.0 * N * P * P * Cc * 4 * Cc
    wins = bool(c["ms"] - f["ms"] > c["spread_ms"])
    emit(rows, what="mask_tail", variant="fused", kernel="dc_mask_head_tail_f32", N=N, P=P, Cin=Cc, Cmid=Cc, C=C, gemm_flop=flop,
         tflops=round(flop / (f["ms"] * 1e-3) / 1e12, 2), max_abs_difference_to_composed=diff, fused_wins=wins, timing=note, **f)
    emit(rows, what="mask_tail", variant="composed", N=N, C=C, intermediate_bytes=int(g1.numel() * 4 + g2.numel() * 4), over_fused=round(c["ms"] / f["ms"], 2),
         timing=note, **c)
    # ---- mask_paste
    H, W = own.image
    hh, ww = rng.randint(20, H // 2, N), rng.randint(20, W // 2, N)
    y1, x1 = (rng.rand(N) * (H - hh)).astype(np.int64), (rng.rand(N) * (W - ww)).astype(np.int64)
    boxes = t(np.stack([y1, x1, y1 + hh, x1 + ww], axis=1), torch.int32)
    masks = torch.sigmoid(t(rng.randn(N, 2 * P, 2 * P) * 3.0))
    full = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
    r = timed_alternating({"mask_paste": lambda: ops.mask_paste(masks, boxes, H, W, out=full)}, max(own.launches // 4, 10), own.repeats, own.warmup)
    s = summary(r["mask_paste"])
    emit(rows, what="kernel", kernel="dc_mask_paste_u8", M=N, H=H, W=W, bytes_written=N * H * W, gbytes_per_s=round(N * H * W / (s["ms"] * 1e-3) / 1e9, 1),
         timing=note, **s)
    return wins


def build_model(own):
    """The model and the image of the detect legs (built once per process)."""
    from image_captioning_amd import synth
    from image_captioning_amd.mask_rcnn_model import MaskRCNN, MaskRCNNConfig
    S = own.side

    class Cfg(MaskRCNNConfig):
        IMAGES_PER_GPU = 1
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
        POST_NMS_ROIS_INFERENCE = own.proposals
        DETECTION_MAX_INSTANCES = own.detections
        DETECTION_MIN_CONFIDENCE = 0
    cfg = Cfg(own.classes)
    model = MaskRCNN("inference", cfg, "logs", stage4_blocks=own.stage4_blocks)
    W = model.get_weights_dict()
    scaled = {"rpn_conv_shared/kernel": 0.05, "rpn_bbox_pred/kernel": 0.3, "mrcnn_class_conv1/kernel": 0.05, "mrcnn_class_logits/kernel": 10.0,
              "mrcnn_bbox_fc/kernel": 0.3}
    model.set_weights({k: W[k] * np.float32(f) for k, f in scaled.items()})
    return model, synth.images(7, 1, own.image[0], own.image[1])[0]


def wall_alternating(model, img, modes, own, run=None):
    """{mode: per-repeat medians (ms)} of detect() -- or of run(**modes[k]) --: wall clock around each call, the modes alternating call by call."""
    run = run or (lambda **kw: model.detect([img], **kw))
    wall = {k: [] for k in modes}
    for _ in range(own.repeats):
        ts = {k: [] for k in modes}
        for _ in range(own.detect_calls):
            for k in ts:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(**modes[k])
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for k in ts:
            wall[k].append(float(np.median(ts[k])))
    return wall


def detect(own, rows, model, img):
    S = own.side
    modes = {"host": dict(postprocess="host"), "device": dict(postprocess="device"),
             "device_masks": dict(postprocess="device", device_masks=True)}      # the last leaves the [N,H,W] bytes on the device
    res = {}
    for post, kw in modes.items():
        for _ in range(own.detect_warmup):
            res[post] = model.detect([img], **kw)[0]
    same = bool(np.array_equal(res["host"]["masks"], res["device"]["masks"]) and np.array_equal(res["host"]["rois"], res["device"]["rois"]))
    wall = wall_alternating(model, img, modes, own)
    for post in wall:
        emit(rows, what="detect", postprocess=post, image=list(img.shape[:2]), molded=S, proposals=own.proposals, classes=own.classes,
             detections=int(len(res[post]["rois"])), mask_pixels=int(res[post]["masks"].sum()), same_results_both_modes=same,
             mask_bytes=int(len(res[post]["rois"]) * img.shape[0] * img.shape[1]),
             conv_math=model.conv_math_name, stage4_blocks=own.stage4_blocks,
             timing="wall clock around each detect() call (it returns host arrays), the modes alternating call by call, median of %d calls per "
                    "repeat, median of %d repeats" % (own.detect_calls, own.repeats), **summary(wall[post]))


def refine(own, rows, model, img):
    """Leg 4: the host stage alone, the launch alone, detect() with refine="host" and "device" alternating."""
    from image_captioning_amd import mask_rcnn_model as MR, ops
    cfg, dev = model.config, model.device
    base = model.detect([img])[0]
    rois, ids, scores, deltas = model.last_selection[0]
    window = model.mold_inputs([img])[2][0]

    def host_stage():
        boxes, cls, sc, _ = MR.refine_detections(rois, ids, scores, deltas, np.asarray(window, np.float32), cfg)
        return MR.unmold_boxes(boxes, img.shape, window)
    per = []
    for _ in range(own.repeats):
        ts = []
        for _ in range(own.detect_calls):
            t0 = time.perf_counter()
            host_stage()
            ts.append((time.perf_counter() - t0) * 1e3)
        per.append(float(np.median(ts)))
    emit(rows, what="refine_stage", where="host", stage="mask_rcnn_model.refine_detections + unmold_boxes (NumPy)", proposals=len(ids), classes=own.classes,
         candidates=int((ids > 0).sum()), detections=int(len(base["rois"])),
         timing="wall clock around each call on the host, median of %d calls per repeat, median of %d repeats" % (own.detect_calls, own.repeats), **summary(per))
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    args = (t(rois[None], torch.float32), t(ids[None], torch.int32), t(scores[None], torch.float32), t(deltas[None], torch.float32),
            t(MR.detection_constants(window, cfg, img.shape)[None], torch.float64), cfg.BBOX_STD_DEV, cfg.DETECTION_MIN_CONFIDENCE,
            cfg.DETECTION_NMS_THRESHOLD, cfg.DETECTION_MAX_INSTANCES, cfg.IMAGE_SHAPE[:2])
    r = timed_alternating({"refine": lambda: ops.refine_detections(*args)}, own.launches, own.repeats, own.warmup)
    emit(rows, what="refine_stage", where="device", kernel="dc_refine_detections_f32", proposals=len(ids), classes=own.classes,
         detections=int(ops.refine_detections(*args)[0].item()),
         timing="device events around each call (the wrapper allocates its seven outputs inside), median of %d calls per repeat, median of %d repeats"
                % (own.launches, own.repeats), **summary(r["refine"]))
    modes = {"%s/%s" % (rf, name): dict(refine=rf, **kw) for name, kw in (("device", dict(postprocess="device")),
                                                                          ("device_masks", dict(postprocess="device", device_masks=True)))
             for rf in ("host", "device")}
    res = {}
    for k, kw in modes.items():
        for _ in range(own.detect_warmup):
            res[k] = model.detect([img], **kw)[0]
    same = bool(all(np.array_equal(res["host/device"][key], res["device/device"][key]) for key in ("rois", "class_ids", "scores", "masks")))
    wall = wall_alternating(model, img, modes, own)
    for name in ("device", "device_masks"):
        h, d = summary(wall["host/" + name]), summary(wall["device/" + name])
        wins = bool(h["ms"] - d["ms"] > h["spread_ms"])
        for rf, s in (("host", h), ("device", d)):
            emit(rows, what="detect_refine", refine=rf, postprocess="device", device_masks=name == "device_masks", image=list(img.shape[:2]), molded=own.side,
                 proposals=own.proposals, classes=own.classes, detections=int(len(res["%s/%s" % (rf, name)]["rois"])),
                 mask_head_rows=int(cfg.DETECTION_MAX_INSTANCES if rf == "device" else len(res["%s/%s" % (rf, name)]["rois"])),
                 same_results_both_refines=same, device_refine_wins=wins, conv_math=model.conv_math_name, stage4_blocks=own.stage4_blocks,
                 timing="wall clock around each detect() call, the four modes alternating call by call, median of %d calls per repeat, median of %d "
                        "repeats" % (own.detect_calls, own.repeats), **s)


def rle(own, rows, model, img):
    """Leg 5: detect() with dense masks copied to the host against mask_format="rle", both with postprocess="device", for refine="host"
    and "device", the four modes alternating; then ops.mask_rle's launches beside ops.mask_paste's on the model's own detections."""
    from image_captioning_amd import mask_rle, ops
    H, W = img.shape[:2]
    modes = {"%s/%s" % (rf, fmt): dict(postprocess="device", refine=rf, mask_format=fmt) for rf in ("host", "device") for fmt in ("dense", "rle")}
    res = {}
    for k, kw in modes.items():
        for _ in range(own.detect_warmup):
            res[k] = model.detect([img], **kw)[0]
    same = {rf: bool(len(res[rf + "/rle"]["masks"]) == len(res[rf + "/dense"]["rois"]) and
                     all(np.array_equal(mask_rle.decode(r), res[rf + "/dense"]["masks"][:, :, i]) for i, r in enumerate(res[rf + "/rle"]["masks"])))
            for rf in ("host", "device")}
    wall = wall_alternating(model, img, modes, own)
    cfg = model.config
    for rf in ("host", "device"):
        dense, runs = summary(wall[rf + "/dense"]), summary(wall[rf + "/rle"])
        n = int(len(res[rf + "/dense"]["rois"]))
        rows_encoded = int(cfg.DETECTION_MAX_INSTANCES) if rf == "device" else n
        words = [int(len(r["counts"])) for r in res[rf + "/rle"]["masks"]]
        capacity = ops.mask_rle_capacity(rows_encoded, H, W)
        for fmt, s in (("dense", dense), ("rle", runs)):
            copied = n * H * W if fmt == "dense" else 4 * (rows_encoded + 1 + capacity)
            emit(rows, what="detect_rle", refine=rf, postprocess="device", mask_format=fmt, image=[int(H), int(W)], molded=own.side, proposals=own.proposals,
                 classes=own.classes, detections=n, mask_bytes_copied=int(copied), rle_decodes_to_the_dense_planes=same[rf],
                 rle_wins=bool(dense["ms"] - runs["ms"] > dense["spread_ms"]), conv_math=model.conv_math_name, stage4_blocks=own.stage4_blocks,
                 timing="wall clock around each detect() call, the four modes alternating call by call, median of %d calls per repeat, median of %d "
                        "repeats" % (own.detect_calls, own.repeats), **s)
        emit(rows, what="rle_run_counts", refine=rf, detections=n, rows_encoded=rows_encoded, words_of_the_detections=int(sum(words)),
             words_with_padded_rows=int(sum(words) + rows_encoded - n), most_words_one_detection=int(max(words) if words else 0),
             median_words_one_detection=float(np.median(words)) if words else 0.0, default_capacity_words=int(capacity),
             mask_pixels=int(sum(mask_rle.area(r) for r in res[rf + "/rle"]["masks"])))
    # the launches alone, on the class masks and boxes of a refine="device" call's detections
    model.detect([img], postprocess="device", refine="device", device_masks=True)
    n = len(model.last_detections[0]["rois"])
    masks = model.last_class_masks[0].clone()
    boxes = torch.tensor(model.last_detections[0]["rois"], dtype=torch.int32, device=model.device)
    full = torch.empty((n, H, W), dtype=torch.uint8, device=model.device)
    capacity = ops.mask_rle_capacity(n, H, W)
    first = ops.mask_rle(masks, boxes, H, W)
    need = int(first.offsets[-1].item())
    r = timed_alternating({"mask_paste": lambda: ops.mask_paste(masks, boxes, H, W, out=full), "mask_rle": lambda: ops.mask_rle(masks, boxes, H, W)},
                          max(own.launches // 4, 10), own.repeats, own.warmup)
    note = ("device events around each call (mask_rle allocates its pack inside), median of %d calls per repeat, the two alternating call by call, median of "
            "%d repeats" % (max(own.launches // 4, 10), own.repeats))
    emit(rows, what="kernel", kernel="dc_mask_paste_u8", M=n, H=int(H), W=int(W), bytes_written=int(n * H * W), timing=note, **summary(r["mask_paste"]))
    emit(rows, what="kernel", kernel="dc_mask_rle_u32", M=n, H=int(H), W=int(W), launches_per_call=7, words_needed=need, capacity_words=int(capacity),
         bytes_written=int(4 * (n + 1 + min(need, capacity))), timing=note, **summary(r["mask_rle"]))


def evaluation(own, rows, model, img):
    """Leg 6: evaluate(backend="host") against backend="device" on mask IoU, alternating; then ops.rle_iou and ops.detection_ap alone."""
    from image_captioning_amd import detection_eval, mask_rle, ops
    H, W = img.shape[:2]
    found = model.detect([img], postprocess="device", refine="device", mask_format="rle")[0]
    n = len(found["rois"])
    G = min(own.ground_truths, n)
    dense = np.stack([np.roll(mask_rle.decode(found["masks"][i]), (3 * (i % 3), -2 * (i % 4)), (0, 1)) for i in range(G)], 2) if G else np.zeros((H, W, 0), np.uint8)
    gt = {"class_ids": found["class_ids"][:G].copy(), "masks": dense}
    modes = {"host": dict(backend="host"), "device": dict(backend="device")}
    run = lambda **kw: model.evaluate([img], [gt], overlap="mask", **kw)
    res = {}
    for k, kw in modes.items():
        for _ in range(own.detect_warmup):
            res[k] = run(**kw)
    same = bool(res["host"]["AP"].tobytes() == res["device"]["AP"].tobytes() and
                all(np.array_equal(a, b) for key in ("pred_match", "gt_match", "order") for a, b in zip(res["host"][key], res["device"][key])))
    wall = wall_alternating(model, img, modes, own, run=run)
    h, d = summary(wall["host"]), summary(wall["device"])
    wins = bool(h["ms"] - d["ms"] > max(h["spread_ms"], d["spread_ms"]))
    for k, s in (("host", h), ("device", d)):
        emit(rows, what="evaluate", backend=k, overlap="mask", image=[int(H), int(W)], molded=own.side, proposals=own.proposals, classes=own.classes,
             detections=n, ground_truths=G, thresholds=len(detection_eval.DEFAULT_THRESHOLDS), mAP=[round(float(v), 6) for v in res[k]["mAP"]],
             same_results_both_backends=same, device_eval_wins=wins, second_mask_rle_launches=len(getattr(model, "last_eval_relaunched", [])),
             conv_math=model.conv_math_name, stage4_blocks=own.stage4_blocks,
             timing="wall clock around each evaluate() call, the two backends alternating call by call, median of %d calls per repeat, median of %d "
                    "repeats" % (own.detect_calls, own.repeats), **s)
    # the two scoring launches alone, on the packs of a refine="device" call's rows and of the ground truth
    M, dev = int(model.config.DETECTION_MAX_INSTANCES), model.device
    model.detect([img], postprocess="device", refine="device", device_masks=True)
    boxes = torch.zeros((M, 4), dtype=torch.int32, device=dev)
    boxes[:n] = torch.tensor(model.last_detections[0]["rois"], dtype=torch.int32, device=dev)
    masks = torch.zeros((M,) + tuple(model.last_class_masks[0].shape[1:]), dtype=torch.float32, device=dev)
    masks[:n] = model.last_class_masks[0]
    pack = ops.mask_rle(masks, boxes, H, W)
    rles = [mask_rle.encode(dense[:, :, g]) for g in range(G)]
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    offs_g = t(np.cumsum([0] + [len(r["counts"]) for r in rles]), torch.int32)
    counts_g = t(np.concatenate([r["counts"] for r in rles] or [np.zeros(0, np.uint32)]).astype(np.uint32).view(np.int32), torch.int32)
    n_det, n_gt = t([n], torch.int32), t([G], torch.int32)
    iou, _, _, status = ops.rle_iou(pack.offsets, pack.counts, offs_g, counts_g, H, W, n_det=n_det)
    cls = torch.full((1, M), -1, dtype=torch.int32, device=dev)
    cls[0, :n] = t(found["class_ids"], torch.int32)
    sc = torch.zeros((1, M), dtype=torch.float32, device=dev)
    sc[0, :n] = t(found["scores"], torch.float32)
    gt_cls, thr = t(gt["class_ids"][None], torch.int32), t(detection_eval.DEFAULT_THRESHOLDS, torch.float64)
    calls = {"rle_iou": lambda: ops.rle_iou(pack.offsets, pack.counts, offs_g, counts_g, H, W, n_det=n_det),
             "detection_ap": lambda: ops.detection_ap(iou[None], n_det, n_gt, cls, sc, gt_cls, thr)}
    r = timed_alternating(calls, own.launches, own.repeats, own.warmup)
    note = ("device events around each call (the wrappers allocate their outputs inside), the two alternating call by call, median of %d calls per repeat, "
            "median of %d repeats" % (own.launches, own.repeats))
    emit(rows, what="kernel", kernel="dc_rle_iou_f64", D=M, G=G, rows_computed=n, H=int(H), W=int(W), launches_per_call=3, status=status.cpu().numpy().tolist(),
         words_detections=int(pack.offsets[-1].item()), words_ground_truth=int(counts_g.numel()), timing=note, **summary(r["rle_iou"]))
    emit(rows, what="kernel", kernel="dc_detection_ap_f64", B=1, Dmax=M, Gmax=G, T=int(thr.numel()), timing=note, **summary(r["detection_ap"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--image", type=int, nargs=2, default=[768, 1024], help="the original image's height and width")
    ap.add_argument("--proposals", type=int, default=1000)
    ap.add_argument("--classes", type=int, default=81)
    ap.add_argument("--detections", type=int, default=100)
    ap.add_argument("--stage4-blocks", type=int, default=22)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--detect-calls", type=int, default=10)
    ap.add_argument("--detect-warmup", type=int, default=3)
    ap.add_argument("--no-detect", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--refine", action="store_true", help="leg 4: detect(refine='host') against refine='device'")
    ap.add_argument("--rle", action="store_true", help="leg 5: detect(mask_format='rle') against dense masks copied to the host")
    ap.add_argument("--eval", action="store_true", help="leg 6: evaluate(backend='host') against backend='device' on mask IoU")
    ap.add_argument("--ground-truths", type=int, default=20)
    ap.add_argument("--out", default=None)
    own = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    if not own.no_kernels:
        kernels(own, rows)
    model, img = build_model(own) if own.refine or own.rle or own.eval or not own.no_detect else (None, None)
    if not own.no_detect:
        detect(own, rows, model, img)
    if own.refine:
        refine(own, rows, model, img)
    if own.rle:
        rle(own, rows, model, img)
    if own.eval:
        evaluation(own, rows, model, img)
    if own.out:
        os.makedirs(os.path.dirname(own.out) or ".", exist_ok=True)
        with open(own.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
