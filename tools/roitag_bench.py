"""What the RoI tag head's fused loss launch buys, and what a tag train step costs beside the caption joint step.

1. dc_tag_focal_f32 (ops.tag_focal: sigmoid + focal loss + gradient, ONE launch) against the same mathematics written as torch
   elementwise ops with autograd on the device, at M = 200 and M = 1000 rows of C = 1000 classes (a third of the rows live, as the
   detection targets leave them).  Two torch forms: "torch_gather" selects the live rows first, as the reference's tf.gather_nd does
   (a data-dependent shape: torch reads the row count back, one host synchronisation per call), "torch_masked" keeps every row and
   multiplies the dead rows' losses by zero (no synchronisation; NaN-free inputs only).  The three alternate call by call in one
   process; device events around every call after a warm-up; a repeat's figure is the median of its calls; reported: the median of
   the repeats and their spread.  The path is launch-latency bound (about 2.4 MB at M = 200): the figure of merit is the time of the
   chain, not a bandwidth.  not_slower_than_torch: fused <= the faster torch form + the spread of the fused repeats.

2. --step: one EAGER ROITagRCNN train step (SGD(momentum=0.9, clipnorm=5.0), fp32) at the benchmark's joint shape -- 1024 x 1024, 2000
   proposals -> 200 RoIs, C = 1000 -- beside the caption joint model's eager step in the same arithmetic (compute_dtype f32, the default
   convolution arithmetic, Adam(amsgrad), step graphs off, no pipeline), for context: wall clock over --steps steps ending in a device
   synchronise, the two models alternating within a repeat.  No claim rests on it.

    python tools/roitag_bench.py --step --out profiles/roitag_bench.json
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

LO, HI = float(np.float32(1e-7)), float(np.float32(1.0 - 1e-7))


def emit(rows, **row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def torch_focal(z, t, alpha, gather):
    """focal_loss / roi_tag_classes_loss_graph (gamma = 2) as torch elementwise ops; returns d(loss)/dz through autograd."""
    z = z.detach().requires_grad_(True)
    live = (t == 1).any(dim=1)
    if gather:
        zz, tt = z[live], t[live].to(torch.float32)
    else:
        zz, tt = z, t.to(torch.float32)
    p = torch.sigmoid(zz)
    q = p.clamp(LO, HI)
    x = torch.log(q / (1.0 - q))
    bce = x.clamp(min=0.0) - x * tt + torch.log1p(torch.exp(-x.abs()))
    one = tt == 1
    fw = torch.where(one, 1.0 - p, p)
    a = torch.where(one, torch.full_like(p, alpha), torch.full_like(p, 1.0 - alpha))
    rows = (a * fw * fw * bce).sum(dim=1)
    loss = rows.sum() if gather else (rows * live.to(torch.float32)).sum()
    loss.backward()
    return loss.detach(), z.grad


def launches(own):
    from image_captioning_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    rows = []
    C = own.classes
    for M in own.rows:
        rng = np.random.RandomState(M)
        z = torch.tensor((rng.randn(M, C) * 3.0 - 2.0).astype(np.float32), device=dev)
        t_np = (rng.rand(M, C) < 0.003).astype(np.int32)
        t_np[::3, 0] = 1
        t_np[1::3] = 0
        t_np[2::3] = 0                                         # a third of the rows live
        t = torch.tensor(t_np, device=dev)
        loss_rows, dz = torch.empty((M,), device=dev), torch.empty((M, C), device=dev)
        call = {"fused": lambda: ops.tag_focal(z, t, 0.25, 2.0, 1.0, loss_rows=loss_rows, dlogits=dz),
                "torch_gather": lambda: torch_focal(z, t, 0.25, True),
                "torch_masked": lambda: torch_focal(z, t, 0.25, False)}
        call["fused"]()
        agree = {k: float((call[k]()[1] - dz).abs().max().item()) for k in ("torch_gather", "torch_masked")}
        loss_ref = float(call["torch_gather"]()[0].item())
        for _ in range(own.warmup):
            for k in call:
                call[k]()
        torch.cuda.synchronize()
        per_repeat = {k: [] for k in call}
        for _ in range(own.repeats):
            ev = {k: [] for k in call}
            for _ in range(own.launches):
                for k in call:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call[k]()
                    e1.record()
                    ev[k].append((e0, e1))
            torch.cuda.synchronize()
            for k in call:
                per_repeat[k].append(float(np.median([a.elapsed_time(b) for a, b in ev[k]])))
        ms = {k: float(np.median(v)) for k, v in per_repeat.items()}
        margin = max(per_repeat["fused"]) - min(per_repeat["fused"])
        best_torch = min(ms["torch_gather"], ms["torch_masked"])
        for k in call:
            emit(rows, what="tag_focal_call", variant=k, M=M, C=C, live_rows=int((t_np == 1).any(axis=1).sum()), ms=round(ms[k], 4),
                 repeats_ms=[round(v, 4) for v in per_repeat[k]], spread_ms=round(max(per_repeat[k]) - min(per_repeat[k]), 4),
                 over_fused=round(ms[k] / ms["fused"], 2), bytes_fused=M * C * 12 + M * 4,
                 max_abs_dz_difference_to_fused=agree.get(k, 0.0), loss=round(float(loss_rows.sum().item()) if k == "fused" else loss_ref, 4),
                 not_slower_than_torch=bool(ms["fused"] <= best_torch + margin) if k == "fused" else None,
                 timing="device events around each call, median of %d calls per repeat, variants alternating call by call, median of %d "
                        "repeats" % (own.launches, own.repeats))
    return rows


def steps(own, rest):
    sys.argv = [sys.argv[0], "--config", "joint", "--joint-dtype", "f32"] + rest
    import bench
    args = bench.parse()
    from image_captioning_amd.roi_tag_model import ROITagRCNN
    from image_captioning_amd.train_roi_tags import RoiTagConfig
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    _, cap, inputs, cap_cfg = bench.build_joint(args, dev)
    cap.use_step_graph = False
    C, S = own.classes, args.image_size

    class Cfg(RoiTagConfig):
        IMAGES_PER_GPU = args.joint_images_per_gpu
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
    cfg = Cfg(C)
    tag = ROITagRCNN("training", cfg, "logs", device=dev, stage4_blocks=args.stage4_blocks, seed=0)
    w = cap.get_weights_dict()                                  # the caption model's encoder, RPN and head: the same proposals and RoIs
    tag.set_weights({k: v for k, v in w.items() if not k.startswith("imgcap_")})
    tag.compile(cfg.LEARNING_RATE, cfg.LEARNING_MOMENTUM)
    rng = np.random.RandomState(5)
    gt_classes = np.zeros(inputs[4].shape[:2] + (C,), np.int32)
    for b in range(gt_classes.shape[0]):
        for g in np.flatnonzero(np.abs(inputs[5][b]).sum(axis=1) > 0):
            gt_classes[b, g, rng.choice(C, rng.randint(1, 4), replace=False)] = 1
    tag_inputs = list(inputs)
    tag_inputs[4] = gt_classes
    legs = {"caption_joint_eager": (cap, inputs), "roitag_eager": (tag, tag_inputs)}
    rows, wall, last = [], {k: [] for k in legs}, {}
    for k, (m, x) in legs.items():
        for _ in range(own.warmup):
            m.train_on_batch_device(x)
    torch.cuda.synchronize()
    for _ in range(own.step_repeats):
        for k, (m, x) in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(own.steps):
                out = m.train_on_batch_device(x)
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3 / own.steps)
            last[k] = m._loss_list(out)
    for k, (m, _) in legs.items():
        emit(rows, what="train_step_eager", model=k, image=S, train_rois=int(cfg.TRAIN_ROIS_PER_IMAGE), n_train=int(m.store.n_train),
             optimizer=type(m.optimizer).__name__, conv_math=m.conv_math_name, ms_per_step=round(float(np.median(wall[k])), 4),
             min_ms_per_step=round(min(wall[k]), 4), repeats_ms=[round(v, 4) for v in wall[k]], losses={n: round(float(v), 5) for n, v in last[k].items()},
             timing="wall clock per step over %d eager steps ending in a device synchronise after %d warm-up steps, the two models alternating "
                    "within a repeat, median / minimum of %d repeats" % (own.steps, own.warmup, own.step_repeats))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[200, 1000], help="M of the per-call timing")
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10, help="calls of each variant / steps of each model before the timed ones")
    ap.add_argument("--step", action="store_true", help="also time one eager train step of the tag model beside the caption joint model's")
    ap.add_argument("--steps", type=int, default=30, help="steps per timed window (--step)")
    ap.add_argument("--step-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    own, rest = ap.parse_known_args()
    rows = launches(own)
    if own.step:
        rows += steps(own, rest)
    if own.out:
        os.makedirs(os.path.dirname(own.out) or ".", exist_ok=True)
        with open(own.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
