"""What rpn_targets="device" buys: the joint model's RPN training targets built by dense_model.build_rpn_targets on the host (NumPy,
float64, on the thread that drives the step) and by ops.rpn_targets on the device, at the configs[4] shape (1024 x 1024, 261 888 anchors,
budget 256) for G = 10 / 50 / 100 ground-truth boxes.

Per G: the host function alone (wall clock on this machine's CPU), ops.rpn_targets alone (device events), then the pipelined joint step
(pipeline.JointTrainPipeline, what train() runs) fed precomputed host arrays -- the path the benchmark times, the yardstick -- and fed
device-mode batches (the boxes travel, the targets are built in front of the encoder pass): the two legs alternate call by call in one
process, a call being --steps steps plus the flush, medians of --repeats (at least 5) with the max - min spread.  Last, a train()-style
loop over a synthetic in-memory dataset in both generator modes: steps per second with the generator on the stepping thread.

    python tools/rpn_targets_bench.py --out profiles/rpn_targets_bench.json
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402
from decode_bench import timed  # noqa: E402


def boxes_for(seed, n, side):
    r = np.random.RandomState(seed)
    y, x = r.randint(0, side - 64, n), r.randint(0, side - 64, n)
    h, w = r.randint(32, side // 2, n), r.randint(32, side // 2, n)
    return np.stack([y, x, np.minimum(y + h, side), np.minimum(x + w, side)], axis=1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed call of a step leg")
    ap.add_argument("--loop-steps", type=int, default=6, help="steps of the train()-style loop per generator mode")
    ap.add_argument("--boxes", type=int, nargs="+", default=[10, 50, 100])
    ap.add_argument("--out", default=None)
    own, rest = ap.parse_known_args()
    sys.argv = [sys.argv[0], "--config", "joint"] + rest
    args = bench.parse()
    from image_captioning_amd import ops, utils
    from image_captioning_amd.dense_model import build_rpn_targets, data_generator
    from image_captioning_amd.pipeline import JointTrainPipeline
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    reps, warm = max(own.repeats, 5), max(own.warmup, 2)
    model, inner, inputs, cfg = bench.build_joint(args, dev)
    S, n = args.image_size, int(cfg.RPN_TRAIN_ANCHORS_PER_IMAGE)
    anchors = utils.generate_pyramid_anchors(cfg.RPN_ANCHOR_SCALES, cfg.RPN_ANCHOR_RATIOS, cfg.BACKBONE_SHAPES, cfg.BACKBONE_STRIDES, 1)
    sizes = [int(h * w * len(cfg.RPN_ANCHOR_RATIOS)) for h, w in cfg.BACKBONE_SHAPES]
    adev = torch.tensor(anchors, dtype=torch.float64, device=dev)
    for _ in range(8):
        inner.train_on_batch(inputs)
    pipe = JointTrainPipeline(inner)
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def piped(batch):
        def call():
            for _ in range(own.steps):
                pipe.step(batch)
            pipe.flush()
        return call

    for G in own.boxes:
        boxes = boxes_for(100 + G, G, S)
        ts = []
        for r in range(reps):
            t0 = time.perf_counter()
            match, deltas = build_rpn_targets((S, S, 3), anchors, None, boxes, cfg, np.random.RandomState(r))
            ts.append((time.perf_counter() - t0) * 1e3)
        host_ms = float(np.median(ts))
        emit(what="build_rpn_targets_alone", G=G, anchors=int(anchors.shape[0]), wall_ms=round(host_ms, 3), runs_ms=[round(t, 3) for t in ts],
             cpu_threads=torch.get_num_threads(), timing="wall clock on this machine's CPU, median of %d" % reps)
        gt = torch.zeros((1, 512, 4), dtype=torch.float64, device=dev)
        gt[0, :G] = torch.tensor(boxes, dtype=torch.float64)
        gc = torch.tensor([G], dtype=torch.int32, device=dev)
        out = ops.rpn_targets(adev, gt, gc, sizes, n, cfg.RPN_BBOX_STD_DEV, 1)
        dev_ms, dev_all = timed(lambda: ops.rpn_targets(adev, gt, gc, sizes, n, cfg.RPN_BBOX_STD_DEV, 1, out=out), 3, 20)
        emit(what="ops_rpn_targets_alone", G=G, event_ms=round(dev_ms, 4), min_ms=min(dev_all), max_ms=max(dev_all), launches=8,
             timing="device events around the call, median of 20")
        host_batch = [inputs[0], inputs[1], match[None, :, None], deltas[None], inputs[4], inputs[5]]
        dev_batch = [inputs[0], inputs[1], [boxes], None, inputs[4], inputs[5]]
        legs = [piped(host_batch), piped(dev_batch)]
        for _ in range(warm):
            for leg in legs:
                leg()
        torch.cuda.synchronize()
        wall = [[], []]
        for _ in range(reps):
            for i, leg in enumerate(legs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg()
                torch.cuda.synchronize()
                wall[i].append((time.perf_counter() - t0) * 1e3 / own.steps)
        med = [float(np.median(w)) for w in wall]
        spread = [max(w) - min(w) for w in wall]
        allowed = dev_ms + max(spread)
        emit(what="joint_step_pipelined", G=G, host_arrays_ms=round(med[0], 4), device_targets_ms=round(med[1], 4),
             host_arrays_spread_ms=round(spread[0], 4), device_targets_spread_ms=round(spread[1], 4), excess_ms=round(med[1] - med[0], 4),
             allowed_excess_ms=round(allowed, 4), within_allowance=bool(med[1] - med[0] <= allowed),
             host_arrays_runs_ms=[round(t, 4) for t in wall[0]], device_targets_runs_ms=[round(t, 4) for t in wall[1]],
             timing="wall clock per step over calls of %d pipelined steps + flush, legs alternating call by call, median of %d" % (own.steps, reps))

        class Memory(utils.Dataset):                       # a synthetic in-memory dataset: G boxes per image
            def load_image(self, image_id):
                return np.random.RandomState(image_id).randint(0, 255, (S, S, 3)).astype(np.uint8)

            def load_captions_and_rois(self, image_id):
                r = np.random.RandomState(500 + image_id)
                caps = np.zeros((G, args.tokens), np.float32)
                caps[:, 0], caps[:, 1:4], caps[:, 4] = 1, r.randint(3, args.vocab, (G, 3)), 2
                return boxes_for(900 + image_id, G, S), caps
        ds = Memory()
        for i in range(4):
            ds.add_image("memory", image_id=i, path=None)
        ds.prepare()
        for mode in ("host", "device"):
            gen = data_generator(ds, cfg, shuffle=True, batch_size=cfg.BATCH_SIZE, rng=np.random.RandomState(3), rpn_targets=mode)
            pipe.step(next(gen)[0])
            pipe.flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(own.loop_steps):
                pipe.step(next(gen)[0])
            pipe.flush()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            emit(what="train_style_loop", G=G, rpn_targets=mode, steps=own.loop_steps, steps_per_s=round(own.loop_steps / dt, 3),
                 ms_per_step=round(1e3 * dt / own.loop_steps, 2), timing="wall clock, generator (image synthesis, resize, targets) on the stepping thread")
    if own.out:
        os.makedirs(os.path.dirname(own.out) or ".", exist_ok=True)
        with open(own.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
