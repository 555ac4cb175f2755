"""What train(mold="device", prefetch=n) buys: the joint model at the configs[4] shape (bf16, 1024 x 1024 canvas) trained from an in-memory
dataset of raw 600 x 800 uint8 images (-> 768 x 1024, 128 rows of padding above and below), rpn_targets="device".

(a) the three resize launches alone (ops.resize_pad_packed on an uploaded batch), device events, median of 20: the old entry point
    (dc_resize_pad_u8, the yardstick), the new one with every flag 0 and with every flag 1.
(b) the pipelined joint step (pipeline.JointTrainPipeline, what train() runs) fed device-resident uint8 canvases -- the fastest path
    there is, the yardstick -- and fed raw batches (packed on the host, uploaded on the copy stream, resized on the backbone stream):
    the legs alternate call by call in one process, a call being --steps steps plus the flush, medians of --repeats (at least 5) with
    the max - min spread.  Allowed excess: the launches' own time from (a) plus the larger spread.
(c) the loop data_generator -> pipe.step, wall clock per step, in four legs: mold="host" / "device", each with prefetch 0 / 2.

    python tools/train_mold_bench.py --out profiles/train_mold_bench.json
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
from rpn_targets_bench import boxes_for  # noqa: E402

RAW = (600, 800)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed call of a step leg")
    ap.add_argument("--loop-steps", type=int, default=12, help="steps of the generator loop per leg")
    ap.add_argument("--boxes", type=int, default=50, help="ground-truth boxes per image")
    ap.add_argument("--out", default=None)
    own, rest = ap.parse_known_args()
    sys.argv = [sys.argv[0], "--config", "joint"] + rest
    args = bench.parse()
    from image_captioning_amd import ops, utils
    from image_captioning_amd.dense_model import data_generator
    from image_captioning_amd.pipeline import JointTrainPipeline
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    reps, warm = max(own.repeats, 5), max(own.warmup, 2)
    model, inner, inputs, cfg = bench.build_joint(args, dev)
    S, B, G = args.image_size, int(cfg.BATCH_SIZE), own.boxes
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    class Memory(utils.Dataset):                           # raw images held in memory: load_image stands for a decode that costs nothing
        def load_image(self, image_id):
            return self.pixels[image_id]

        def load_captions_and_rois(self, image_id):
            r = np.random.RandomState(500 + image_id)
            caps = np.zeros((G, args.tokens), np.float32)
            caps[:, 0], caps[:, 1:4], caps[:, 4] = 1, r.randint(3, args.vocab, (G, 3)), 2
            return boxes_for(900 + image_id, G, S), caps
    ds = Memory()
    ds.pixels = [np.random.default_rng(i).integers(0, 256, RAW + (3,), dtype=np.uint8) for i in range(4)]
    for i in range(4):
        ds.add_image("memory", image_id=i, path=None)
    ds.prepare()

    # ---- (a) the launches alone
    images = [ds.pixels[b % 4] for b in range(B)]
    geo = [utils.resize_geometry(im.shape, cfg.IMAGE_MIN_DIM, cfg.IMAGE_MAX_DIM, True) for im in images]
    place = [(g[0], g[1], g[2][0], g[2][1]) for g in geo]
    packed, records = ops.pack_resize_batch(images, place, [False] * B)        # (a buffer with flags serves both entry points)
    pdev = torch.from_numpy(packed).to(dev)
    out = torch.empty((B, S, S, 3), dtype=torch.uint8, device=dev)
    alone = {}
    for name, flips in (("old_entry_point", None), ("flags_0", [False] * B), ("flags_1", [True] * B)):
        if flips is not None:
            pdev[B * 32:B * 36].copy_(torch.from_numpy(np.asarray(flips, np.int32).view(np.uint8)))
        ms, runs = timed(lambda: ops.resize_pad_packed(pdev, records, out=out, flips=flips), 3, 20)
        alone[name] = ms
        emit(what="resize_launches_alone", leg=name, B=B, raw="%dx%d" % RAW, resized="%dx%d" % geo[0][:2], event_ms=round(ms, 4), min_ms=min(runs),
             max_ms=max(runs), launches=3, timing="device events around the call, median of 20")
    emit(what="resize_launches_ratio", flags_0_over_old=round(alone["flags_0"] / alone["old_entry_point"], 4),
         flags_1_over_old=round(alone["flags_1"] / alone["old_entry_point"], 4))

    # ---- (b) the pipelined step: device-resident canvases against raw batches
    for _ in range(8):
        inner.train_on_batch(inputs)
    pipe = JointTrainPipeline(inner)
    raw_gen = data_generator(ds, cfg, shuffle=False, batch_size=B, rng=np.random.RandomState(3), rpn_targets="device", mold="device")
    raw_batch = next(raw_gen)[0]
    canvas = torch.empty((B, S, S, 3), dtype=torch.uint8, device=dev)
    ops.resize_pad_images(raw_batch[0].images, cfg.IMAGE_MIN_DIM, cfg.IMAGE_MAX_DIM, out=canvas, flips=raw_batch[0].flips)
    resident_batch = [canvas] + raw_batch[1:]

    def piped(batch):
        def call():
            for _ in range(own.steps):
                pipe.step(batch)
            pipe.flush()
        return call
    legs = [piped(resident_batch), piped(raw_batch)]
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
    allowed = alone["flags_1"] + max(spread)
    emit(what="joint_step_pipelined", resident_canvas_ms=round(med[0], 4), raw_batch_ms=round(med[1], 4), resident_spread_ms=round(spread[0], 4),
         raw_spread_ms=round(spread[1], 4), excess_ms=round(med[1] - med[0], 4), allowed_excess_ms=round(allowed, 4),
         within_allowance=bool(med[1] - med[0] <= allowed), resident_runs_ms=[round(t, 4) for t in wall[0]],
         raw_runs_ms=[round(t, 4) for t in wall[1]], packed_bytes=int(packed.size),
         timing="wall clock per step over calls of %d pipelined steps + flush, legs alternating call by call, median of %d" % (own.steps, reps))
    t0 = time.perf_counter()
    for _ in range(reps):
        inner.plan().pack_images(raw_batch[0].images, cfg.IMAGE_MIN_DIM, cfg.IMAGE_MAX_DIM, True, raw_batch[0].flips)
    emit(what="pack_images_alone", wall_ms=round((time.perf_counter() - t0) * 1e3 / reps, 3), timing="wall clock on this machine's CPU, mean of %d" % reps)

    # ---- (c) the generator loop, four legs
    for mold in ("host", "device"):
        for prefetch in (0, 2):
            gen = data_generator(ds, cfg, shuffle=True, batch_size=B, rng=np.random.RandomState(3), rpn_targets="device", mold=mold)
            if prefetch:
                gen = utils.Prefetcher(gen, prefetch)
            pipe.step(next(gen)[0])
            pipe.flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(own.loop_steps):
                pipe.step(next(gen)[0])
            pipe.flush()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            gen.close()
            emit(what="generator_loop", mold=mold, prefetch=prefetch, steps=own.loop_steps, ms_per_step=round(1e3 * dt / own.loop_steps, 2),
                 steps_per_s=round(own.loop_steps / dt, 3), timing="wall clock; prefetch 0: the generator runs on the stepping thread")
    if own.out:
        os.makedirs(os.path.dirname(own.out) or ".", exist_ok=True)
        with open(own.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
