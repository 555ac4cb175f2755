"""What the choice of optimizer costs per step: ONE fused update launch over the joint model's flat parameter bucket (about 77 M fp32
elements) under AMSGrad (ops.amsgrad_step, the default and the yardstick), Adam, SGD with momentum and plain SGD (ops.optimizer_step).
Per element AMSGrad reads five streams (p, g, m, v, vhat) and writes four; Adam 4 + 3, SGD with momentum 3 + 2, plain SGD 2 + 1: the
bytes a launch must move are 9 : 7 : 5 : 3.

Per-launch timing, twice -- plain (no segment table, no bf16 shadow) and as the joint step launches it (the regulariser's segment table
+ the bf16 shadow of the whole bucket + the norm clip): device events around every single launch after a warm-up, --launches (200)
launches of each variant, the four variants ALTERNATING launch by launch in one process, the whole thing --repeats (3) times.  A
repeat's figure is the median of its launches; reported: the median of the repeats, their max - min spread, the bytes moved and TB/s,
and each variant's time over AMSGrad's.  no_slower_than_amsgrad: variant <= AMSGrad + the spread of AMSGrad's repeats in this run.

    python tools/optimizer_bench.py --out profiles/optimizer_bench.json

--step: the pipelined joint train step (pipeline.JointTrainPipeline, what train() runs) at the configs[4] shape under each of the four
optimizers: per repeat (5) and optimizer compile(), warm up, then --steps (100) steps + the flush by the wall clock -- the optimizers
alternate within a repeat -- and, by device events, the optimizer's two passes alone (reg_sumsq + the update with the segment table and
the shadow: Optimizer.apply as the step calls it), 20 calls.  Median, minimum and every repeat are reported; one pipeline (one pair of side streams) serves every leg.  No
threshold: the update is one launch of a step of a few hundred.

    python tools/optimizer_bench.py --step --out profiles/optimizer_bench_step.json
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

JOINT_BUCKET = 77_000_000       # the joint model's trainable parameters at configs[4] (V = 50 000), rounded
# variant -> (streams read, streams written) per element
STREAMS = {"amsgrad": (5, 4), "adam": (4, 3), "sgd_momentum": (3, 2), "sgd_plain": (2, 1)}


def emit(rows, **row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def segment_table(ops, n, dev):
    """A table shaped like the joint model's: a few dozen runs, the last (the vocabulary layer) two thirds of the bucket, BatchNorm-like
    runs without a coefficient, one frozen run; run ends are no multiples of 4."""
    rng = np.random.RandomState(0)
    cuts = np.unique(np.concatenate([[0], np.sort(rng.randint(1, n // 3, 40)), [n // 3 + 1, n]]))
    coef = np.zeros(n, np.float32)
    mask = np.ones(n, np.float32)
    for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        coef[lo:hi] = 0.0 if i % 5 == 4 else 1e-4 / (hi - lo)
    mask[cuts[3]:cuts[4]] = 0.0
    coef[cuts[3]:cuts[4]] = 0.0
    return ops.RegSegmentTable(coef, mask, dev)


def launches(own):
    from image_captioning_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    n = own.n
    rows = []
    gen = torch.Generator(device=dev).manual_seed(0)
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    gn = torch.full((1,), float((g * g).sum().item()), device=dev)
    segs = segment_table(ops, n, dev)
    for fused in (False, True):
        p = {k: torch.randn(n, device=dev, generator=gen) for k in STREAMS}
        st = {k: [torch.zeros(n, device=dev) for _ in range(sum(STREAMS[k]) // 2 - 1)] for k in STREAMS}      # 3, 2, 1, 0 state buckets
        shadow = torch.empty(n // 4 * 4, dtype=torch.bfloat16, device=dev) if fused else None
        kw = dict(gnorm_sq=gn, clipnorm=0.5, p_bf16=shadow, reg=segs) if fused else {}
        call = {
            "amsgrad": lambda: ops.amsgrad_step(p["amsgrad"], g, *st["amsgrad"], 1e-5, **kw),
            "adam": lambda: ops.optimizer_step("adam", p["adam"], g, st["adam"], 1e-5, **kw),
            "sgd_momentum": lambda: ops.optimizer_step("sgd", p["sgd_momentum"], g, st["sgd_momentum"], 1e-5, beta1=0.9, **kw),
            "sgd_plain": lambda: ops.optimizer_step("sgd", p["sgd_plain"], g, (), 1e-5, beta1=0.0, **kw),
        }
        for _ in range(own.warmup):
            for k in STREAMS:
                call[k]()
        torch.cuda.synchronize()
        per_repeat = {k: [] for k in STREAMS}
        for _ in range(own.repeats):
            ev = {k: [] for k in STREAMS}
            for _ in range(own.launches):
                for k in STREAMS:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call[k]()
                    e1.record()
                    ev[k].append((e0, e1))
            torch.cuda.synchronize()
            for k in STREAMS:
                per_repeat[k].append(float(np.median([a.elapsed_time(b) for a, b in ev[k]])))
        base = float(np.median(per_repeat["amsgrad"]))
        margin = max(per_repeat["amsgrad"]) - min(per_repeat["amsgrad"])
        for k, (rd, wr) in STREAMS.items():
            ms = float(np.median(per_repeat[k]))
            nbytes = (rd + wr) * 4 * n + (2 * shadow.numel() if fused else 0)
            emit(rows, what="one_launch", variant=k, n=n, segment_table_and_bf16_shadow=fused, ms=round(ms, 4),
                 repeats_ms=[round(t, 4) for t in per_repeat[k]], spread_ms=round(max(per_repeat[k]) - min(per_repeat[k]), 4),
                 bytes=nbytes, tb_per_s=round(nbytes / (ms * 1e-3) / 1e12, 3), over_amsgrad=round(ms / base, 4),
                 bytes_over_amsgrad=round((rd + wr) / 9.0, 4), amsgrad_spread_ms=round(margin, 4), no_slower_than_amsgrad=bool(ms <= base + margin),
                 timing="device events around each launch, median of %d launches per repeat, variants alternating launch by launch, "
                        "median of %d repeats" % (own.launches, own.repeats))
        del p, st, shadow
    return rows


def steps(own, rest):
    sys.argv = [sys.argv[0], "--config", "joint"] + rest
    import bench
    args = bench.parse()
    from image_captioning_amd.params import Adam, SGD
    from image_captioning_amd.pipeline import JointTrainPipeline
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    model, inner, inputs, cfg = bench.build_joint(args, dev)
    make = {"amsgrad": lambda: None,                                       # compile()'s default: Adam(clipnorm=0.5, amsgrad=True)
            "adam": lambda: Adam(clipnorm=0.5),
            "sgd_momentum": lambda: SGD(momentum=float(cfg.LEARNING_MOMENTUM), clipnorm=5.0),
            "sgd_plain": lambda: SGD(clipnorm=5.0)}
    rows, wall, alone = [], {k: [] for k in make}, {k: [] for k in make}
    # ONE pipeline for every leg: a pipeline makes its backbone and copy streams when it is built, and which hardware queues a new pair
    # of streams lands on moved whole 100-step windows by 1 - 3 ms per step under any optimizer (a pipeline per leg: 6.57 / 7.56 ms for
    # AMSGrad, 6.30 / 9.80 for SGD with momentum in one run) while the passes alone stayed within 0.01 ms
    pipe = JointTrainPipeline(inner)
    for _ in range(own.step_repeats):
        for k in make:
            inner.compile(1e-5, optimizer=make[k]())
            for _ in range(own.warmup):
                pipe.step(inputs)
            pipe.flush()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(own.steps):
                pipe.step(inputs)
            pipe.flush()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3 / own.steps)
            segs = inner._reg_segments()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                inner.optimizer.apply(inner.store, reg=segs)
            e1.record()
            torch.cuda.synchronize()
            alone[k].append(e0.elapsed_time(e1) / 20)
    base, base_alone = float(np.median(wall["amsgrad"])), float(np.median(alone["amsgrad"]))
    for k in make:
        ms, ams = float(np.median(wall[k])), float(np.median(alone[k]))
        emit(rows, what="joint_step_pipelined", optimizer=k, n_train=int(inner.store.n_train), ms_per_step=round(ms, 4), min_ms_per_step=round(min(wall[k]), 4),
             repeats_ms=[round(t, 4) for t in wall[k]], spread_ms=round(max(wall[k]) - min(wall[k]), 4), minus_amsgrad_ms=round(ms - base, 4),
             min_minus_amsgrad_min_ms=round(min(wall[k]) - min(wall["amsgrad"]), 4), optimizer_passes_alone_ms=round(ams, 4),
             optimizer_passes_alone_minus_amsgrad_ms=round(ams - base_alone, 4), optimizer_passes_alone_repeats_ms=[round(t, 4) for t in alone[k]],
             timing="wall clock per step over %d pipelined steps + flush after compile() and %d warm-up steps, optimizers alternating within a "
                    "repeat, median / minimum of %d repeats; the passes alone: device events around 20 apply() calls" % (own.steps, own.warmup, own.step_repeats))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=JOINT_BUCKET, help="elements of the bucket (per-launch timing)")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10, help="launches of each variant (per-launch timing) / steps (--step) before the timed ones")
    ap.add_argument("--step", action="store_true", help="time the pipelined joint step under each optimizer instead")
    ap.add_argument("--steps", type=int, default=100, help="steps per timed call (--step)")
    ap.add_argument("--step-repeats", type=int, default=5, help="repeats of --step")
    ap.add_argument("--out", default=None)
    own, rest = ap.parse_known_args()
    rows = steps(own, rest) if own.step else launches(own)
    if own.out:
        os.makedirs(os.path.dirname(own.out) or ".", exist_ok=True)
        with open(own.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
