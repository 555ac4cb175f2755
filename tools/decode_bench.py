"""Greedy caption decoding per image: CaptionModelV1.generate(decoder='prefix') -- the reference's T zero-padded prefix passes -- against
decoder='incremental' (decode_greedy: one token per step with carried LSTM state, ops.vocab_top1), on synthetic weights, plus
ops.vocab_top1 alone as a fraction of the fp32 matrix peak.  Both decoders run with return_probabilities=False (the prefix path then
still writes and reads its [T*B, V] logits every step, but copies no [B,V] rows to the host).
A bf16 model gets a third leg, decoder='incremental' with vocab_math='bf16' (the vocabulary top-1 on the bf16 matrix pipe), timed
ALTERNATING with the fp32-vocabulary incremental leg in this process (call by call, so both see the same clocks), the share of RoIs
whose captions are identical between the two vocabulary arithmetics, and ops.vocab_top1 on bf16 operands alone at the step's shape on
both tile shapes and the automatic choice, against the bf16 MFMA peak and the time to stream W once from HBM.

Shapes: configs[4] inference (K = 1000 RoIs = POST_NMS_ROIS_INFERENCE, T = 15, V = 50 000, 512 units) and a configs[2]-style one
(K = 200, V = 10 000).  Times: torch.cuda.Event around the whole call (host copies of the ids included), warm-up first, median of
--repeats.  Prints one JSON line per measurement and, with --out, writes them all to that JSON file (profiles/decode_bench.json).

    python tools/decode_bench.py [--repeats 5] [--out decode_bench.json]

--what beam: the beam decoder instead (profiles/decode_bench_beam_v1.json).  Per shape and dtype, generate(decoder='beam') at beam_size 3
and 5, each without an end token and with end_id=2, timed ALTERNATING with the incremental leg of the same vocabulary arithmetic (fp32 model:
fp32; bf16 model: vocab_math='bf16') in one process; then ops.beam_step alone at R = 1000, k = 5 with four row sets of U = 512 (Model 3's
step), alternating with the sequence it replaces: ops.beam_select without rows plus four torch.index_select copies of the same bytes
(their row index made outside the timed region).  Device events, medians of --repeats (at least 5).

    python tools/decode_bench.py --what beam --out profiles/decode_bench_beam_v1.json

--what refine: the joint model's generate_captions end to end per image (1024 x 1024, ResNet-101 + FPN + RPN, the bf16 model with
vocab_math='bf16') with postprocess='host' and 'device', at both shapes (K = POST_NMS_ROIS_INFERENCE), incremental and beam k = 3; the
two legs alternate call by call in one process.  Device events around the call AND wall clock (the host leg's cost is host time, which
events alone do not show; the call ends with its result on the host, so the wall clock covers all of it); medians of --repeats (at
least 5) and max - min spreads.  Then ops.refine_generations alone on random RoIs.  --legs host times the host leg alone and names no
new argument, so the same file measures an older checkout of the package (profiles/refine_generations_bench.json).

    python tools/decode_bench.py --what refine --out profiles/refine_generations_bench.json

--what sampling: decoder='sampling' (ops.vocab_sample, the Gumbel-max draw fused into the vocabulary GEMM) over the whole vocabulary and
at top_k = 5 against decoder='incremental' of the same build, on the fp32 model and on the bf16 model with vocab_math='bf16', at both
shapes; the bf16 model also with the incremental decoder held to the 128 x 128 tile (the sampler's full-vocabulary epilogue exists on
that tile alone; the default tile at these shapes is 256 x 256).  The legs alternate call by call in one process; device events and
wall clock, medians of --repeats (at least 5) with max - min spreads, and each leg's cost over the incremental one per decoded token.
Then the fused vocabulary kernels alone at the step's shape (profiles/sampling_decode_bench.json).

    python tools/decode_bench.py --what sampling --out profiles/sampling_decode_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_PEAK = 157e12          # MI355X dense fp32 matrix peak (TFLOP/s x 1e12)
BF16_PEAK = 2.5e15          # MI355X dense bf16 matrix peak
HBM_PEAK = 8.0e12           # HBM3E bytes / s (spec)


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), [round(t, 3) for t in ts]


def timed_alternating(fns, warm, reps):
    """The calls of `fns` in turn, `reps` rounds after `warm` rounds: [(median ms, [ms ...]) per fn]."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [(float(np.median(t)), [round(x, 3) for x in t]) for t in ts]


def model_for(V, T, K, units, dtype, seed=0):
    from image_captioning_amd import synth
    from image_captioning_amd.text_generation_model import DenseCapConfig, CaptionModelV1
    cfg = DenseCapConfig(V, synth.embedding_matrix(seed + 3, V), K)
    cfg.PADDING_SIZE = T
    return CaptionModelV1([7, 7, 256], cfg, units, 'inference', seed=seed, compute_dtype=dtype)


def beam_legs(args, shapes, rows):
    """--what beam: the beam decoder against the incremental one, then ops.beam_step alone against beam_select + index_select."""
    from image_captioning_amd import ops
    reps, warm = max(args.repeats, 5), max(args.warmup, 1)
    for key in args.shapes.split(","):
        sh = shapes[key]
        for dtype in args.dtypes.split(","):
            model = model_for(sh["V"], sh["T"], sh["K"], sh["units"], dtype)
            feat = torch.tensor(np.random.default_rng(1).standard_normal((sh["K"], 7, 7, 256)).astype(np.float32), device="cuda:0")
            vm = "bf16" if dtype == "bf16" else None
            legs = [(dict(decoder="incremental"), lambda: model.generate(feat, return_probabilities=False, decoder="incremental", vocab_math=vm))]
            for k in (3, 5):
                for end_id in (None, 2):
                    legs.append((dict(decoder="beam", beam_size=k, end_id=end_id),
                                 lambda k=k, e=end_id: model.generate(feat, return_probabilities=False, decoder="beam", beam_size=k, end_id=e, vocab_math=vm)))
            res = timed_alternating([fn for _, fn in legs], warm, reps)
            inc = res[0][0]
            for (kw, _), (ms, all_ms) in zip(legs, res):
                rows.append(dict(what="decode_per_image", shape=sh["name"], dtype=dtype, vocab_math=vm or "f32", alternating=True, K=sh["K"], T=sh["T"],
                                 V=sh["V"], units=sh["units"], ms=round(ms, 3), runs_ms=all_ms, spread_ms=round(max(all_ms) - min(all_ms), 3),
                                 times_incremental=round(ms / inc, 2), timing="device events around the call, median of %d, legs alternating" % reps, **kw))
                print(json.dumps(rows[-1]), flush=True)
            del model
            torch.cuda.empty_cache()
    # the step kernel alone: Model 3's step at configs[4] (four state tensors of 512 units follow their beams)
    R, k, U, nsets = 1000, 5, 512, 4
    rng = np.random.default_rng(3)
    dev = lambda a, dt: torch.tensor(a, dtype=dt, device="cuda:0")
    cid = dev(np.stack([rng.permutation(50000)[:k] for _ in range(k * R)]), torch.int32)
    cp = dev(rng.uniform(1e-4, 0.2, (k * R, k)), torch.float32)
    sin = dev(-rng.uniform(0, 10, (R, k)), torch.float32)
    so = torch.empty((R, k), device="cuda:0")
    par, hist = (torch.zeros((2, R, k), dtype=torch.int32, device="cuda:0") for _ in range(2))
    tok, mask = torch.empty((k * R,), dtype=torch.int32, device="cuda:0"), torch.empty((k * R,), dtype=torch.uint8, device="cuda:0")
    src = [dev(rng.standard_normal((k * R, U)), torch.float32) for _ in range(nsets)]
    dst = [torch.empty((k * R, U), device="cuda:0") for _ in range(nsets)]
    ops.beam_select(cid, cp, sin, so, par, hist, 1, k, True, tokens=tok, mask=mask)
    index = (par[1].t().contiguous().view(-1).long() * R + torch.arange(R, device="cuda:0").repeat(k))       # source row of row q * R + r

    def fused():
        ops.beam_step(cid, cp, sin, so, par, hist, 1, k, True, tokens=tok, mask=mask, rows=list(zip(src, dst)))

    def unfused():
        ops.beam_select(cid, cp, sin, so, par, hist, 1, k, True, tokens=tok, mask=mask)
        for s_, d_ in zip(src, dst):
            torch.index_select(s_, 0, index, out=d_)

    def select_only():
        ops.beam_step(cid, cp, sin, so, par, hist, 1, k, True, tokens=tok, mask=mask)

    fused()
    want = [d_.clone() for d_ in dst]
    unfused()
    same = all(bool(torch.equal(a, b)) for a, b in zip(want, dst))
    res = timed_alternating([fused, unfused, select_only], 3, 20)
    moved = 2.0 * nsets * k * R * U * 4
    for name, (ms, all_ms) in zip(("beam_step, 4 row sets", "beam_select + 4 x index_select", "beam_step, no row sets"), res):
        rows.append(dict(what="beam_step_alone", leg=name, R=R, k=k, U=U, sets=nsets, ms=round(ms, 4), min_ms=min(all_ms), max_ms=max(all_ms),
                         spread_ms=round(max(all_ms) - min(all_ms), 4), copy_bytes=int(moved),
                         copy_tb_per_s=None if name.endswith("no row sets") else round(moved / (ms * 1e-3) / 1e12, 2),
                         timing="device events around the call, median of 20, legs alternating", runs_ms=all_ms))
        print(json.dumps(rows[-1]), flush=True)
    (mf, rf), (mu, ru), _ = res
    spread = max(max(rf) - min(rf), max(ru) - min(ru))
    rows.append(dict(what="beam_step_vs_unfused", fused_ms=round(mf, 4), unfused_ms=round(mu, 4), ratio=round(mu / mf, 2), larger_spread_ms=round(spread, 4),
                     fused_not_slower_beyond_spread=bool(mf <= mu + spread), rows_identical=same))
    print(json.dumps(rows[-1]), flush=True)


def joint_for(sh, dtype, S=1024):
    """The joint model in inference mode on synthetic weights: K proposals per S x S image, the shape's vocabulary."""
    from image_captioning_amd import synth
    from image_captioning_amd.config import Config
    from image_captioning_amd.dense_model import DenseImageCapRCNN

    class Cfg(Config):
        NAME = "joint"
        IMAGES_PER_GPU = 1
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
        PADDING_SIZE = sh["T"]
        VOCABULARY_SIZE = sh["V"]
        EMBEDDING_SIZE = 300
        RECURRENT_DROPOUT = 0.0
        POST_NMS_ROIS_INFERENCE = sh["K"]
    cfg = Cfg()
    cfg.EMBEDDING_WEIGHTS = synth.embedding_matrix(3, sh["V"])
    model = DenseImageCapRCNN("inference", cfg, "logs", lstm_units=sh["units"], compute_dtype=dtype)
    # random FPN maps are O(10): keep the RPN / head activations in a trained network's range (as tools/joint_bench.py)
    w = model.get_weights_dict()
    model.set_weights({"rpn_conv_shared/kernel": w["rpn_conv_shared/kernel"] * np.float32(0.02),
                       "rpn_bbox_pred/kernel": w["rpn_bbox_pred/kernel"] * np.float32(0.3),
                       "mrcnn_class_conv1/kernel": w["mrcnn_class_conv1/kernel"] * np.float32(0.05)})
    return model, cfg


def timed_alternating_wall(fns, warm, reps):
    """timed_alternating with the wall clock beside the events: [(median event ms, [ms ...], median wall ms, [ms ...]) per fn].  Every
    fn returns with its results on the host, so the device is idle when the next one starts."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev, wall = [[] for _ in fns], [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            b.synchronize()
            wall[i].append((time.perf_counter() - t0) * 1e3)
            ev[i].append(a.elapsed_time(b))
    return [(float(np.median(e)), [round(x, 3) for x in e], float(np.median(w)), [round(x, 3) for x in w]) for e, w in zip(ev, wall)]


def refine_legs(args, shapes, rows):
    """--what refine: generate_captions with the post-processing on the host and on the device, then ops.refine_generations alone."""
    from image_captioning_amd import ops, synth
    reps, warm = max(args.repeats, 5), max(args.warmup, 2)
    posts = ("host",) if args.legs == "host" else ("host", "device")
    img = synth.images(7, 1, 1024, 1024)[0]
    for key in args.shapes.split(","):
        sh = shapes[key]
        model, cfg = joint_for(sh, "bf16")
        for kw in (dict(decoder="incremental"), dict(decoder="beam", beam_size=3)):
            # (the host leg is called without the argument: the default, and the call an older checkout understands)
            fns = [lambda kw=kw, p=p: model.generate_captions([img], return_probabilities=False, vocab_math="bf16",
                                                              **dict(kw, **({} if p == "host" else dict(postprocess=p)))) for p in posts]
            out = [fn() for fn in fns]
            same = None if len(out) < 2 else all(np.array_equal(out[0][0][k_], out[1][0][k_]) for k_ in out[0][0])
            res = timed_alternating_wall(fns, warm, reps)
            for p, (ems, eall, wms, wall) in zip(posts, res):
                rows.append(dict(what="generate_captions_per_image", shape=sh["name"], dtype="bf16", vocab_math="bf16", postprocess=p, K=sh["K"],
                                 T=sh["T"], V=sh["V"], image=1024, kept=int(len(out[0][0]["rois"])), event_ms=round(ems, 3),
                                 event_spread_ms=round(max(eall) - min(eall), 3), wall_ms=round(wms, 3), wall_spread_ms=round(max(wall) - min(wall), 3),
                                 event_runs_ms=eall, wall_runs_ms=wall, timing="median of %d, legs alternating call by call" % reps, **kw))
                print(json.dumps(rows[-1]), flush=True)
            if len(res) == 2:
                (_, _, wh, rh), (_, _, wd, rd) = res
                spread = max(max(rh) - min(rh), max(rd) - min(rd))
                rows.append(dict(what="postprocess_device_vs_host", shape=sh["name"], K=sh["K"], host_wall_ms=round(wh, 3), device_wall_ms=round(wd, 3),
                                 gain_ms=round(wh - wd, 3), larger_spread_ms=round(spread, 3), device_faster_beyond_spread=bool(wh - wd > spread),
                                 results_identical=same, **kw))
                print(json.dumps(rows[-1]), flush=True)
        del model
        torch.cuda.empty_cache()
        if args.legs == "host":
            continue
        # the post-processing launches alone: K random RoIs, the greedy decoder's word scores
        from image_captioning_amd import dense_model
        K, T = sh["K"], sh["T"]
        rng = np.random.default_rng(5)
        yx, hw = rng.uniform(0, 0.8, (K, 2)), rng.uniform(0.03, 0.2, (K, 2))
        rois = torch.tensor(np.concatenate([yx, yx + hw], axis=1)[None].astype(np.float32), device="cuda:0")
        ws = torch.tensor(rng.uniform(0.05, 1.0, (K, T)).astype(np.float32), device="cuda:0")
        consts = torch.tensor(dense_model.refine_constants((0, 0, 1024, 1024), cfg, (1024, 1024, 3))[None], device="cuda:0")
        ms, all_ms = timed(lambda: ops.refine_generations(rois, consts, 0.3, 100, word_scores=ws), 3, 20)
        t0 = time.perf_counter()
        for _ in range(20):
            dense_model.refine_generations(rois[0].cpu().numpy(), ws.cpu().numpy(), (0, 0, 1024, 1024), cfg)
        host_ms = (time.perf_counter() - t0) / 20 * 1e3
        rows.append(dict(what="refine_generations_alone", shape=sh["name"], K=K, T=T, max_instances=100, ms=round(ms, 4), min_ms=min(all_ms),
                         max_ms=max(all_ms), launches=5, numpy_host_ms=round(host_ms, 3), timing="device events around the call, median of 20", runs_ms=all_ms))
        print(json.dumps(rows[-1]), flush=True)


def sampling_legs(args, shapes, rows):
    """--what sampling: the sampling decoder against the incremental one, then the fused vocabulary kernels alone at the step's shape."""
    from image_captioning_amd import decoding, ops
    reps, warm = max(args.repeats, 5), max(args.warmup, 1)
    for key in args.shapes.split(","):
        sh = shapes[key]
        for dtype in args.dtypes.split(","):
            model = model_for(sh["V"], sh["T"], sh["K"], sh["units"], dtype)
            feat = torch.tensor(np.random.default_rng(1).standard_normal((sh["K"], 7, 7, 256)).astype(np.float32), device="cuda:0")
            vm = "bf16" if dtype == "bf16" else None
            gen = lambda **kw: model.generate(feat, return_probabilities=False, vocab_math=vm, **kw)
            legs = [(dict(decoder="incremental"), lambda: gen(decoder="incremental")),
                    (dict(decoder="sampling", top_k=None), lambda: gen(decoder="sampling", seed=1)),
                    (dict(decoder="sampling", top_k=5), lambda: gen(decoder="sampling", seed=1, top_k=5))]
            if vm:                                          # the greedy decoder held to the 128 tile, the one the sampler's epilogue exists on
                def top1_128(j, x, W, bias, **out):
                    ops.vocab_top1(x, W, bias, tile=128, **out)
                B = sh["K"]
                legs.append((dict(decoder="incremental", tile=128), lambda: decoding.greedy_views(
                    decoding.greedy(B, model.T, model.device, lambda: model._decode_setup(feat, B, 'dec_', vm), select=top1_128).cpu().numpy())))
            res = timed_alternating_wall([fn for _, fn in legs], warm, reps)
            inc = res[0][0]
            for (kw, _), (ems, eall, wms, wall) in zip(legs, res):
                rows.append(dict(what="decode_per_image", shape=sh["name"], dtype=dtype, vocab_math=vm or "f32", K=sh["K"], T=sh["T"], V=sh["V"],
                                 units=sh["units"], event_ms=round(ems, 3), event_spread_ms=round(max(eall) - min(eall), 3), wall_ms=round(wms, 3),
                                 wall_spread_ms=round(max(wall) - min(wall), 3), times_incremental=round(ems / inc, 3),
                                 over_incremental_us_per_token=round((ems - inc) * 1e3 / (sh["K"] * sh["T"]), 4), event_runs_ms=eall, wall_runs_ms=wall,
                                 timing="median of %d, legs alternating call by call" % reps, **kw))
                print(json.dumps(rows[-1]), flush=True)
            del model
            torch.cuda.empty_cache()
        # the fused vocabulary kernels alone, at the decode step's shape (M = K live rows, 1024 inputs), on fp32 and bf16 operands
        M_, Kd, V = sh["K"], 1024, sh["V"]
        rng = np.random.default_rng(2)
        X = torch.tensor(rng.standard_normal((M_, Kd)).astype(np.float32), device="cuda:0")
        W = torch.tensor((rng.standard_normal((Kd, V)) / 32).astype(np.float32), device="cuda:0")
        b = torch.zeros(V, dtype=torch.float32, device="cuda:0")
        tok = torch.empty(M_, dtype=torch.int32, device="cuda:0")
        for dtype, (Xo, Wo) in (("f32", (X, W)), ("bf16", (X.to(torch.bfloat16), W.to(torch.bfloat16)))):
            tiles = ((None, None),) if dtype == "f32" else ((128, 128), (None, ops.vocab_topk_bf16_tile(M_, V, Kd)))
            legs = [(dict(op="vocab_top1", tile=run), lambda t=t: ops.vocab_top1(Xo, Wo, b, tokens=tok, tile=t)) for t, run in tiles]
            legs.append((dict(op="vocab_sample", top_k=None, tile=None if dtype == "f32" else 128), lambda: ops.vocab_sample(Xo, Wo, b, seed=1, tokens=tok)))
            legs += [(dict(op="vocab_sample", top_k=5, tile=run), lambda t=t: ops.vocab_sample(Xo, Wo, b, seed=1, top_k=5, tokens=tok, tile=t))
                     for t, run in tiles]
            res = timed_alternating([fn for _, fn in legs], 3, 20)
            for (kw, _), (ms, all_ms) in zip(legs, res):
                rows.append(dict(what="vocab_step_alone", shape=sh["name"], dtype=dtype, M=M_, K=Kd, V=V, ms=round(ms, 4),
                                 spread_ms=round(max(all_ms) - min(all_ms), 4), times_first_leg=round(ms / res[0][0], 3),
                                 timing="device events, median of 20, legs alternating", runs_ms=all_ms, **kw))
                print(json.dumps(rows[-1]), flush=True)
        del X, W
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="JSON file for all rows (default: print only)")
    ap.add_argument("--shapes", default="c4,c2")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--what", default="greedy", choices=("greedy", "beam", "refine", "sampling"),
                    help="greedy: prefix / incremental (default); beam: the beam decoder; refine: generate_captions' post-processing on the host / device; "
                         "sampling: the sampling decoder against the incremental one")
    ap.add_argument("--legs", default="both", choices=("both", "host"), help="--what refine: both legs (default) or the host leg alone")
    args = ap.parse_args()
    from image_captioning_amd import ops
    torch.cuda.set_device(0)
    rows = []
    shapes = {"c4": dict(name="configs[4] inference", K=1000, T=15, V=50000, units=512),
              "c2": dict(name="configs[2]-style", K=200, T=15, V=10000, units=512)}
    if args.what == "beam":
        beam_legs(args, shapes, rows)
    if args.what == "refine":
        refine_legs(args, shapes, rows)
    if args.what == "sampling":
        sampling_legs(args, shapes, rows)
    for key in args.shapes.split(",") if args.what == "greedy" else ():
        sh = shapes[key]
        for dtype in args.dtypes.split(","):
            model = model_for(sh["V"], sh["T"], sh["K"], sh["units"], dtype)
            feat = torch.tensor(np.random.default_rng(1).standard_normal((sh["K"], 7, 7, 256)).astype(np.float32), device="cuda:0")
            got = {}
            for dec in ("prefix", "incremental"):
                got[dec] = model.generate(feat, return_probabilities=False, decoder=dec)
                ms, all_ms = timed(lambda: model.generate(feat, return_probabilities=False, decoder=dec), args.warmup, args.repeats)
                rows.append(dict(what="decode_per_image", shape=sh["name"], dtype=dtype, decoder=dec, K=sh["K"], T=sh["T"], V=sh["V"],
                                 units=sh["units"], ms=round(ms, 3), runs_ms=all_ms))
                print(json.dumps(rows[-1]), flush=True)
            same = bool(np.array_equal(got["prefix"][1], got["incremental"][1]))
            rel = float(np.max(np.abs(got["prefix"][2] - got["incremental"][2]) / np.maximum(got["prefix"][2], 1e-30)))
            p, i = rows[-2]["ms"], rows[-1]["ms"]
            rows.append(dict(what="decode_speedup", shape=sh["name"], dtype=dtype, speedup=round(p / i, 2), ids_identical=same,
                             max_rel_score_diff=rel))
            print(json.dumps(rows[-1]), flush=True)
            if dtype == "bf16":
                # the two vocabulary arithmetics of the incremental decoder, call by call in turn
                legs = (("f32", lambda: model.generate(feat, return_probabilities=False, decoder="incremental", vocab_math="f32")),
                        ("bf16", lambda: model.generate(feat, return_probabilities=False, decoder="incremental", vocab_math="bf16")))
                out = [fn() for _, fn in legs]
                res = timed_alternating([fn for _, fn in legs], max(args.warmup, 1), max(args.repeats, 5))
                for (vm, _), (ms, all_ms) in zip(legs, res):
                    rows.append(dict(what="decode_per_image", shape=sh["name"], dtype=dtype, decoder="incremental", vocab_math=vm, alternating=True,
                                     K=sh["K"], T=sh["T"], V=sh["V"], units=sh["units"], ms=round(ms, 3), runs_ms=all_ms,
                                     spread_ms=round(max(all_ms) - min(all_ms), 3)))
                    print(json.dumps(rows[-1]), flush=True)
                (m32, r32), (m16, r16) = res
                spread = max(max(r32) - min(r32), max(r16) - min(r16))
                same_rois = (out[0][1] == out[1][1]).all(axis=1)
                first = np.where(same_rois, sh["T"], (out[0][1] != out[1][1]).argmax(axis=1))
                rows.append(dict(what="vocab_math_bf16_vs_f32", shape=sh["name"], dtype=dtype, f32_ms=round(m32, 3), bf16_ms=round(m16, 3),
                                 speedup=round(m32 / m16, 2), larger_spread_ms=round(spread, 3), gain_exceeds_spread=bool(m32 - m16 > spread),
                                 identical_caption_share=round(float(same_rois.mean()), 4), mean_first_differing_step=round(float(first.mean()), 2)))
                print(json.dumps(rows[-1]), flush=True)
            del model
            torch.cuda.empty_cache()
        # the fused vocabulary top-1 alone, at the decode step's shape (M = K live rows, 1024 inputs)
        M_, Kd, V = sh["K"], 1024, sh["V"]
        rng = np.random.default_rng(2)
        X = torch.tensor(rng.standard_normal((M_, Kd)).astype(np.float32), device="cuda:0")
        W = torch.tensor((rng.standard_normal((Kd, V)) / 32).astype(np.float32), device="cuda:0")
        b = torch.zeros(V, dtype=torch.float32, device="cuda:0")
        tok = torch.empty(M_, dtype=torch.int32, device="cuda:0")
        ms, all_ms = timed(lambda: ops.vocab_top1(X, W, b, tokens=tok), 3, 20)
        flops = 2.0 * M_ * Kd * V
        rows.append(dict(what="vocab_top1", shape=sh["name"], M=M_, K=Kd, V=V, ms=round(ms, 4), tflops=round(flops / ms / 1e9, 1),
                         fraction_of_fp32_peak=round(flops / (ms * 1e-3) / FP32_PEAK, 3), runs_ms=all_ms))
        print(json.dumps(rows[-1]), flush=True)
        logits = torch.empty((M_, V), dtype=torch.float32, device="cuda:0")
        ms_g, _ = timed(lambda: ops.gemm(X, W, shift=b, out=logits), 3, 20)
        rows.append(dict(what="unfused_gemm_same_shape", shape=sh["name"], M=M_, K=Kd, V=V, ms=round(ms_g, 4),
                         fraction_of_fp32_peak=round(flops / (ms_g * 1e-3) / FP32_PEAK, 3)))
        print(json.dumps(rows[-1]), flush=True)
        # the same step on bf16 operands: both tile shapes forced and the automatic choice; the roof is the larger of the MFMA time at
        # the bf16 peak and the time to stream W [K,V] bf16 once from HBM
        Xb, Wb = X.to(torch.bfloat16), W.to(torch.bfloat16)
        t_mfma, t_hbm = flops / BF16_PEAK * 1e3, Kd * V * 2.0 / HBM_PEAK * 1e3
        auto = ops.vocab_topk_bf16_tile(M_, V, Kd)
        res = timed_alternating([lambda t=t: ops.vocab_top1(Xb, Wb, b, tokens=tok, tile=t) for t in (128, 256, 0)], 3, 20)
        for t, (ms, all_ms) in zip((128, 256, 0), res):
            rows.append(dict(what="vocab_top1_bf16", shape=sh["name"], M=M_, K=Kd, V=V, tile=t, tile_run=t or auto, ms=round(ms, 4),
                             tflops=round(flops / ms / 1e9, 1), fraction_of_bf16_peak=round(flops / (ms * 1e-3) / BF16_PEAK, 3),
                             mfma_roof_ms=round(t_mfma, 4), hbm_w_once_roof_ms=round(t_hbm, 4), larger_roof="mfma" if t_mfma > t_hbm else "hbm",
                             fraction_of_larger_roof=round(max(t_mfma, t_hbm) / ms, 3), runs_ms=all_ms))
            print(json.dumps(rows[-1]), flush=True)
        faster = 128 if res[0][0] <= res[1][0] else 256
        rows.append(dict(what="vocab_top1_bf16_tile_choice", shape=sh["name"], automatic=auto, faster=faster, automatic_is_faster=bool(auto == faster)))
        print(json.dumps(rows[-1]), flush=True)
        del X, W, Xb, Wb, logits
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
