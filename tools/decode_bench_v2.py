"""Caption decoding of the v2 decoders (inject and merge) per call: CaptionModelV2.generate(decoder='prefix') -- greedy_decode per RoI,
the reference's test loop (the whole model on the pre-padded prefix per token, a [V] row to the host per token) -- against
decoder='incremental' (decode_greedy: one token per step with carried word-LSTM state, ops.vocab_top1) and decoder='beam' with k = 3
and 5 (decode_beam: ops.vocab_topk + ops.beam_step over the k*R beam rows), on synthetic weights; plus ops.vocab_topk alone as a
fraction of the fp32 matrix peak.

Shapes (Tw = 10, 9 tokens, 256 inject units): configs[1] (R = 64, V = 10 000), one image's ground-truth RoIs (R = 50, V = 10 000) and
R = 1000 (V = 10 000).  Times: torch.cuda.Event around the whole generate() call (the host copies of its results included), warm-up
first, median of the repeats (--prefix-repeats for the slow prefix path).  Prints one JSON line per measurement and, with --out, writes
them all to that JSON file (profiles/decode_bench_v2.json).

    python tools/decode_bench_v2.py [--repeats 5] [--prefix-repeats 2] [--out decode_bench_v2.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_PEAK = 157e12          # MI355X dense fp32 matrix peak (TFLOP/s x 1e12)


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


def model_for(V, Tw, units, inject, seed=0):
    from image_captioning_amd import synth
    from image_captioning_amd.text_generation_model_v2 import DenseCapConfig, build_model
    cfg = DenseCapConfig(V, synth.embedding_matrix(seed + 3, V))
    cfg.PADDING_SIZE = Tw
    return build_model((7, 7, 256), (Tw,), cfg, units, inject, seed=seed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--prefix-repeats", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="JSON file for all rows (default: print only)")
    ap.add_argument("--shapes", default="c1,img,r1000")
    ap.add_argument("--modes", default="inject,merge")
    args = ap.parse_args()
    from image_captioning_amd import ops
    torch.cuda.set_device(0)
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    shapes = {"c1": dict(name="configs[1]", R=64, V=10000, Tw=10, units=256),
              "img": dict(name="one image's ground-truth RoIs", R=50, V=10000, Tw=10, units=256),
              "r1000": dict(name="R = 1000", R=1000, V=10000, Tw=10, units=256)}
    decoders = [("prefix", None), ("incremental", None), ("beam", 3), ("beam", 5)]
    for key in args.shapes.split(","):
        sh = shapes[key]
        feat = torch.tensor(np.random.default_rng(1).standard_normal((sh["R"], 7, 7, 256)).astype(np.float32), device="cuda:0")
        for mode in args.modes.split(","):
            model = model_for(sh["V"], sh["Tw"], sh["units"], mode == "inject")
            got, ms = {}, {}
            for dec, k in decoders:
                name = dec if k is None else "beam%d" % k
                call = lambda: model.generate(feat, decoder=dec, beam_size=k)
                got[name] = call()
                reps = args.prefix_repeats if dec == "prefix" else args.repeats
                ms[name], all_ms = timed(call, args.warmup, reps)
                emit(what="decode", shape=sh["name"], mode=mode, decoder=name, R=sh["R"], V=sh["V"], Tw=sh["Tw"], steps=sh["Tw"] - 1,
                     units=sh["units"], ms=round(ms[name], 3), us_per_roi=round(1e3 * ms[name] / sh["R"], 2), runs_ms=all_ms)
            emit(what="decode_summary", shape=sh["name"], mode=mode,
                 speedup_incremental=round(ms["prefix"] / ms["incremental"], 1), speedup_beam3=round(ms["prefix"] / ms["beam3"], 1),
                 speedup_beam5=round(ms["prefix"] / ms["beam5"], 1),
                 ids_identical_fraction=float((got["prefix"][0] == got["incremental"][0]).all(1).mean()),
                 max_abs_score_diff=float(np.abs(got["prefix"][1] - got["incremental"][1]).max()))
            del model
            torch.cuda.empty_cache()
        # the fused vocabulary top-k alone, at the beam step's shape (M = k*R beam rows; K = 256 inject units, 2048 merge inputs)
        V = sh["V"]
        rng = np.random.default_rng(2)
        for K in (256, 2048):
            for k in (3, 5):
                M_ = k * sh["R"]
                X = torch.tensor(rng.standard_normal((M_, K)).astype(np.float32), device="cuda:0")
                W = torch.tensor((rng.standard_normal((K, V)) / np.sqrt(K)).astype(np.float32), device="cuda:0")
                b = torch.zeros(V, dtype=torch.float32, device="cuda:0")
                ids = torch.empty((M_, k), dtype=torch.int32, device="cuda:0")
                pr = torch.empty((M_, k), dtype=torch.float32, device="cuda:0")
                t, all_ms = timed(lambda: ops.vocab_topk(X, W, b, k, ids=ids, probs=pr), 3, 20)
                flops = 2.0 * M_ * K * V
                logits = torch.empty((M_, V), dtype=torch.float32, device="cuda:0")
                tg, _ = timed(lambda: ops.gemm(X, W, shift=b, out=logits), 3, 20)
                emit(what="vocab_topk", shape=sh["name"], M=M_, K=K, V=V, k=k, ms=round(t, 4), tflops=round(flops / t / 1e9, 1),
                     fraction_of_fp32_peak=round(flops / (t * 1e-3) / FP32_PEAK, 3), unfused_gemm_ms=round(tg, 4),
                     unfused_gemm_fraction_of_fp32_peak=round(flops / (tg * 1e-3) / FP32_PEAK, 3), runs_ms=all_ms)
                del X, W, logits
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
