"""What the whole-image captioner's device path costs, measured (nothing here is a target; every figure is reported with the spread of
its repeats, legs alternating within one process).

(a) image-level features of one image: today's path -- generate_features(image, model): the [1000,7,7,256] RoI block copied to the host
    (50 MB) and np.mean(axis=0) there -- against generate_features(..., device_features=True) (ops.row_mean on the device, 50 KB
    handed back), call by call; wall clock per call ending in a device synchronise (the device leg also copies its 50 KB to the host,
    so both legs end with the vector in host memory).  Then dc_row_mean_f32 alone at [1000,12544]: device events around each launch,
    over a ring of 8 input blocks (400 MB, more than the 256 MB Infinity Cache, so every launch reads HBM) and over one block (which
    the cache may hold); achieved bytes/s = (K C + C) 4 bytes / time.
(b) one train step at B = 100, T = 10, V = 8192 with the reference's layer sizes (12544 -> 128, words 256, LSTMs 256 / 1000), device-
    resident inputs: eager (use_step_graph off, the default) against captured (replayed from a hipGraph), two models alternating window by window;
    wall clock per step over a window of steps ending in a device synchronise.
(c) model.generate with k = 5 at R = 1 and R = 16 (T = 10: nine re-runs of the ten-step stack on 5 R prefixes), wall clock per call
    (it ends in its one device-to-host copy), the two alternating call by call.

    python tools/imgcap_bench.py --out profiles/imgcap_bench.json
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


def _stats(per_repeat):
    return dict(ms=round(float(np.median(per_repeat)), 4), repeats_ms=[round(v, 4) for v in per_repeat],
                spread_ms=round(max(per_repeat) - min(per_repeat), 4))


def _wall(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def features(own, rows):
    from image_captioning_amd import ops, synth
    from image_captioning_amd.generate_roi_features import InferenceConfig, generate_features, load_model
    S = own.image_size

    class Cfg(InferenceConfig):
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
    cfg = Cfg()
    Wt = dict(synth.encoder_weights(0, own.stage4_blocks), **synth.rpn_weights(4))
    Wt['rpn_conv_shared/kernel'] = Wt['rpn_conv_shared/kernel'] * np.float32(0.02)
    Wt['rpn_bbox_pred/kernel'] = Wt['rpn_bbox_pred/kernel'] * np.float32(0.3)
    model = load_model(weights=Wt, config=cfg, stage4_blocks=own.stage4_blocks)
    img = synth.images(3, 1, S, S)[0]
    legs = {"host_mean": lambda: generate_features(img, model), "device_mean": lambda: generate_features(img, model, device_features=True).cpu().numpy()}
    same = bool(np.array_equal(legs["host_mean"](), legs["device_mean"]()))
    for _ in range(own.warmup):
        for fn in legs.values():
            fn()
    per = {k: [] for k in legs}
    for _ in range(own.repeats):
        calls = {k: [] for k in legs}
        for _ in range(own.feature_calls):
            for k, fn in legs.items():
                calls[k].append(_wall(fn, 1))
        for k in legs:
            per[k].append(float(np.median(calls[k])))
    for k in legs:
        emit(rows, what="image_level_features", variant=k, image=S, rois=int(cfg.POST_NMS_ROIS_INFERENCE), stage4_blocks=own.stage4_blocks,
             bit_equal_to_host=same, over_device=round(float(np.median(per[k]) / np.median(per["device_mean"])), 3), **_stats(per[k]),
             timing="wall clock per call ending in a device synchronise with the vector in host memory, legs alternating call by call, median of "
                    "%d calls per repeat, median of %d repeats" % (own.feature_calls, own.repeats))
    # the kernel alone
    K, C = 1000, 12544
    ring = [torch.randn((K, C), device="cuda") for _ in range(8)]
    out = torch.empty((C,), device="cuda")
    nbytes = (K * C + C) * 4
    for name, bufs in (("hbm_ring_of_8", ring), ("one_block", ring[:1])):
        for i in range(own.warmup):
            ops.row_mean(bufs[i % len(bufs)], out=out)
        per_k = []
        for _ in range(own.repeats):
            ev = []
            for i in range(own.launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.row_mean(bufs[i % len(bufs)], out=out)
                e1.record()
                ev.append((e0, e1))
            torch.cuda.synchronize()
            per_k.append(float(np.median([a.elapsed_time(b) for a, b in ev])))
        st = _stats(per_k)
        emit(rows, what="row_mean_kernel", inputs=name, K=K, C=C, bytes=nbytes, tb_per_s=round(nbytes / (st["ms"] * 1e-3) / 1e12, 3), **st,
             timing="device events around each launch, median of %d launches per repeat, median of %d repeats" % (own.launches, own.repeats))


def _captioner(V, graph):
    from image_captioning_amd.whole_image.model import create_model
    m = create_model(dict(embedding_dim=128, vocabulary_size=V, max_caption_length=10, batch_size=100), seed=0)
    m.use_step_graph = graph
    return m


def train_step(own, rows):
    V, B, T = 8192, 100, 10
    rng = np.random.default_rng(1)
    feat = torch.tensor(rng.standard_normal((B, 12544)).astype(np.float32), device="cuda")
    words = torch.tensor(rng.integers(0, V, (B, T)).astype(np.int32), device="cuda")
    tgt = torch.tensor(rng.integers(0, V, B).astype(np.int32), device="cuda")
    legs = {"eager": _captioner(V, False), "captured": _captioner(V, True)}
    last = {}
    for k, m in legs.items():
        for _ in range(max(own.warmup, 4)):
            last[k] = m.train_on_batch_device([feat, words], tgt)
    per = {k: [] for k in legs}
    for _ in range(own.repeats):
        for k, m in legs.items():
            per[k].append(_wall(lambda: m.train_on_batch_device([feat, words], tgt), own.steps))
    same = bool(torch.equal(legs["eager"].store.flat, legs["captured"].store.flat))
    for k, m in legs.items():
        cs = [c.last for c in m._steps.values()]
        emit(rows, what="train_step", variant=k, B=B, T=T, V=V, n_train=int(m.store.n_train), step_path=cs, weights_bit_equal_across_legs=same,
             **_stats(per[k]), timing="wall clock per step over %d steps ending in a device synchronise, device-resident inputs, the two "
                                      "models alternating window by window, median of %d repeats" % (own.steps, own.repeats))


def generate(own, rows):
    V = 8192
    m = _captioner(V, False)
    rng = np.random.default_rng(2)
    feats = {R: torch.tensor(rng.standard_normal((R, 12544)).astype(np.float32), device="cuda") for R in (1, 16)}
    for _ in range(own.warmup):
        for R, f in feats.items():
            m.generate(f, beam_size=5, start_id=1)
    per = {R: [] for R in feats}
    for _ in range(own.repeats):
        calls = {R: [] for R in feats}
        for _ in range(own.generate_calls):
            for R, f in feats.items():
                calls[R].append(_wall(lambda: m.generate(f, beam_size=5, start_id=1), 1))
        for R in feats:
            per[R].append(float(np.median(calls[R])))
    for R in feats:
        st = _stats(per[R])
        emit(rows, what="generate", R=R, k=5, T=10, V=V, ms_per_image=round(st["ms"] / R, 4), **st,
             timing="wall clock per call (ends in its one device-to-host copy), R = 1 and R = 16 alternating call by call, median of %d calls "
                    "per repeat, median of %d repeats" % (own.generate_calls, own.repeats))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-size", type=int, default=1024)
    ap.add_argument("--stage4-blocks", type=int, default=22)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--feature-calls", type=int, default=10)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--generate-calls", type=int, default=10)
    ap.add_argument("--skip", nargs="*", default=[], choices=["features", "train", "generate"])
    ap.add_argument("--out", default=None)
    own = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    for name, fn in (("features", features), ("train", train_step), ("generate", generate)):
        if name not in own.skip:
            fn(own, rows)
    if own.out:
        os.makedirs(os.path.dirname(own.out) or ".", exist_ok=True)
        with open(own.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
