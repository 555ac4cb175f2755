"""What mold="device" buys: generate_captions end to end with the images resized on the host (utils.resize_image: PIL, np.pad, np.stack,
upload of the molded 1024 x 1024 batch) and on the device (upload of the raw bytes, ops.resize_pad_images into the plan's image buffer).

The six committed 600 x 800 sample JPEGs (tests/golden/sample_images/), decoded once, through the bf16 joint model at the configs[4]
inference shape (1024 x 1024, ResNet-101 + FPN + RPN, 1000 proposals, T = 15, V = 50 000) with decoder="incremental", vocab_math="bf16",
postprocess="device", IMAGE_MIN_DIM = 800, IMAGE_MAX_DIM = 1024.  The two legs alternate call by call in one process, one image per
call, the images in turn; device events and the wall clock around each call, medians of --repeats (at least 5) with the max - min
spread.  mold="host" is the default code path and the yardstick.  Then ops.resize_pad_images alone (device events, upload included, and
the launches alone on an uploaded batch) and the host stage alone on this machine's CPU (utils.resize_image + np.stack, wall clock).

    python tools/mold_bench.py --out profiles/mold_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from decode_bench import joint_for, timed, timed_alternating_wall  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sample_images():
    from image_captioning_amd import utils
    folder = os.path.join(ROOT, "tests", "golden", "sample_images")
    return [utils.imread(os.path.join(folder, n)) for n in sorted(os.listdir(folder))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="JSON file for all rows (default: print only)")
    ap.add_argument("--skip-model", action="store_true", help="only the resize alone and the host stage alone")
    args = ap.parse_args()
    from image_captioning_amd import ops, utils
    torch.cuda.set_device(0)
    reps, warm = max(args.repeats, 5), max(args.warmup, 2)
    images = sample_images()
    rows = []

    def emit(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    if not args.skip_model:
        sh = dict(name="configs[4] inference", K=1000, T=15, V=50000, units=512)
        model, cfg = joint_for(sh, "bf16")
        cfg.IMAGE_MIN_DIM = 800
        kw = dict(return_probabilities=False, decoder="incremental", vocab_math="bf16", postprocess="device")
        turn = {"host": 0, "device": 0}

        def leg(mold):
            def call():
                img = images[turn[mold] % len(images)]
                turn[mold] += 1
                return model.generate_captions([img], **dict(kw, **({} if mold == "host" else dict(mold=mold))))
            return call
        same = True
        for img in images:
            h, d = (model.generate_captions([img], mold=m, **kw)[0] for m in ("host", "device"))
            same = same and all(np.array_equal(h[k], d[k]) for k in h)
        res = timed_alternating_wall([leg("host"), leg("device")], warm, reps)
        for mold, (ems, eall, wms, wall) in zip(("host", "device"), res):
            emit(what="generate_captions_per_image", mold=mold, shape=sh["name"], image="600x800 -> 768x1024 in 1024x1024", event_ms=round(ems, 3),
                 event_spread_ms=round(max(eall) - min(eall), 3), wall_ms=round(wms, 3), wall_spread_ms=round(max(wall) - min(wall), 3),
                 event_runs_ms=eall, wall_runs_ms=wall, timing="median of %d, legs alternating call by call, six images in turn" % reps, **kw)
        (_, _, wh, rh), (_, _, wd, rd) = res
        spread = max(max(rh) - min(rh), max(rd) - min(rd))
        emit(what="mold_device_vs_host", host_wall_ms=round(wh, 3), device_wall_ms=round(wd, 3), gain_ms=round(wh - wd, 3),
             larger_spread_ms=round(spread, 3), device_faster_beyond_spread=bool(wh - wd > spread), results_identical=bool(same))
        del model
        torch.cuda.empty_cache()

    # the resize alone: one image and the six in one call, upload included; then the three launches on an uploaded batch
    for batch in (images[:1], images):
        out = torch.empty((len(batch), 1024, 1024, 3), dtype=torch.uint8, device="cuda:0")
        ms, all_ms = timed(lambda: ops.resize_pad_images(batch, 800, 1024, out=out), 3, 20)
        geo = [utils.resize_geometry(im.shape, 800, 1024, True) for im in batch]
        packed, rec = ops.pack_resize_batch(batch, [(g[0], g[1], g[2][0], g[2][1]) for g in geo])
        dev = torch.from_numpy(packed).to("cuda:0")
        ms_k, all_k = timed(lambda: ops.resize_pad_packed(dev, rec, out=out), 3, 20)
        emit(what="resize_pad_images_alone", images=len(batch), upload_bytes=int(packed.size), pack_upload_launch_ms=round(ms, 4),
             min_ms=min(all_ms), max_ms=max(all_ms), launches_only_ms=round(ms_k, 4), launches_only_min_ms=min(all_k), launches_only_max_ms=max(all_k),
             launches=3, timing="device events around the call, median of 20")

    # the host stage alone on this machine's CPU
    per_image = []
    for img in images:
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            np.stack([utils.resize_image(img, 800, 1024, True)[0]])
            ts.append((time.perf_counter() - t0) * 1e3)
        per_image.append(float(np.median(ts)))
    emit(what="host_stage_alone", stage="utils.resize_image + np.stack, one 600x800 image", cpu_threads=torch.get_num_threads(),
         min_ms=round(min(per_image), 3), max_ms=round(max(per_image), 3), per_image_ms=[round(t, 3) for t in per_image],
         timing="wall clock, median of %d per image" % reps)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
