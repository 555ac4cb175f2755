"""Caption metrics: the device path against the package's host path on the same machine.

Shapes: 1000 records x at most 15 tokens x {1, 5} references, as 1 group and as 16 groups; and 100 000 records (5 references) in one
group.  Ids come from a 1000-word vocabulary with candidates that are noisy copies of their first reference (so that n-grams match).

Per shape:
  host_s        caption_metrics.score(backend="host") on the CPU of the machine this runs on (wall clock; once at 100 000 records)
  device_s      caption_metrics.score(backend="device") from tensors already on the device to results on the device, ending in a
                device synchronise (host clock: the CIDEr path synchronises for torch.unique's sizes anyway); a warm-up call, then the
                median of --repeats calls and their spread
  kernels_ms    device events around ops.caption_metrics and ops.caption_cider alone (the two launches, their tables built before)
  tables_ms     caption_metrics.cider_gram_tables alone (the torch.unique plumbing that numbers the n-grams)
  agree         the device results against the host's at the tests' tolerances (statistics exact, rtol 1e-9)
The reference's own scorers are not on the GPU machine; REFERENCE_BUILD_MACHINE_S quotes what they took on the build machine's CPU
for 1000 records x 15 tokens x 1-5 references (synthetic id strings), for context only: it is another machine's CPU.

    python tools/metrics_bench.py --out profiles/metrics_bench.json
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

REFERENCE_BUILD_MACHINE_S = {"Bleu(4)": 0.16, "Cider()": 0.46, "Rouge()": 0.07, "records": 1000, "where": "build machine CPU, not the GPU machine"}


def make_batch(cm, seed, N, nref, groups, vocab=1000, max_len=15):
    rng = np.random.RandomState(seed)
    ref_counts = np.full(N, nref) if nref == 1 else rng.randint(1, nref + 1, size=N)
    M = int(ref_counts.sum())
    ref_len = rng.randint(3, max_len + 1, size=M).astype(np.int32)
    refs = rng.randint(0, vocab, size=(M, max_len)).astype(np.int32)
    ref_start = np.concatenate([[0], np.cumsum(ref_counts)]).astype(np.int32)
    cand = refs[ref_start[:-1]].copy()
    noise = rng.rand(N, max_len) < 0.2
    cand[noise] = rng.randint(0, vocab, size=int(noise.sum()))
    cand_len = np.clip(ref_len[ref_start[:-1]] + rng.randint(-2, 3, size=N), 1, max_len).astype(np.int32)
    group_start = np.linspace(0, N, groups + 1).astype(np.int32)
    return cm.CaptionBatch(cand, cand_len, refs, ref_len, ref_start, group_start)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--big", type=int, default=100000, help="records of the large shape (0: skip it)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "metrics_bench needs the GPU: there is no CPU stand-in for the device path"
    from image_captioning_amd import caption_metrics as cm, ops

    shapes = [(1000, 1, 1), (1000, 1, 16), (1000, 5, 1), (1000, 5, 16)] + ([(args.big, 5, 1)] if args.big else [])
    rows = []
    for N, nref, groups in shapes:
        batch = make_batch(cm, N + nref + groups, N, nref, groups)
        t0 = time.perf_counter()
        host = cm.score(batch)
        host_s = time.perf_counter() - t0
        if N <= 1000:
            again = []
            for _ in range(2):
                t0 = time.perf_counter()
                cm.score(batch)
                again.append(time.perf_counter() - t0)
            host_s = float(np.median([host_s] + again))
        dev_batch = cm.CaptionBatch(*(torch.from_numpy(a).cuda() for a in batch.host()))
        t = [getattr(dev_batch, f) for f in cm.CaptionBatch.FIELDS]
        res = cm.score(dev_batch, backend="device")                      # warm-up: code objects, the workspace of torch.unique
        torch.cuda.synchronize()
        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            res = cm.score(dev_batch, backend="device")
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        tables_ms, kern_ms = [], []
        for _ in range(args.repeats):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            grams, df, df_off, group_n = cm.cider_gram_tables(t)
            e[1].record()
            lens = torch.cat([t[1], t[3]])
            ops.caption_metrics(*t[:5])
            ops.caption_cider(grams, lens, t[4], df, df_off, group_n)
            e[2].record()
            torch.cuda.synchronize()
            tables_ms.append(e[0].elapsed_time(e[1]))
            kern_ms.append(e[1].elapsed_time(e[2]))
        agree = bool((res["stats"].cpu().numpy() == host["stats"]).all())
        for m in ("BLEU", "ROUGE"):
            agree = agree and bool(np.allclose(res[m].cpu().numpy(), host[m], rtol=1e-9, atol=0))
        agree = agree and bool(np.allclose(res["CIDER"].cpu().numpy(), host["CIDER"], rtol=1e-9, atol=1e-12))
        row = dict(records=N, max_refs=nref, groups=groups, references=int(batch.refs.shape[0]), host_s=round(host_s, 4),
                   device_s=round(float(np.median(times)), 5), device_s_min_max=[round(min(times), 5), round(max(times), 5)],
                   tables_ms=round(float(np.median(tables_ms)), 3), kernels_ms=round(float(np.median(kern_ms)), 3),
                   speedup=round(host_s / float(np.median(times)), 1), agree=agree,
                   cider_max_rel_err=float(np.max(np.abs(res["CIDER"].cpu().numpy() - host["CIDER"]) / np.maximum(np.abs(host["CIDER"]), 1e-3))))
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "reference_scorers_s": REFERENCE_BUILD_MACHINE_S,
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
