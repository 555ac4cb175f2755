"""Golden vectors of the caption metrics, produced by RUNNING THE REFERENCE'S OWN SCORERS (not a restatement).

Feeds space-joined decimal token ids to the reference's Bleu(4), Rouge() and Cider() (eval/bleu, eval/rouge, eval/cider: pure
Python) and records their per-record and corpus outputs, plus the integer statistics its BleuScorer and my_lcs hold; then runs the
reference's DenseCaptioningEvaluator.evaluate loop (evaluate_models/test_score_dense_captions.py, its class compiled alone through
the `ast` route of make_reference_vectors.py, with the data getters and score_captions overridden) on synthetic records and scores.
Inputs and recorded results only go to  tests/golden/caption_metrics_reference.npz ; no reference text is stored.

The conditions asserted at the end are what the fixture is FOR (tests/test_caption_metrics_ref.py re-asserts them on the file).

Run:  python tests/golden/make_caption_metric_vectors.py        (needs the reference checkout; the GPU box never runs this)
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_vectors import REF, functions_from  # noqa: E402

REF_ROOT = os.path.dirname(REF)                                              # the checkout that holds eval/ and evaluate_models/
OUT = os.path.join(HERE, "caption_metrics_reference.npz")
VOCAB = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 2 ** 31 - 1], np.int64)       # about ten words; ids 0 and 2^31 - 1 among them
GROUP_SIZES = [1, 5, 20, 41]                                                 # 67 records; CIDEr's corpus is the group
MIN_SCORES = [-1, 0, 0.05, 0.1, 0.15, 0.2, 0.25]


def sentence(rng, n):
    return VOCAB[rng.randint(0, len(VOCAB), size=n)].tolist()


def noisy_copy(rng, s, n):
    """n tokens that keep runs of s (so that 4-grams survive) with a few words replaced."""
    out = (list(s) * (n // max(1, len(s)) + 1))[:n] if s else sentence(rng, n)
    for i in range(len(out)):
        if rng.rand() < 0.12:
            out[i] = int(VOCAB[rng.randint(len(VOCAB))])
    return out


def build_records(rng):
    N = sum(GROUP_SIZES)
    cands, refs = [None] * N, [None] * N
    fixed = {
        0: ([3, 1, 4, 1, 5], [[3, 1, 4, 1, 5, 0], [1, 5]]),                              # the group of one record
        1: ([7, 7, 7, 7], [[7, 7]]),                                                     # a clipped count
        2: ([1, 2, 3, 4, 5], [[1, 2, 3, 4, 5, 6], [1, 2, 3, 4]]),                        # closest-length tie: 6 and 4 around 5
        3: ([], [[1, 2, 3], [4]]),                                                       # empty candidate
        4: ([2 ** 31 - 1, 0, 2 ** 31 - 1], [[], [0, 2 ** 31 - 1, 0, 5]]),                # an empty reference
        5: ([5], [[5], [6, 5]]),
        6: ([1, 2], [[2, 1], [1, 2, 1, 2]]),
        7: ([0, 0, 1], [[0, 1, 0]]),
        8: ([3, 1, 4, 1, 5], [[3, 1, 4, 1, 5, 0]]),                                      # record 0's n-grams again, in another group
        9: ([5, 4, 3, 2, 1], [[3, 4, 5]]),                                               # the my_lcs quirk: 3 where the LCS is 1
    }
    for i in range(N):
        if i in fixed:
            cands[i], refs[i] = fixed[i]
            continue
        nref = (1, 2, 9)[i % 3] if i % 5 else int(rng.randint(1, 6))
        lens = [int(rng.randint(1, 16)) for _ in range(nref)]
        if i == 20:
            lens[0] = 64
        if i == 21:
            lens[0] = 63
        rs = [sentence(rng, n) for n in lens]
        n = {20: 63, 21: 64, 22: 64}.get(i, int(rng.randint(1, 16)))
        if i == 22:
            rs[0] = sentence(rng, 64)
        cands[i] = noisy_copy(rng, rs[0], n) if rng.rand() < 0.7 else sentence(rng, n)
        refs[i] = rs
    return cands, refs


def padded(rng, sentences):
    """int32 [rows, width] with the padding filled by ids that are words elsewhere, and the lengths."""
    lens = np.array([len(s) for s in sentences], np.int32)
    out = VOCAB[rng.randint(0, len(VOCAB), size=(len(sentences), int(lens.max())))].astype(np.int32)
    for i, s in enumerate(sentences):
        out[i, :len(s)] = s
    return out, lens


def text(s):
    return " ".join("%d" % t for t in s)


def main():
    sys.path.insert(0, REF_ROOT)
    from eval.bleu.bleu import Bleu
    from eval.bleu.bleu_scorer import BleuScorer
    from eval.cider.cider import Cider
    from eval.rouge.rouge import Rouge, my_lcs

    rng = np.random.RandomState(20240611)
    cands, refs = build_records(rng)
    N = len(cands)
    group_start = np.concatenate([[0], np.cumsum(GROUP_SIZES)]).astype(np.int32)
    gens = {str(i): [text(c)] for i, c in enumerate(cands)}
    gts = {str(i): [text(r) for r in refs[i]] for i in range(N)}

    with contextlib.redirect_stdout(io.StringIO()):                    # Bleu.compute_score prints its totals
        bleu_corpus, bleu = Bleu(4).compute_score(gts, gens)
    scorer = BleuScorer(n=4)
    for i in range(N):
        scorer += (gens[str(i)][0], gts[str(i)])
    again_corpus, again = scorer.compute_score(option="closest", verbose=0)
    assert again_corpus == bleu_corpus and again == bleu
    stats = np.zeros((N, 12), np.int32)
    for i, comps in enumerate(scorer.ctest):
        stats[i, 0:4], stats[i, 4:8], stats[i, 8] = comps["correct"], comps["guess"], comps["testlen"]
        stats[i, 9] = min((abs(l - comps["testlen"]), l) for l in comps["reflen"])[1]
        stats[i, 10] = max(my_lcs(r.split(" "), gens[str(i)][0].split(" ")) for r in gts[str(i)])
    rouge_mean, rouge = Rouge().compute_score(gts, gens)
    cider = np.zeros(N)
    for g0, g1 in zip(group_start[:-1], group_start[1:]):
        keys = [str(i) for i in range(g0, g1)]
        _, cider[g0:g1] = Cider().compute_score({k: gts[k] for k in keys}, {k: gens[k] for k in keys})

    cand, cand_len = padded(rng, cands)
    flat, ref_len = padded(rng, [r for rs in refs for r in rs])
    ref_start = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int32)
    out = dict(cand=cand, cand_len=cand_len, refs=flat, ref_len=ref_len, ref_start=ref_start, group_start=group_start,
               BLEU=np.array(bleu, np.float64), BLEU_corpus=np.array(bleu_corpus, np.float64), ROUGE=np.array(rouge, np.float64),
               ROUGE_mean=np.float64(rouge_mean), CIDER=cider, CIDER_mean=np.float64(np.mean(cider)), stats=stats)

    # ---- the evaluate loop on synthetic records: reference-less records last, scores away from the thresholds
    E = functions_from(os.path.join(REF_ROOT, "evaluate_models", "test_score_dense_captions.py"), ["DenseCaptioningEvaluator"])
    per_image = [9, 1, 14, 6, 11]
    n = sum(per_image)
    n_without = 7
    ev_ok = rng.randint(0, 2, size=n).astype(np.int32)
    ev_ov = np.round(rng.uniform(0.1, 0.95, size=n), 3)
    ev_ov[::6] = np.array([0.3, 0.4, 0.5, 0.6, 0.7, 0.3, 0.5])[:len(ev_ov[::6])]      # overlaps that sit ON a threshold (>= holds)
    ev_has_ref = (np.arange(n) < n - n_without).astype(np.int32)
    ev_scores = np.round(rng.uniform(-0.04, 0.36, size=n), 4)
    ev_scores[~ev_has_ref.astype(bool)] = np.nan
    gt_counts = np.array([4, 2, 9, 5, 8], np.int32)
    records, at = [], 0
    for c in per_image:
        records.append([{"ok": int(ev_ok[i]), "ov": float(ev_ov[i]), "candidate": "x", "references": [["y"]] if ev_has_ref[i] else []}
                        for i in range(at, at + c)])
        at += c

    class Evaluator(E.DenseCaptioningEvaluator):
        def get_gt_captions(self, image_ids):
            return [None] * len(per_image), [np.zeros((c, 4)) for c in gt_counts], None

        def get_generated_captions(self, num_images, images):
            return None, None, None

        @staticmethod
        def assign_detections_to_ground_truth(*args):
            return records

        def score_captions(self, recs, method):
            return [ev_scores[ev_has_ref.astype(bool)].tolist()]

    dataset = types.SimpleNamespace(num_images=len(per_image), _image_ids=list(range(len(per_image))))
    ev = Evaluator(None, None, "METEOR", dataset, None, None, None, "golden")
    assert ev.min_scores == MIN_SCORES
    result = ev.evaluate()
    out.update(ev_per_image=np.array(per_image, np.int32), ev_ok=ev_ok, ev_ov=ev_ov, ev_has_ref=ev_has_ref, ev_scores=ev_scores,
               ev_npos=np.int64(gt_counts.sum()), ev_map=np.float64(result["map"]), ev_detmap=np.float64(result["detmap"]),
               ev_ap_keys=np.array(list(result["ap_breakdown"])), ev_ap_values=np.array(list(result["ap_breakdown"].values()), np.float64),
               ev_det_keys=np.array(list(result["det_breakdown"])), ev_det_values=np.array(list(result["det_breakdown"].values()), np.float64))

    check_conditions(out)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


def check_conditions(v):
    """What the fixture must contain (the CPU test runs this on the file as well)."""
    cand, cand_len, refs, ref_len, ref_start, group_start, stats = (v[k] for k in ("cand", "cand_len", "refs", "ref_len", "ref_start",
                                                                                   "group_start", "stats"))
    N = cand.shape[0]
    words = set()
    for tok, lens in ((cand, cand_len), (refs, ref_len)):
        for row, n in zip(tok, lens):
            words.update(row[:n].tolist())
    assert 8 <= len(words) <= 12 and 0 in words and 2 ** 31 - 1 in words
    assert (stats[:, 3] > 0).mean() >= 0.25, (stats[:, 3] > 0).mean()
    C = [tuple(cand[i, :cand_len[i]]) for i in range(N)]
    R = [[tuple(refs[j, :ref_len[j]]) for j in range(ref_start[i], ref_start[i + 1])] for i in range(N)]
    assert any(c == (7, 7, 7, 7) and (7, 7) in r for c, r in zip(C, R)) and (stats[:, 0] < stats[:, 4]).any()      # a clipped count
    assert any(len(set(abs(len(r) - len(c)) for r in rs)) < len(set(len(r) for r in rs)) for c, rs in zip(C, R))  # a closest-length tie
    lengths = set(cand_len.tolist()) | set(ref_len.tolist())
    assert {0, 1, 2, 3, 4, 63, 64} <= lengths, sorted(lengths)
    assert {1, 2, 9} <= set(np.diff(ref_start).tolist())
    sizes = np.diff(group_start).tolist()
    assert len(set(sizes)) >= 3 and 1 in sizes
    grams = [set(r[i:i + 4] for rs in R[g0:g1] for r in rs for i in range(len(r) - 3)) for g0, g1 in zip(group_start[:-1], group_start[1:])]
    assert any(grams[a] & grams[b] for a in range(len(grams)) for b in range(a + 1, len(grams)))                    # one n-gram in two groups
    for tok, lens in ((cand, cand_len), (refs, ref_len)):
        pad = tok[np.arange(tok.shape[1])[None, :] >= lens[:, None]]
        assert pad.size and set(pad.tolist()) <= words and len(set(pad.tolist())) > 3                               # padding looks like words
    assert not any(len(c) == 0 and any(len(r) == 0 for r in rs) for c, rs in zip(C, R))
    recorded = np.concatenate([v["ev_scores"][v["ev_has_ref"].astype(bool)]])
    assert np.abs(recorded[:, None] - np.array(MIN_SCORES, np.float64)[None, :]).min() > 1e-6
    assert (v["ev_has_ref"][:-1] >= v["ev_has_ref"][1:]).all() and not v["ev_has_ref"][-1]                          # reference-less records last


if __name__ == "__main__":
    main()
