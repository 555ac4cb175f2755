"""Inputs for the ProposalLayer tests that use the anchors as boxes (plain functions: no GPU, no fixtures).

ops.rpn_proposals takes the anchor array as an input and accepts one level with anchors_per_loc = 1 (heads [B, 1, N, 6], A_total = N).
With the four box logits zero the decode maps anchor a to a box the oracle reproduces with the same float32 operations (expf(0) = 1),
so a case chooses N boxes in pixels (the "anchors") and, per image of the batch, their ranking (through the foreground logit), and the
device's order / keep / proposals must equal O.proposal_layer's bit for bit.

test_proposal_cases.py (CPU) checks that every case has the property it exists for, on the oracle alone; test_gpu_proposals.py
checks the same guards on the device's own scores and then compares the device with the oracle.  The kernel's tuning constants the
guards speak about are read from proposal.hip (kernel_constants), so a retuned kernel fails a guard instead of leaving its case behind."""
import os
import re

import numpy as np

from oracle import np_oracle as O

F32 = np.float32
LANES = 64                                     # candidates per mask word; words per removed-set register of the wave scan


def kernel_constants(repo_root):
    """NMS_G, NMS_ROWS and the largest `words` the wave scan takes, from the source."""
    src = open(os.path.join(repo_root, "image-captioning_amd", "csrc", "proposal.hip")).read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, "proposal.hip: expected one match of %r, found %d" % (pattern, len(m))
        return int(m[0])

    c = {"G": one(r"constexpr\s+int\s+NMS_G\s*=\s*(\d+)\s*;"), "ROWS": one(r"constexpr\s+int\s+NMS_ROWS\s*=\s*(\d+)\s*;"),
         "MAX_WORDS": one(r"if\s*\(\s*words\s*<=\s*(\d+)\s*\)\s*hipLaunchKernelGGL\(\s*nms_scan_wave_kernel\b")}
    c["MAX_K"] = c["MAX_WORDS"] * LANES
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# box families: (boxes_px [N, 4] float32 as (y1, x1, y2, x2), image_hw)
# ------------------------------------------------------------------------------------------------------------------------------

def sparse(n, seed, image=1024):
    """Small boxes (8..40 px) uniformly in the image: nearly everything is kept."""
    rng = np.random.default_rng(seed)
    hw = rng.uniform(8, 40, (n, 2))
    yx = rng.uniform(0, 1, (n, 2)) * (image - hw)
    return np.concatenate([yx, yx + hw], axis=1).astype(F32), (image, image)


def clustered(n, nclu, seed, image=1024):
    """nclu cluster centres; the members differ from their centre by ~6 % of its size in position and ~6 % in log-size."""
    rng = np.random.default_rng(seed)
    chw = rng.uniform(40, 200, (nclu, 2))
    cyx = rng.uniform(0, 1, (nclu, 2)) * image
    which = rng.integers(0, nclu, n)
    hw = chw[which] * np.exp(0.06 * rng.standard_normal((n, 2)))
    yx = cyx[which] + 0.06 * chw[which] * rng.standard_normal((n, 2))
    return np.concatenate([yx - 0.5 * hw, yx + 0.5 * hw], axis=1).astype(F32), (image, image)


def identical(n, image=1024):
    """One box n times: one survivor."""
    return np.tile(np.array([[100.5, 200.25, 300.75, 420.5]], F32), (n, 1)), (image, image)


def zero_area(n, seed, share=1.0, image=1024):
    """sparse with y2 == y1 in a share of the boxes: those never suppress and are never suppressed."""
    b, hw = sparse(n, seed, image)
    flat = np.random.default_rng(seed + 1).uniform(0, 1, n) < share
    b[flat, 2] = b[flat, 0]
    return b, hw


def flipped(n, seed, share=0.5, image=1024):
    """clustered with y1 > y2 and / or x1 > x2 in a share of the boxes (the min / max normalisation of the IoU)."""
    b, hw = clustered(n, max(n // 8, 1), seed, image)
    rng = np.random.default_rng(seed + 1)
    kind = rng.integers(0, 3, n)                                         # 0: y, 1: x, 2: both
    kind[rng.uniform(0, 1, n) >= share] = -1
    fy, fx = (kind == 0) | (kind == 2), (kind == 1) | (kind == 2)
    b[fy] = b[fy][:, [2, 1, 0, 3]]
    b[fx] = b[fx][:, [0, 3, 2, 1]]
    return b, hw


def outside(n, seed, share=0.5, image=1024):
    """clustered with a share of the boxes moved wholly outside the image, one side each: clipped to zero area."""
    b, hw = clustered(n, max(n // 8, 1), seed, image)
    rng = np.random.default_rng(seed + 1)
    side = rng.integers(0, 4, n)
    side[rng.uniform(0, 1, n) >= share] = -1
    h, w = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    far = rng.uniform(1, 50, n).astype(F32)
    for s, (lo, hi, ext, sign) in enumerate([(0, 2, h, -1), (1, 3, w, -1), (0, 2, h, 1), (1, 3, w, 1)]):
        m = side == s
        start = np.where(sign < 0, -far - ext, image + far)[m]           # above / left of 0, or below / right of the image
        b[m, lo], b[m, hi] = start, start + ext[m]
    return b, hw


THRESHOLD_REPS = 10


def threshold_pairs(image=512):
    """Pairs (A, B) in 60 of the 64-pixel cells of a power-of-two image (normalisation and areas exact in float32).  A is the cell; B
    shares A's corner and height and is 32 pixels wide (IoU exactly 0.5), 33, 31, 48 (IoU exactly 0.75), 49 or 47.  Returns the boxes, the
    image size and the list of (index of A, index of B, width of B)."""
    boxes, pairs = [], []
    cell = 0
    for rep in range(THRESHOLD_REPS):
        for wb in (32, 33, 31, 48, 49, 47):
            y, x = 64 * (cell // 8), 64 * (cell % 8)
            cell += 1
            pairs.append((len(boxes), len(boxes) + 1, wb))
            boxes += [[y, x, y + 64, x + 64], [y, x, y + 64, x + wb]]
    return np.array(boxes, F32), (image, image), pairs


# ------------------------------------------------------------------------------------------------------------------------------
# rankings -> heads
# ------------------------------------------------------------------------------------------------------------------------------

def fg_logits(order_ids, ties=()):
    """The foreground logit of every anchor so that anchor order_ids[r] has rank r: evenly spaced in [-3, 3] (neighbouring scores differ by
    >= 1e-5, hundreds of float32 ulps).  ties: ranks r whose anchor gets the logit of rank r - 1 too (an exact score tie; top-k then puts the
    lower anchor index first)."""
    n = len(order_ids)
    by_rank = np.linspace(3.0, -3.0, n) if n > 1 else np.zeros(1)
    for r in ties:
        if 0 < r < n:
            by_rank[r] = by_rank[r - 1]
    out = np.empty(n, F32)
    out[np.asarray(order_ids)] = by_rank.astype(F32)
    return out


def heads_from_logits(logits):
    """[B, N] foreground logits -> the one-level head [B, 1, N, 6]: class logits (0, fg), four zero box logits."""
    logits = np.asarray(logits, F32)
    h = np.zeros(logits.shape[:1] + (1, logits.shape[1], 6), F32)
    h[:, 0, :, 1] = logits
    return h


def host_scores(logits):
    """float32 foreground scores as the CPU test takes them (the GPU test starts from the device's own)."""
    l = np.asarray(logits, np.float64)
    return (1.0 / (1.0 + np.exp(-l))).astype(F32)


def _default_ties(n, k):
    return tuple(r for r in (6, 1001, k) if r < n)                      # rank k ties with rank k - 1: the tie spans the top-k boundary


class Case:
    """anchors [N, 4], image_hw, logits [B, N], k (= pre_nms_limit), count, thr, guards: {name: argument}."""

    def __init__(self, name, anchors, image_hw, logits, k, count, thr, guards):
        self.name, self.anchors, self.image_hw, self.logits = name, np.ascontiguousarray(anchors, F32), image_hw, np.asarray(logits, F32)
        self.k, self.count, self.thr, self.guards = k, count, thr, guards
        self.B, self.N = self.logits.shape
        self.words = (min(k, self.N) + LANES - 1) // LANES

    def heads(self):
        return heads_from_logits(self.logits)


def _ranked(name, boxes_hw, k, count, thr, guards, seed, B=2, extra=300, ties=None):
    """B random rankings of one family's boxes."""
    boxes, hw = boxes_hw
    n = len(boxes)
    assert n == k + extra
    rng = np.random.default_rng(seed)
    t = _default_ties(n, k) if ties is None else ties
    return Case(name, boxes, hw, np.stack([fg_logits(rng.permutation(n), t) for _ in range(B)]), k, count, thr, guards)


def _planted_4097(name, nclu, seed):
    """k = 4097: word 64 holds one candidate, rank 4096.  Image 0 gives that rank to a near-duplicate of its rank-0 box, image 1 to a
    tiny corner box no cluster box overlaps by more than a few per cent."""
    k, extra = 4097, 300
    base, hw = clustered(k - 1 + extra, nclu, seed)
    rng = np.random.default_rng(seed + 10)
    n = len(base)
    order0, order1 = rng.permutation(n), rng.permutation(n)
    dup = base[order0[0]] + F32(0.5)
    lonely = np.array([1, 1, 3, 3], F32)
    anchors = np.concatenate([base, dup[None], lonely[None]])
    i_dup, i_lonely = n, n + 1
    o0 = np.concatenate([order0[:k - 1], [i_dup], order0[k - 1:], [i_lonely]])
    o1 = np.concatenate([order1[:k - 1], [i_lonely], order1[k - 1:], [i_dup]])
    ties = (6, 1001)
    return Case(name, anchors, hw, np.stack([fg_logits(o0, ties), fg_logits(o1, ties)]), k, 2000, 0.7,
                {"wave": None, "kept_lt_count": None, "planted_rank": k - 1})


def _with_identical_image(name, nclu, seed):
    """B = 3: two images rank clustered boxes first, the third ranks k copies of one box first, so it is finished (one survivor, nothing
    alive) while the others still keep boxes in their last groups."""
    k, extra = 6000, 300
    base, hw = clustered(k + extra, nclu, seed)
    same, _ = identical(k)
    anchors = np.concatenate([base, same])
    n = len(base)
    rng = np.random.default_rng(seed + 10)
    orders = [np.concatenate([rng.permutation(n), n + np.arange(k)]) for _ in range(2)]
    orders.append(np.concatenate([n + rng.permutation(k), rng.permutation(n)]))
    ties = (6, 1001)
    return Case(name, anchors, hw, np.stack([fg_logits(o, ties) for o in orders]), k, 2000, 0.7,
                {"wave": None, "kept_lt_count": None, "last_group": (0, 1), "one_kept": (2,)})


def _threshold_case(name, thr):
    boxes, hw, pairs = threshold_pairs()
    n = len(boxes)
    a_first = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])             # every A, then every B: most B one chunk after their A
    interleaved = np.arange(n)                                                     # A, B, A, B: both in one chunk
    return Case(name, boxes, hw, np.stack([fg_logits(a_first), fg_logits(interleaved)]), n, n, thr,
                {"wave": None, "threshold_pairs": pairs})


def _builders():
    far = {"wave": None, "far_suppress": None, "big_chunk": None}
    b = {}

    def add(name, fn):
        assert name not in b
        b[name] = fn

    add("sparse_6000", lambda: _ranked("sparse_6000", sparse(6300, 1), 6000, 2000, 0.7,
                                       {"wave": None, "count_reached_early": None, "count_reached_mid_chunk": None, "big_chunk": None}, 101))
    add("clustered300_6000", lambda: _ranked("clustered300_6000", clustered(6300, 300, 2), 6000, 2000, 0.7,
                                             dict(far, kept_lt_count=None, last_group=(0, 1)), 102))
    add("clustered1500_6000", lambda: _ranked("clustered1500_6000", clustered(6300, 1500, 3), 6000, 2000, 0.7,
                                              dict(far, count_reached_early=None, last_kept_beyond=64 * LANES), 103))
    add("clustered300_6000_thr03", lambda: _ranked("clustered300_6000_thr03", clustered(6300, 300, 4), 6000, 2000, 0.3,
                                                   dict(far, kept_lt_count=None), 104))
    add("clustered40_8192", lambda: _ranked("clustered40_8192", clustered(8492, 40, 5), 8192, 2000, 0.7,
                                            dict(far, kept_lt_count=None, last_group=(0, 1), max_words=None), 105, ties=(6, 1001, 8192)))
    add("clustered40_8193", lambda: _ranked("clustered40_8193", clustered(8492, 40, 5), 8193, 2000, 0.7,
                                            {"serial": None, "kept_lt_count": None}, 105, extra=299, ties=(6, 1001, 8192)))      # the boxes, rankings and ties of clustered40_8192
    add("sparse_8193", lambda: _ranked("sparse_8193", sparse(8493, 6), 8193, 300, 0.7, {"serial": None, "count_reached_early": None}, 106))
    add("clustered500_12000", lambda: _ranked("clustered500_12000", clustered(12300, 500, 7), 12000, 2000, 0.7,
                                              {"serial": None, "kept_lt_count": None, "last_kept_beyond": 128 * LANES}, 107))
    add("sparse_4096", lambda: _ranked("sparse_4096", sparse(4396, 8), 4096, 1000, 0.7, {"wave": None, "count_reached_early": None}, 108))
    add("sparse_4097", lambda: _ranked("sparse_4097", sparse(4397, 9), 4097, 1000, 0.7, {"wave": None, "count_reached_early": None}, 109))
    add("clustered100_4097", lambda: _planted_4097("clustered100_4097", 100, 10))
    add("clustered300_4097", lambda: _planted_4097("clustered300_4097", 300, 11))
    add("sparse_512", lambda: _ranked("sparse_512", sparse(812, 12), 512, 512, 0.7, {"wave": None, "one_group": None, "all_kept": None}, 112))
    add("sparse_513", lambda: _ranked("sparse_513", sparse(813, 13), 513, 100, 0.7, {"wave": None, "count_reached_early": None}, 113))
    add("sparse_64", lambda: _ranked("sparse_64", sparse(364, 14), 64, 64, 0.7, {"wave": None, "all_kept": None}, 114))
    add("sparse_63", lambda: _ranked("sparse_63", sparse(363, 15), 63, 10, 0.7, {"wave": None, "count_reached_mid_chunk": None}, 115))
    add("sparse_1", lambda: _ranked("sparse_1", sparse(301, 16), 1, 5, 0.7, {"wave": None, "all_kept": None, "count_gt_k": None}, 116))
    add("identical_6000", lambda: _ranked("identical_6000", identical(6300), 6000, 2000, 0.7, {"wave": None, "one_kept": (0, 1)}, 117))
    add("zero_area_6000", lambda: _ranked("zero_area_6000", zero_area(6300, 18), 6000, 2000, 0.7,
                                          {"wave": None, "first_count_kept": None}, 118))
    add("flipped_6000", lambda: _ranked("flipped_6000", flipped(6300, 19), 6000, 2000, 0.7,
                                        {"wave": None, "far_suppress": None, "flipped_kept_and_suppressed": None}, 119))
    add("outside_6000", lambda: _ranked("outside_6000", outside(6300, 20), 6000, 2000, 0.7,
                                        {"wave": None, "zero_area_candidates": None}, 120))
    # The `area <= 0` early-out of the IoU cannot be seen at a threshold >= 0: without it a zero-area box gives inter = 0, and 0 / area or
    # 0 / 0 (NaN) never exceeds the threshold.  A negative threshold (which tf.image.non_max_suppression would refuse) shows it: every
    # box of positive area suppresses every later one, whatever their overlap, and the zero-area boxes are exempt on both sides.
    add("zero_area_negative_thr", lambda: _ranked("zero_area_negative_thr", zero_area(1324, 21, share=0.5), 1024, 600, -0.5,
                                                  {"wave": None, "one_positive_area_kept": None}, 121))
    add("clustered300_6000_B3_identical", lambda: _with_identical_image("clustered300_6000_B3_identical", 300, 22))
    add("threshold_050", lambda: _threshold_case("threshold_050", 0.5))
    add("threshold_075", lambda: _threshold_case("threshold_075", 0.75))
    return b


BUILDERS = _builders()
CASE_NAMES = list(BUILDERS)


def build(name):
    return BUILDERS[name]()


# ------------------------------------------------------------------------------------------------------------------------------
# the oracle's answer and the guards on it
# ------------------------------------------------------------------------------------------------------------------------------

def reference(case, scores):
    """Per image: {"order", "keep" (ranks), "proposals" [count, 4], "boxes" [k, 4] (every candidate, normalised, in rank order)}."""
    refs = []
    zero = np.zeros((case.N, 4), F32)
    h, w = case.image_hw
    for b in range(case.B):
        want, ix, kp = O.proposal_layer(scores[b], zero, case.anchors, case.image_hw, case.count, case.thr, pre_nms_limit=case.k)
        nb = (O.clip_boxes_f32(O.apply_box_deltas_f32(case.anchors[ix], zero[ix]), (0, 0, h, w)) / np.array([h, w, h, w], F32)).astype(F32)
        np.testing.assert_array_equal(nb[kp], want[:len(kp)])
        refs.append({"order": ix, "keep": kp, "proposals": want, "boxes": nb})
    return refs


def iou_f32(a, b):
    """IoU of box a with every box of b, float32 operation by operation as O.nms_tf (0 where either area is not positive)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32).reshape(-1, 4)
    ay0, ay1, ax0, ax1 = min(a[0], a[2]), max(a[0], a[2]), min(a[1], a[3]), max(a[1], a[3])
    by0, by1 = np.minimum(b[:, 0], b[:, 2]), np.maximum(b[:, 0], b[:, 2])
    bx0, bx1 = np.minimum(b[:, 1], b[:, 3]), np.maximum(b[:, 1], b[:, 3])
    aa, ab = (ay1 - ay0) * (ax1 - ax0), (by1 - by0) * (bx1 - bx0)
    ih = np.maximum(np.minimum(ay1, by1) - np.maximum(ay0, by0), F32(0))
    iw = np.maximum(np.minimum(ax1, bx1) - np.maximum(ax0, bx0), F32(0))
    inter = ih * iw
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (aa + ab - inter)
    return np.where((aa > 0) & (ab > 0), iou, F32(0)).astype(F32)


def _areas(nb):
    return (np.maximum(nb[:, 0], nb[:, 2]) - np.minimum(nb[:, 0], nb[:, 2])) * (np.maximum(nb[:, 1], nb[:, 3]) - np.minimum(nb[:, 1], nb[:, 3]))


def check_guards(case, refs, consts):
    """Assert, on the oracle's result alone, the property every case exists for.  Returns a dict of figures for the log."""
    G, ROWS, MAXW = consts["G"], consts["ROWS"], consts["MAX_WORDS"]
    k, words, thr = min(case.k, case.N), case.words, F32(case.thr)
    g = case.guards
    known = {"wave", "serial", "max_words", "one_group", "kept_lt_count", "count_reached_early", "count_reached_mid_chunk", "big_chunk", "far_suppress",
             "last_group", "last_kept_beyond", "all_kept", "count_gt_k", "one_kept", "first_count_kept", "flipped_kept_and_suppressed",
             "zero_area_candidates", "one_positive_area_kept", "planted_rank", "threshold_pairs"}
    assert set(g) <= known, set(g) - known
    assert ("wave" in g) != ("serial" in g)
    if "wave" in g:
        assert words <= MAXW, "%s: %d words no longer reach the wave scan" % (case.name, words)
    if "serial" in g:
        assert words > MAXW, "%s: %d words no longer reach the serial scan" % (case.name, words)
    if "max_words" in g:
        assert words == MAXW
    if "one_group" in g:
        assert words == G
    if "count_gt_k" in g:
        assert case.count > k
    figures = []
    for b, r in enumerate(refs):
        kp, nb, n = r["keep"], r["boxes"], len(r["keep"])
        assert len(nb) == k and n >= 1
        per_chunk = np.bincount(kp // LANES, minlength=words)
        last = int(kp[-1])
        figures.append({"kept": n, "last": last, "chunks_over_rows": int((per_chunk > ROWS).sum())})
        if "kept_lt_count" in g and b in (g["kept_lt_count"] or range(case.B)):
            assert n < case.count, (case.name, b, n)
        if "count_reached_early" in g:
            assert n == case.count and last < LANES * (words - 1), (case.name, b, n, last)
        if "count_reached_mid_chunk" in g:
            # candidates after the last kept one in its chunk that nothing kept suppresses: the scan has to stop for `count`, not for lack of candidates
            assert n == case.count, (case.name, b, n)
            rest = np.arange(last + 1, min(k, (last // LANES + 1) * LANES))
            assert any(not np.any(iou_f32(nb[i], nb[kp]) > thr) for i in rest), (case.name, b, last)
        if "big_chunk" in g:
            assert per_chunk.max() > ROWS, (case.name, b, int(per_chunk.max()))
        if "far_suppress" in g:
            # a box kept in the first group suppresses a candidate in a word of the second removed-set register
            assert k > LANES * LANES
            early = kp[kp < LANES * G]
            assert any(np.any(iou_f32(nb[i], nb[LANES * LANES:]) > thr) for i in early), (case.name, b)
        if "last_group" in g and b in g["last_group"]:
            assert last >= LANES * G * ((words - 1) // G), (case.name, b, last)
        if "last_kept_beyond" in g:
            assert last >= g["last_kept_beyond"], (case.name, b, last)
        if "all_kept" in g:
            assert n == min(k, case.count) == k, (case.name, b, n)
        if "one_kept" in g and b in g["one_kept"]:
            assert n == 1 and case.count > 1, (case.name, b, n)
        if "first_count_kept" in g:
            assert np.all(_areas(nb) == 0) and np.array_equal(kp, np.arange(case.count)), (case.name, b)
        if "flipped_kept_and_suppressed" in g:
            fl = (nb[:, 0] > nb[:, 2]) | (nb[:, 1] > nb[:, 3])
            dead = np.ones(k, bool)
            dead[kp] = False
            dead[last + 1:] = False
            assert fl[kp].sum() > 50 and (fl & dead).sum() > 50, (case.name, b)
        if "zero_area_candidates" in g:
            flat = _areas(nb) == 0
            seen = np.flatnonzero(flat)
            seen = seen[seen <= last]
            assert len(seen) > 300 and np.all(np.isin(seen, kp)) and (~flat[kp]).sum() > 300 and n < (last + 1), (case.name, b)
        if "one_positive_area_kept" in g:
            assert case.thr < 0
            flat = _areas(nb) == 0
            assert (~flat[kp]).sum() == 1 and flat[kp].sum() > 100 and n < case.count, (case.name, b)
            assert np.array_equal(kp[flat[kp]], np.flatnonzero(flat)[:n - 1])
        if "planted_rank" in g:
            p = g["planted_rank"]
            assert p == k - 1 == LANES * LANES and words == LANES + 1
            if b == 0:
                assert p not in kp and kp[0] == 0 and iou_f32(nb[0], nb[p])[0] > thr, (case.name, "the near-duplicate is not suppressed")
            else:
                assert last == p, (case.name, "the corner box is not the last survivor")
        if "threshold_pairs" in g:
            anchor_rank = np.empty(case.N, np.int64)
            anchor_rank[r["order"]] = np.arange(k)
            exact = 0
            for ia, ib, wb in g["threshold_pairs"]:
                ra, rb = anchor_rank[ia], anchor_rank[ib]
                iou = iou_f32(nb[ra], nb[rb])[0]
                assert ra < rb and ra in kp and iou == F32(wb / 64.0)
                exact += int(iou == thr)
                assert (rb in kp) == (not iou > thr), (case.name, b, wb)
            assert exact == THRESHOLD_REPS, (case.name, b, exact)
    return figures


# ------------------------------------------------------------------------------------------------------------------------------
# the real pyramid at the production shape
# ------------------------------------------------------------------------------------------------------------------------------

PYRAMID = {"S": 512, "k": 6000, "count": 2000, "thr": 0.7, "strides": [4, 8, 16, 32, 64], "scales": (32, 64, 128, 256, 512), "ratios": [0.5, 1, 2]}


def pyramid_inputs(seed, B=2, level_bias=3.0):
    """Random five-level heads [B, h, w, 18] and the pyramid anchors at 512 x 512.  With plain random heads the 2000th survivor has a rank
    near 2100; the foreground logit of level l is raised by level_bias * l, so the coarse levels (whose anchors overlap heavily) rank first
    and the scan has to go on into the second half of the candidates.  Returns (heads, anchors, class logits [B, A, 2], box logits
    [B, A, 4])."""
    rng = np.random.default_rng(seed)
    S = PYRAMID["S"]
    shapes = [[S // s, S // s] for s in PYRAMID["strides"]]
    heads = []
    for level, (h, w) in enumerate(shapes):
        hd = rng.standard_normal((B, h, w, 18)).astype(F32)
        hd[..., 6:] *= F32(0.1)
        hd[..., 1:6:2] += F32(level_bias * level)
        heads.append(hd)
    anchors = O.generate_pyramid_anchors(PYRAMID["scales"], PYRAMID["ratios"], shapes, PYRAMID["strides"], 1).astype(F32)
    cls = np.concatenate([h[..., :6].reshape(B, -1, 2) for h in heads], axis=1)
    box = np.concatenate([h[..., 6:].reshape(B, -1, 4) for h in heads], axis=1)
    return heads, anchors, cls, box


def pyramid_reference(scores, box, anchors):
    """[(proposals, order, keep)] per image; asserts the guard: `count` boxes are kept and the last of them has a rank >= 4096."""
    S, out = PYRAMID["S"], []
    for b in range(len(scores)):
        want, ix, kp = O.proposal_layer(scores[b], box[b], anchors, (S, S), PYRAMID["count"], PYRAMID["thr"], pre_nms_limit=PYRAMID["k"])
        assert len(kp) == PYRAMID["count"] and LANES * LANES <= kp[-1] < LANES * ((PYRAMID["k"] + LANES - 1) // LANES - 1), (b, len(kp), kp[-1])
        out.append((want, ix, kp))
    return out
