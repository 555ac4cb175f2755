"""Inputs for test_gpu_roi_rpn_edges.py: the RPN loss kernel in the train step's call form, DetectionTargetLayer at odd counts, ties and
thresholds, RoIAlign off the square 7 x 7 x 256 path (plain functions: seeded NumPy and small literal boxes, no GPU, no fixtures).

Every case states what it holds -- which 256-wide pass of the one-block loop a positive lies in, that two IoUs are one float32 value,
that a sample lands on a pixel -- and test_roi_rpn_cases.py (CPU) proves the statements on the oracle alone, so a case that has lost its
property is red wherever the suite runs.  philox2x32 and dt_case moved here from test_gpu_kernels.py, which imports them."""
import numpy as np

from oracle import np_oracle as O

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------------
# RPN losses (rpn_loss_grad_kernel): five levels of a 64 x 64 image, 1023 anchors per image, the batched selection of the train step
# ------------------------------------------------------------------------------------------------------------------------------
RPN_A, RPN_STRIDE, RPN_PASS = 3, 20, 256                     # anchors per location, head columns, selected anchors per pass of the block
RPN_SHAPES = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
RPN_SIZES = [h * w * RPN_A for h, w in RPN_SHAPES]           # anchors per image of each level
RPN_ANCHORS = sum(RPN_SIZES)                                 # 1023
RPN_SEL_CAPACITY, RPN_TARGET_CAPACITY = 768, 384


class RpnCase(object):
    """heads: five float32 [B, h, w, 20]; match int32 [B, 1023] (1 positive, -1 negative, 0 neutral); target float32 [n_pos, 4], the
    positives' rows packed image-major in anchor order."""

    def __init__(self, heads, match, target):
        self.heads, self.match, self.target = heads, match, target
        self.B = match.shape[0]
        sel = [self._image_selection(b) for b in range(self.B)]
        self.lvl, self.idx, self.mt = (np.concatenate([s[k] for s in sel]).astype(np.int32) for k in range(3))
        self.n_sel, self.n_pos = int(self.mt.size), int((self.mt == 1).sum())
        assert target.shape == (self.n_pos, 4) and target.dtype == F32

    def _image_selection(self, b):
        """dense_model._rpn_selection: the non-neutral anchors in anchor order, image b's anchor i of a level at b * h * w * A + i."""
        m = self.match[b]
        idx = np.nonzero(m != 0)[0]
        bounds = np.cumsum([0] + RPN_SIZES)
        level = np.searchsorted(bounds, idx, side="right") - 1
        return level, idx - bounds[level] + b * np.asarray(RPN_SIZES)[level], m[idx]

    def flat(self):
        """(match, logits [B * 1023, 2], bbox [B * 1023, 4]) image-major: what the reference's batched loss graphs gather over."""
        A = RPN_A
        logits = np.concatenate([h[b, :, :, :2 * A].reshape(-1, 2) for b in range(self.B) for h in self.heads])
        bbox = np.concatenate([h[b, :, :, 2 * A:6 * A].reshape(-1, 4) for b in range(self.B) for h in self.heads])
        return self.match.reshape(-1), logits, bbox

    def oracle(self):
        """(class loss, bbox loss, d logits [B, 1023, 2], d bbox [B, 1023, 4]) in float64."""
        m, logits, bbox = self.flat()
        l_cls, d_cls = O.rpn_class_loss(m, logits)
        l_box, d_box = O.rpn_bbox_loss(self.target, m, bbox)
        return l_cls, l_box, d_cls.reshape(self.B, RPN_ANCHORS, 2), d_box.reshape(self.B, RPN_ANCHORS, 4)

    def pass_positives(self):
        """Positives among the selected anchors [0, 256), [256, 512), ... : the passes of the kernel's one-block loop."""
        return [int((self.mt[i:i + RPN_PASS] == 1).sum()) for i in range(0, self.n_sel, RPN_PASS)]

    def padded(self):
        """The selection in buffers of fixed capacity (768 anchors, 384 target rows).  The slack anchors are valid, in range and not
        otherwise selected, their match is 1 and the slack target rows are 1e3: a kernel that read past the device counts would return
        other finite numbers.  Returns (lvl, idx, mt, target, slack) with slack = the (level, index) pairs of the slack anchors."""
        used = set(zip(self.lvl.tolist(), self.idx.tolist()))
        rng = np.random.default_rng(41)
        slack = []
        while len(slack) < RPN_SEL_CAPACITY - self.n_sel:
            l = int(rng.integers(0, len(RPN_SIZES)))
            i = int(rng.integers(0, self.B * RPN_SIZES[l]))
            if (l, i) not in used:
                used.add((l, i))
                slack.append((l, i))
        sl = np.array(slack, np.int32)
        lvl, idx = np.concatenate([self.lvl, sl[:, 0]]), np.concatenate([self.idx, sl[:, 1]])
        mt = np.concatenate([self.mt, np.ones(len(slack), np.int32)])
        target = np.full((RPN_TARGET_CAPACITY, 4), 1e3, F32)
        target[:self.n_pos] = self.target
        return lvl.astype(np.int32), idx.astype(np.int32), mt.astype(np.int32), target, slack


RPN_SELECTED, RPN_POSITIVES = (230, 256, 114), (97, 61, 38)


def rpn_three_passes():
    """B = 3 with 230, 256 and 114 selected anchors (600: three passes of 256, the last ragged) of which 97, 61 and 38 are positives;
    the first and the last anchor of the first and of the last image take part, anchor 0 of image 0 and anchor 1022 of image 2 as
    positives."""
    rng = np.random.default_rng(600)
    B = len(RPN_SELECTED)
    heads = [rng.standard_normal((B, h, w, RPN_STRIDE)).astype(F32) for h, w in RPN_SHAPES]
    match = np.zeros((B, RPN_ANCHORS), np.int32)
    for b, (n, p) in enumerate(zip(RPN_SELECTED, RPN_POSITIVES)):
        ends = b in (0, B - 1)                               # both end anchors selected, one of them a positive
        rest = rng.permutation(np.arange(1, RPN_ANCHORS - 1))[:n - 2 * ends]
        match[b, rest] = -1
        match[b, rest[:p - ends]] = 1
        if ends:
            match[b, 0], match[b, RPN_ANCHORS - 1] = (1, -1) if b == 0 else (-1, 1)
    target = (1.5 * rng.standard_normal((sum(RPN_POSITIVES), 4))).astype(F32)
    return RpnCase(heads, match, target)


def rpn_all_negative():
    """The three-pass selection with every match -1: no positive, no target row."""
    c = rpn_three_passes()
    return RpnCase(c.heads, -np.abs(c.match), np.zeros((0, 4), F32))


KNEE_TARGETS = np.array([[1.0, -1.0, 1.0 - 2.0 ** -24, -(1.0 - 2.0 ** -24)],
                         [1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23), 0.5, -0.5],
                         [0.0, 3.0, -3.0, 0.0]], np.float64)
KNEE_ANCHORS = (0, 500, RPN_ANCHORS - 1)


def rpn_knee():
    """One image, three positives whose bbox outputs are 0, so that diff = target exactly: |diff| on, one ulp below and one ulp above
    the smooth-L1 knee, inside (0.5, 0), far outside (3), each with both signs; 40 negatives beside them."""
    rng = np.random.default_rng(77)
    heads = [rng.standard_normal((1, h, w, RPN_STRIDE)).astype(F32) for h, w in RPN_SHAPES]
    match = np.zeros((1, RPN_ANCHORS), np.int32)
    match[0, rng.permutation(np.arange(1, RPN_ANCHORS - 1))[:40]] = -1
    match[0, list(KNEE_ANCHORS)] = 1
    bounds = np.cumsum([0] + RPN_SIZES)
    for a in KNEE_ANCHORS:
        l = int(np.searchsorted(bounds, a, side="right") - 1)
        cell, k = divmod(a - bounds[l], RPN_A)
        heads[l].reshape(-1, RPN_STRIDE)[cell, 2 * RPN_A + 4 * k:2 * RPN_A + 4 * k + 4] = 0
    return RpnCase(heads, match, KNEE_TARGETS.astype(F32))


# ------------------------------------------------------------------------------------------------------------------------------
# DetectionTargetLayer (detection_targets_kernel)
# ------------------------------------------------------------------------------------------------------------------------------

def philox2x32(c0, c1, key):
    """NumPy restatement of the library's counter-based generator (csrc/dcap_internal.h philox2x32: Philox-2x32-10)."""
    c0 = np.asarray(c0, np.uint64) & 0xFFFFFFFF
    c1 = np.full_like(c0, int(c1) & 0xFFFFFFFF)
    key = int(key) & 0xFFFFFFFF
    for _ in range(10):
        p = (np.uint64(0xD256D193) * c0) & np.uint64(0xFFFFFFFFFFFFFFFF)
        hi, lo = p >> np.uint64(32), p & np.uint64(0xFFFFFFFF)
        c0 = (hi ^ np.uint64(key) ^ c1) & np.uint64(0xFFFFFFFF)
        c1 = lo
        key = (key + 0x9E3779B9) & 0xFFFFFFFF
    return c0.astype(np.uint32)


def dt_case(seed, n_props, n_gt, pad_props, pad_gt, T=6, jitter=0.08):
    """Proposals scattered around GT boxes (some close: IoU above 0.5, some far), zero padding rows in both lists, one all-zero
    proposal in the middle of the list and a degenerate (zero-area) proposal."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((n_gt + pad_gt, 4), np.float32)
    y1, x1 = rng.uniform(0, 0.6, n_gt), rng.uniform(0, 0.6, n_gt)
    gt[:n_gt] = np.stack([y1, x1, y1 + rng.uniform(0.1, 0.4, n_gt), x1 + rng.uniform(0.1, 0.4, n_gt)], 1)
    caps = np.zeros((n_gt + pad_gt, T), np.int32)
    caps[:n_gt] = rng.integers(1, 1000, (n_gt, T))
    props = np.zeros((n_props + pad_props, 4), np.float32)
    src = rng.integers(0, max(n_gt, 1), n_props)
    noise = rng.normal(0, jitter, (n_props, 4)) * (rng.random((n_props, 1)) < 0.6)
    base = gt[src] if n_gt else rng.uniform(0.1, 0.5, (n_props, 4)).astype(np.float32)
    props[:n_props] = np.clip(base + noise, 0, 1)
    far = rng.random(n_props) < 0.3
    fy, fx = rng.uniform(0, 0.9, n_props), rng.uniform(0, 0.9, n_props)
    props[:n_props][far] = np.stack([fy, fx, fy + 0.05, fx + 0.05], 1)[far]
    if n_props > 10:
        props[5] = 0                                         # a zero row that is NOT trailing padding: later indices shift when compacted
        props[7] = [0.3, 0.3, 0.3, 0.6]                      # zero area, non-zero row
    if pad_gt and n_gt > 2:
        gt[[1, n_gt]] = gt[[n_gt, 1]]                        # a zero GT row in the middle
        caps[[1, n_gt]] = caps[[n_gt, 1]]
    return props.astype(np.float32), gt, caps


class DtCase(object):
    def __init__(self, props, gt, caps, n_rois, ratio):
        self.props, self.gt, self.caps = np.asarray(props, F32), np.asarray(gt, F32), np.asarray(caps, np.int32)
        self.n_rois, self.ratio = n_rois, ratio

    @property
    def nonzero_rows(self):
        return int((np.abs(self.props).sum(1) > 0).sum())

    def best_iou(self):
        """Best float32 IoU of every non-zero proposal over the non-zero GT boxes (NaN where a pair is 0 / 0)."""
        p, g = self.props[np.abs(self.props).sum(1) > 0], self.gt[np.abs(self.gt).sum(1) > 0]
        return O.overlaps_f32(p, g).max(axis=1)

    def oracle(self, shuffle=None):
        return O.detection_targets(self.props, self.caps, self.gt, self.n_rois, self.ratio, shuffle)


# name -> (seed, proposals, GT boxes, zero proposal rows appended, zero GT rows, parity of the non-zero proposal rows); every N is odd
DT_ODD = {"n1": (13, 1, 2, 0, 0, 1), "n3": (12, 3, 2, 0, 1, 1), "n255": (13, 250, 9, 5, 3, 1),
          "n257_odd_rows": (14, 256, 12, 1, 0, 1),          # 256 drawn rows less the zero row in the middle
          "n257_even_rows": (15, 257, 12, 0, 4, 0),         # the second workgroup ranks the one proposal 256
          "n1023": (16, 1000, 30, 23, 2, 1), "n4095": (17, 4000, 40, 95, 8, 1)}


def dt_odd(name):
    seed, n_props, n_gt, pad_p, pad_g, _ = DT_ODD[name]
    return DtCase(*dt_case(seed, n_props, n_gt, pad_p, pad_g), n_rois=200, ratio=0.33)


def _caps(n, T=6):
    return (np.arange(n)[:, None] * 10 + np.arange(T)[None, :] + 1).astype(np.int32)        # every row different, no zero


TIE_PROPOSAL = (0.25, 0.25, 0.75, 0.75)
TIE_GT = ((0.25, 0.125, 0.75, 0.75), (0.25, 0.25, 0.75, 0.875))        # both 0.25 / 0.3125 = 0.8 against TIE_PROPOSAL


def dt_first_maximum(kind, swapped):
    """tf.argmax takes the FIRST maximum.  "identical": GT rows 1 and 3 are one box with two captions, and five proposals equal it;
    "equal_iou": GT rows 1 and 3 are two boxes with one float32 IoU (0.8) against three proposals.  Row 0 is another box, row 2 a zero
    row; swapped exchanges rows 1 and 3 (boxes and captions).  Returns (case, tied proposals, the two tied GT rows)."""
    other = (0.05, 0.6, 0.2, 0.9)
    if kind == "identical":
        a = (0.3, 0.1, 0.8, 0.55)
        gt = np.array([other, a, (0, 0, 0, 0), a], F32)
        tied = [0, 2, 3, 5, 8]
        props = np.array([a, (0.31, 0.1, 0.8, 0.55), a, a, other, a, (0.6, 0.6, 0.7, 0.7), (0, 0, 0, 0), a], F32)
    else:
        gt = np.array([other, TIE_GT[0], (0, 0, 0, 0), TIE_GT[1]], F32)
        tied = [1, 2, 6]
        props = np.array([other, TIE_PROPOSAL, TIE_PROPOSAL, (0.6, 0.6, 0.7, 0.7), TIE_GT[0], TIE_GT[1], TIE_PROPOSAL], F32)
    caps = _caps(4)
    if swapped:
        gt[[1, 3]], caps[[1, 3]] = gt[[3, 1]], caps[[3, 1]]
    return DtCase(props, gt, caps, n_rois=16, ratio=0.5), tied, (1, 3)


HALF_BELOW = float(np.nextafter(F32(0.5), F32(0)))


def dt_threshold():
    """GT (0, 0, 1, 1): proposal 1 has IoU exactly 0.5 (a positive), proposal 0 the float32 below it (a negative), proposal 2 is far
    below.  ratio 0.25: room for three negatives per positive, so every classified proposal is in the output."""
    props = np.array([(0, 0, HALF_BELOW, 1), (0, 0, 0.5, 1), (0.1, 0.1, 0.3, 0.3)], F32)
    return DtCase(props, np.array([(0, 0, 1, 1)], F32), _caps(1), n_rois=8, ratio=0.25)


def dt_nan_row():
    """Proposal 1 and GT row 1 have zero area and are not zero rows: their IoU is 0 / 0.  That proposal is neither a positive nor a
    negative; the two positives and three negatives around it are classified as usual, and the negative quota (6) has room for it."""
    gt = np.array([(0.1, 0.1, 0.5, 0.5), (0.5, 0.2, 0.5, 0.4), (0.5, 0.5, 0.9, 0.9)], F32)
    props = np.array([(0.7, 0.1, 0.8, 0.2), (0.3, 0.3, 0.3, 0.6), (0.1, 0.1, 0.5, 0.5), (0.0, 0.6, 0.1, 0.7), (0.5, 0.5, 0.9, 0.85),
                      (0.3, 0.3, 0.35, 0.6)], F32)
    return DtCase(props, gt, _caps(3), n_rois=16, ratio=0.25)


def dt_all_positive():
    """101 proposals, each a copy of one of five GT boxes: 16 = max_positive positives, no negative at all."""
    rng = np.random.default_rng(5)
    y1, x1 = rng.uniform(0, 0.5, 5), rng.uniform(0, 0.5, 5)
    gt = np.stack([y1, x1, y1 + rng.uniform(0.1, 0.4, 5), x1 + rng.uniform(0.1, 0.4, 5)], 1).astype(F32)
    return DtCase(gt[rng.integers(0, 5, 101)], gt, _caps(5), n_rois=32, ratio=0.5)


def dt_no_positive():
    """75 small proposals, none reaching IoU 0.5 with one of four large GT boxes: no positive, hence int(r * 0) - 0 = 0 negatives."""
    rng = np.random.default_rng(6)
    gt = np.array([(0, 0, 0.6, 0.6), (0.3, 0.3, 1, 1), (0, 0.4, 0.5, 1), (0.5, 0, 1, 0.5)], F32)
    y1, x1 = rng.uniform(0, 0.9, 75), rng.uniform(0, 0.9, 75)
    return DtCase(np.stack([y1, x1, y1 + 0.08, x1 + 0.08], 1), gt, _caps(4), n_rois=32, ratio=0.5)


# ------------------------------------------------------------------------------------------------------------------------------
# RoIAlign (roi_align_kernel / roi_align_bwd_gather_kernel): non-square maps, every pool / C path
# ------------------------------------------------------------------------------------------------------------------------------
ROI_HW = [(24, 40), (12, 20), (6, 10), (3, 5)]
ROI_IMAGE = (512, 512)                   # image_area 2^18: sqrt(h w) = 0.4375 is level 4, log-uniform sides 0.05 .. 0.95 reach all four levels
ROI_B, ROI_R = 2, 70
ROI_MARGIN = 0.02                        # distance of every random box's float level from a half-integer
# (pool, C): pool 1 has its own sample formula, 16 is RA_MAX_POOL; C = 4 one lane, 260 = 65 float4 (a second accumulator with one live
# lane), 512 two full accumulators, 1024 all four.  C >= 512 with pool <= 7 only: the oracle's loops stay near a second.
ROI_SWEEP = [(1, 4), (2, 4), (7, 4), (16, 4), (1, 260), (2, 260), (7, 260), (16, 260), (7, 512), (1, 1024), (2, 1024), (7, 1024)]

ROI_LITERALS = {                         # name -> (image, index, box)
    "zero_a": (0, 0, (0, 0, 0, 0)), "zero_b": (0, 66, (0, 0, 0, 0)), "zero_c": (1, 69, (0, 0, 0, 0)),
    "flipped_both": (0, 3, (0.7, 0.8, 0.45, 0.55)),
    "flipped_y": (1, 64, (0.6, 0.2, 0.3, 0.5)),              # h w < 0: sqrt = NaN -> level 2, the samples run upwards
    "full": (0, 69, (0, 0, 1, 1)),
    "overrun": (1, 2, (-0.2, -0.2, 1.2, 1.2)),
    "nan": (0, 65, (np.nan, 0.2, 0.6, 0.7)),
}


def roi_float_level(boxes, image=ROI_IMAGE):
    """log2(sqrt(h w) / (224 / sqrt(area))) before rounding, float32 like O.roi_levels (NaN / -inf where the reference has them)."""
    b = np.asarray(boxes, F32)
    h, w = b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]
    with np.errstate(all="ignore"):
        ratio = np.sqrt(h * w, dtype=F32) / (F32(224.0) / np.sqrt(F32(image[0] * image[1]), dtype=F32))
        return np.log(ratio, dtype=F32) / np.log(F32(2.0), dtype=F32)


def roi_boxes():
    """[2, 70, 4] normalised (y1, x1, y2, x2): seeded boxes with log-uniform size and aspect ratios up to 2 : 1, each at least ROI_MARGIN
    away from a routing boundary, and the literal boxes of ROI_LITERALS (four of them in the ragged second round of 64 of the backward)."""
    rng = np.random.default_rng(70)
    boxes = np.zeros((ROI_B, ROI_R, 4), F32)
    for b in range(ROI_B):
        r = 0
        while r < ROI_R:
            s, ar = np.exp(rng.uniform(np.log(0.05), np.log(0.95))), np.exp(rng.uniform(np.log(0.5), np.log(2.0)))
            h, w = min(s * np.sqrt(ar), 1.0), min(s / np.sqrt(ar), 1.0)
            y, x = rng.uniform(0, 1 - h), rng.uniform(0, 1 - w)
            box = np.array([y, x, y + h, x + w], F32)
            lvl = float(roi_float_level(box))
            if abs(lvl - np.floor(lvl) - 0.5) >= ROI_MARGIN:
                boxes[b, r] = box
                r += 1
    for img, i, box in ROI_LITERALS.values():
        boxes[img, i] = box
    return boxes


def roi_random_mask():
    m = np.ones((ROI_B, ROI_R), bool)
    for img, i, _ in ROI_LITERALS.values():
        m[img, i] = False
    return m


def roi_maps(C, seed, B=ROI_B, hw=ROI_HW):
    """Four float32 maps [B, H, W, C] (and, with another seed, the non-zero maps the backward accumulates into)."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((B, h, w, C)).astype(F32) for h, w in hw]


def roi_grad(R, pool, C, seed, B=ROI_B):
    return np.random.default_rng(seed).standard_normal((B, R, pool, pool, C)).astype(F32)


# Integral samples: level-2 maps of 13 x 25 (H - 1 = 12, W - 1 = 24), pool 7, corners on multiples of 1/12 and 1/24, extents multiples
# of 6/12 and 6/24: sample (py, px) is pixel (y1 12 + py ey / 6, x1 24 + px ex / 6) exactly.  (y1 12, ey, x1 24, ex) per box:
INTEGRAL_HW = [(13, 25), (7, 13), (4, 7), (2, 4)]
INTEGRAL_IMAGE = (64, 64)                # image_area 2^12: every box with sqrt(h w) <= 1 is below level 2.5
INTEGRAL_GRID = [(0, 6, 0, 6), (0, 12, 0, 24), (6, 6, 18, 6), (3, 6, 6, 12), (6, 6, 0, 18), (2, 6, 2, 6), (5, 6, 11, 12), (4, 6, 7, 12),
                 (12, -12, 24, -24), (9, -6, 3, 12)]       # the last two flipped: in both axes (level 2 by size), in y (level 2 by NaN)


def integral_boxes():
    """[1, 10, 4] float32 boxes of INTEGRAL_GRID and, per box, the pixel rows [7] and columns [7] its samples land on."""
    g = np.array(INTEGRAL_GRID, np.float64)
    boxes = np.stack([g[:, 0] / 12, g[:, 2] / 24, (g[:, 0] + g[:, 1]) / 12, (g[:, 2] + g[:, 3]) / 24], 1).astype(F32)
    p = np.arange(7)[None, :]
    rows, cols = g[:, :1] + p * g[:, 1:2] / 6, g[:, 2:3] + p * g[:, 3:4] / 6
    return boxes[None], rows.astype(np.int64), cols.astype(np.int64)


def integral_sample_coordinates(boxes, hw=INTEGRAL_HW[0], pool=7):
    """The float32 sample coordinates of crop_and_resize, operation by operation (O.crop_and_resize): ([n, pool] in_y, [n, pool] in_x)."""
    b = np.asarray(boxes, F32).reshape(-1, 4)
    p = np.arange(pool, dtype=F32)[None, :]

    def axis(lo, hi, n):
        step = (hi - lo) * F32(n - 1) / F32(pool - 1)
        return (lo * F32(n - 1))[:, None] + p * step[:, None]
    return axis(b[:, 0], b[:, 2], hw[0]), axis(b[:, 1], b[:, 3], hw[1])
