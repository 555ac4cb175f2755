"""Inputs for test_gpu_detect_edges.py: the detection kernels of csrc/detect.hip at the sizes where their grids and loops wrap (plain
functions: seeded NumPy and literal boxes, no GPU, no fixtures).

Every case states what it holds -- a box in the third 256-wide x block, ones in the rows of paste_v_kernel's second grid-stride pass, an
axis with 129 taps, an invalid class id on a wave's last lane, a maximum that only the last pass of the lane loop sees -- and
test_detect_cases.py (CPU) proves the statements on the host references alone.  select_case and tail_case moved here from
test_gpu_detect_kernels.py, which imports them.

Out of scope, everywhere: NaN (its cast to a byte is undefined on the host, and np.argmax's answer differs from a comparison's), +inf
logits and rows of nothing but -inf (class_select_kernel documents them as not expected), masks with subnormal values or a range below
1e-30 (bytescale's 255 / range must stay finite)."""
import functools
import zlib

import numpy as np

import _maskrcnn_ref as R

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------------
# class_select (class_select_kernel): one wave per row, lane j takes classes j, j + 64, j + 128, ...; four rows per block
# ------------------------------------------------------------------------------------------------------------------------------
CS_LANES, CS_ROWS = 64, 4


def select_case(R_, C, seed=0):
    """Logits normal * 3 with +-80 planted; ties between equal maximal logits planted in the first rows: two lanes (3 and 70 -> lanes 3
    and 6 when C = 81), one lane's two passes (5 and 69), neighbours (0 and 1)."""
    rng = np.random.RandomState(100 * R_ + C + seed)
    z = (rng.randn(R_, C) * 3.0).astype(np.float32)
    z.reshape(-1)[rng.permutation(z.size)[:max(2, z.size // 50)]] = rng.choice([80.0, -80.0], max(2, z.size // 50))
    ties = [(0, 1), (C - 2, C - 1)] + ([(3, 70), (5, 69)] if C > 70 else [])
    for r, (a, b) in enumerate(ties):
        if r < R_:
            z[r, a] = z[r, b] = np.float32(max(81.0, z[r].max() + 1.0)) if r % 2 == 0 else z[r].max() + np.float32(0.5)
    d = rng.randn(R_, 4 * C).astype(np.float32)
    return z, d


SELECT_C = [63, 64, 65, 128, 129, 200]          # one pass less a lane, one pass, one lane's second pass, two passes, a lone third, three and a bit
SELECT_R = [4, 5, 259]                          # one full block, one row in a second block, 64 blocks and three rows


def select_finite_gap(z):
    """The largest finite max - z_j: what the score bound (d_max + C + 8) u is stated on (exp(-inf) is an exact 0 and adds no error)."""
    gap = np.asarray(z, np.float64).max(axis=1, keepdims=True) - np.asarray(z, np.float64)
    return float(gap[np.isfinite(gap)].max())


def select_planted(C):
    """(z [n,C], d [n,4C], names, expected ids): the planted rows that exist at this C, each on a base row of normal * 3.
      last_only         the maximum at C - 1 alone (C = 65 / 129: the single element of the last pass)
      tie_5_69_133      C = 200: one lane's three passes hold the same maximum -> 5
      tie_64_1          C = 65: lane 0's second pass against lane 1's first -> 1
      tie_63_64         C >= 65: the last lane's first pass against lane 0's second -> 63
      only_70_finite    C > 70: -inf everywhere but index 70 -> 70, score exactly 1
      neg_inf_at_0      -inf at index 0, finite elsewhere -> the maximum of the rest"""
    rng = np.random.RandomState(7000 + C)
    rows, names, want = [], [], []

    def base():
        return (rng.randn(C) * 3.0).astype(F32)

    def add(name, row, k):
        rows.append(row), names.append(name), want.append(k)

    z = base()
    z[C - 1] = z.max() + F32(2.0)
    add("last_only", z, C - 1)
    if C == 200:
        z = base()
        z[[5, 69, 133]] = z.max() + F32(1.0)
        add("tie_5_69_133", z, 5)
    if C == 65:
        z = base()
        z[[64, 1]] = z.max() + F32(1.0)
        add("tie_64_1", z, 1)
    if C >= 65:
        z = base()
        z[[63, 64]] = z.max() + F32(0.5)
        add("tie_63_64", z, 63)
    if C > 70:
        z = np.full(C, -np.inf, F32)
        z[70] = F32(-3.25)
        add("only_70_finite", z, 70)
    z = base()
    z[0] = -np.inf
    k = 1 + int(np.argmax(z[1:]))
    add("neg_inf_at_0", z, k)
    return np.stack(rows), rng.randn(len(rows), 4 * C).astype(F32), names, want


# ------------------------------------------------------------------------------------------------------------------------------
# mask_head_tail (mask_head_tail_kernel): blocks of 128 rows (N P P pixels), 4 waves x 32 pixels, weight slices of 32 channels
# ------------------------------------------------------------------------------------------------------------------------------
MT_ROWS, MT_WAVE_ROWS = 128, 32
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def tail_case(N, Cin, Cmid, C, big=False, P=14):
    rng = np.random.RandomState(N * 1000 + Cin + Cmid + C + (7 if big else 0))
    x = np.maximum(rng.randn(N, P, P, Cin), 0.0).astype(np.float32)      # what a ReLU hands over
    wd = (rng.randn(2, 2, Cmid, Cin) / np.sqrt(Cin)).astype(np.float32)
    bd = (0.1 * rng.randn(Cmid)).astype(np.float32)
    wm = (rng.randn(Cmid, C) * 2.0 / np.sqrt(Cmid)).astype(np.float32)
    bm = (0.1 * rng.randn(C)).astype(np.float32)
    ids = rng.randint(0, C, N).astype(np.int32)
    ids[-1] = C - 1
    if N >= 3:
        ids[0], ids[1] = 0, (C if N == 3 else -1)                        # one id out of range, between two valid neighbours
    if big:
        bm[0], bm[C - 1] = 200.0, -200.0
    return x, wd, bd, wm, bm, ids


def _lane_ids():
    ids = np.arange(70, dtype=np.int64)
    ids[0], ids[31], ids[32], ids[69] = -1, 70, INT_MAX, INT_MIN
    return ids


# name -> (P, N, Cin, Cmid, C, signed x, class ids or None for seeded valid ones)
TAIL_EDGES = {
    "single_pixel": (1, 1, 32, 32, 2, True, [1]),                        # 127 clamped lanes; Cin = 32: one staged word per thread
    "lane_per_roi": (1, 70, 96, 96, 70, False, _lane_ids()),             # every lane another RoI and class column
    "max_p_four_blocks": (16, 2, 160, 64, 5, True, [4, 0]),              # 512 rows: exactly four blocks
    "cin_below_cmid": (7, 3, 32, 256, 81, False, [0, 37, 80]),           # 147 rows
    "cin_above_cmid": (7, 3, 256, 32, 81, True, [80, 0, 41]),
    "rows_128": (4, 8, 224, 96, 5, False, None),                         # one full block and nothing else
    "rows_144": (4, 9, 224, 96, 5, True, None),                          # a block and 16 rows
    "all_invalid": (14, 3, 128, 128, 5, False, [-1, 5, INT_MAX]),
    "invalid_first": (14, 3, 64, 32, 5, True, [5, 1, 4]),
    "invalid_last": (14, 3, 64, 32, 5, False, [0, 3, -1]),
    "off_boundary": (7, 3, 96, 96, 5, True, [0, 2, 4]),                  # the 4-byte-load instantiation away from 64 / 32
}


@functools.lru_cache(maxsize=None)
def tail_edge(name):
    """(x, wd, bd, wm, bm, ids) of TAIL_EDGES[name], at tail_case's scales; signed: x is normal, not what a ReLU hands over."""
    P, N, Cin, Cmid, C, signed, ids = TAIL_EDGES[name]
    rng = np.random.RandomState(zlib.crc32(name.encode()))           # the name alone: adding a case reseeds no other
    x = rng.randn(N, P, P, Cin)
    x = (x if signed else np.maximum(x, 0.0)).astype(F32)
    wd = (rng.randn(2, 2, Cmid, Cin) / np.sqrt(Cin)).astype(F32)
    bd = (0.1 * rng.randn(Cmid)).astype(F32)
    wm = (rng.randn(Cmid, C) * 2.0 / np.sqrt(Cmid)).astype(F32)
    bm = (0.1 * rng.randn(C)).astype(F32)
    ids = np.asarray(rng.randint(0, C, N) if ids is None else ids, np.int64).astype(np.int32)
    assert ids.shape == (N,)
    for a in (x, wd, bd, wm, bm, ids):
        a.setflags(write=False)
    return x, wd, bd, wm, bm, ids


@functools.lru_cache(maxsize=None)
def tail_reference(name):
    """R.mask_tail of the case, computed once: (out, z, A)."""
    return R.mask_tail(*tail_edge(name))


def tail_pre_relu(name):
    """[N P P, 4 Cmid] float64: what the ReLU of the case sees, whatever the class ids."""
    x, wd, bd = (np.asarray(a, np.float64) for a in tail_edge(name)[:3])
    return np.concatenate([x.reshape(-1, x.shape[-1]) @ wd[dy, dx].T + bd for dy in range(2) for dx in range(2)], axis=1)


# ------------------------------------------------------------------------------------------------------------------------------
# mask_paste (paste_coef_kernel / paste_h_kernel / paste_v_kernel): x = blockIdx.x * 256 + threadIdx.x, rows by a grid-stride loop of
# at most 65535 blocks
# ------------------------------------------------------------------------------------------------------------------------------
MP_THREADS, MP_MAX_GRID = 256, 65535


def resize_ksize(in_size, out_size):
    """resize_core.h's resize_ksize (precompute_coeffs' ksize for the bilinear filter, support 1.0)."""
    scale = float(in_size) / float(out_size)
    return int(np.ceil(1.0 * max(scale, 1.0))) * 2 + 1


def blob_masks(M, h=28, w=28, seed=11):
    """Soft discs of differing centre and radius over a lattice of high lines (rows and columns 0, 8, 9, 17, 18, 26, 27 of 28: the
    first and the last sample of both axes are high, so a box holds ones at its far edges), plus 3 % noise, in [0.02, 1]."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = 0.43 * h, 0.54 * w
    lattice = np.where(np.isin(yy % 9, (0, 8)) | np.isin(xx % 9, (0, 8)), 0.85, 0.0)
    out = []
    for i in range(M):
        r = np.hypot((yy - cy - i % 3) * 28.0 / h, (xx - cx + i % 5) * 28.0 / w)
        blob = np.maximum(1.0 / (1.0 + np.exp(-(5.0 + i % 4 - r) * 0.8)), lattice)
        out.append((0.02 + 0.95 * blob + 0.03 * rng.rand(h, w)).astype(F32))
    return np.stack(out)


def stripe_masks(M, h, w, axis, seed):
    """Bands one sample wide along `axis`, low first: the last sample is high, so the far end of a box holds ones and the stretch
    before it zeros.  10 % noise."""
    rng = np.random.RandomState(seed)
    idx = np.arange(h if axis == 0 else w)
    band = np.where(idx % 2 == 1, 0.85, 0.05)
    plane = np.broadcast_to(band[:, None] if axis == 0 else band[None, :], (h, w))
    return np.stack([(plane + 0.1 * rng.rand(h, w)).astype(F32) for _ in range(M)])


def structured_masks(h, w):
    """[3,h,w]: a checker of period 8 (squares of 4), the half-plane y < h / 2 or x < w / 2 (whichever axis is longer), and a diagonal
    half-plane -- in each, a dropped or doubled tap of a long window moves the byte across the threshold."""
    yy, xx = np.mgrid[0:h, 0:w]
    checker = ((yy // 4 + xx // 4) % 2).astype(F32)
    half = (yy < h / 2.0 if h >= w else xx < w / 2.0).astype(F32)
    diag = (yy * w + xx * h < h * w * 1.02).astype(F32) * F32(0.9) + F32(0.05)
    if h == 1 or w == 1:
        diag = ((yy + xx) % 8 < 5).astype(F32)                          # on a line: period 8, five high of eight
    return np.stack([checker, half, diag])


class PasteCase(object):
    """masks float32 [M,h,w], boxes int32 [M,4] (y1, x1, y2, x2), the image H x W; labels[i] names what box i is there for."""

    def __init__(self, name, H, W, masks, boxes, labels):
        self.name, self.H, self.W = name, H, W
        self.masks, self.boxes, self.labels = np.ascontiguousarray(masks, F32), np.asarray(boxes, np.int32).reshape(-1, 4), list(labels)
        self.M = self.masks.shape[0]
        assert self.boxes.shape[0] == self.M == len(self.labels)
        self._want = None

    def index(self, label):
        return self.labels.index(label)

    def reference(self):
        """mask_rcnn_model.unmold_mask (PIL) of every detection, uint8 [M,H,W]; computed once, read-only."""
        if self._want is None:
            from image_captioning_amd import mask_rcnn_model as MR
            want = np.stack([MR.unmold_mask(self.masks[i], self.boxes[i], (self.H, self.W, 3)) for i in range(self.M)])
            want.setflags(write=False)
            self._want = want
        return self._want


BLOCKS_BOXES = [
    ("full", (0, 0, 300, 521)),
    ("across_256", (10, 200, 60, 400)),                # x1 < 256 < x2 < 512
    ("past_512", (20, 513, 50, 520)),                  # the third x block alone
    ("w256_at_0", (5, 0, 40, 256)),
    ("w257_at_0", (5, 0, 40, 257)),
    ("w256_at_255", (100, 255, 130, 511)),
    ("w257_at_255", (100, 255, 130, 512)),
    ("column_256", (50, 256, 90, 257)),
    ("column_520", (50, 520, 90, 521)),
    ("taller_than_256", (3, 300, 290, 330)),
    ("touches_corner", (270, 480, 300, 521)),
    ("leaves_in_x", (270, 480, 300, 522)),             # one pixel past the right edge, y inside: zeros
]


def _paste_blocks():
    return PasteCase("blocks_300x521", 300, 521, blob_masks(len(BLOCKS_BOXES)), [b for _, b in BLOCKS_BOXES], [n for n, _ in BLOCKS_BOXES])


def _paste_tall():
    boxes = [("full", (0, 0, 70001, 3)), ("second_pass_only", (65600, 1, 69990, 3)), ("straddles_65535", (65000, 0, 66000, 2))]
    return PasteCase("rows_70001x3", 70001, 3, stripe_masks(3, 28, 28, 0, 21), [b for _, b in boxes], [n for n, _ in boxes])


def _paste_wide():
    boxes = [("full", (0, 0, 3, 70001)), ("wider_than_65535", (1, 100, 3, 66000))]
    return PasteCase("cols_3x70001", 3, 70001, stripe_masks(2, 28, 28, 1, 22), [b for _, b in boxes], [n for n, _ in boxes])


# box sides (bh, bw) on the 40 x 50 image, each with the three structured masks
TAPS_BOXES_64x64 = [(1, 1), (1, 3), (3, 1), (2, 2), (3, 50)]
TAPS_BOXES_64x1 = [(1, 1), (2, 1), (3, 1), (3, 3)]         # a 64 x 1 mask: the y axis shrinks 64 -> 1 .. 3
TAPS_BOXES_1x64 = [(1, 1), (1, 2), (1, 3), (3, 3)]


def _paste_taps(name, h, w, sides):
    three = structured_masks(h, w)
    masks, boxes, labels = [], [], []
    for j, (bh, bw) in enumerate(sides):
        for k, kind in enumerate(("checker", "half", "diagonal")):
            y1, x1 = (7 * j + 3 * k) % (40 - bh + 1), (11 * j + 5 * k) % (50 - bw + 1)
            masks.append(three[k]), boxes.append((y1, x1, y1 + bh, x1 + bw)), labels.append("%dx%d_%s" % (bh, bw, kind))
    return PasteCase(name, 40, 50, np.stack(masks), boxes, labels)


def _paste_production():
    return PasteCase("production_1024", 1024, 1024, blob_masks(1), [(60, 70, 960, 970)], ["900x900"])


TIE_SHIFT = 3                                    # the x.5 grid: lo = 0, hi = 255 * 2^-3, values (j + 0.5) * 2^-3


def bytescale_edge_masks():
    """[3,28,28]: `ulp`: 0.5 and the float32 above it (range 2^-24) in a disc; `negative`: a blob in [-1.46, -0.5]; `ties`: 0, 255 / 8
    and the half-integers of the grid between them, so that (m - lo) * scale is j + 0.5 exactly, with a 6 x 6 patch at 127.5 -- byte
    128 when the tie goes up as bytescale's does, 127 when it goes down: the threshold itself."""
    blob = blob_masks(1)[0].astype(np.float64)
    ulp = np.where(blob > 0.5, np.nextafter(F32(0.5), F32(1.0)), F32(0.5)).astype(F32)
    negative = (blob - 1.5).astype(F32)
    j = np.floor(np.clip(blob, 0.0, 1.0) * 254.0)
    j[10:16, 2:8] = 127.0
    ties = ((j + 0.5) * 2.0 ** -TIE_SHIFT).astype(F32)
    ties[0, 0], ties[27, 27] = 0.0, 255.0 * 2.0 ** -TIE_SHIFT
    return np.stack([ulp, negative, ties])


def tie_bytes(ties, mode):
    """bytescale of the `ties` mask with its exact x.5 values rounded "up" (bytescale's own: floor(v + 0.5)), "down" or to "even"."""
    v = np.asarray(ties, np.float64) * 2.0 ** TIE_SHIFT              # exact: lo = 0 and the scale is 2^3
    up = np.floor(v + 0.5)
    tie = v - np.floor(v) == 0.5
    out = {"up": up, "down": np.where(tie, up - 1.0, up), "even": np.where(tie & (up % 2 == 1), up - 1.0, up)}[mode]
    return out.astype(np.uint8)


def paste_bytes(bytes_, bbox, image_shape):
    """_maskrcnn_ref.unmold_mask from the byte plane on: the integer resize, the threshold, the paste (for boxes inside the image)."""
    import _resize_ref as RS
    y1, x1, y2, x2 = (int(v) for v in bbox)
    full = np.zeros((int(image_shape[0]), int(image_shape[1])), np.uint8)
    small = RS.resize_bilinear(np.asarray(bytes_, np.uint8)[:, :, None], y2 - y1, x2 - x1)[:, :, 0]
    full[y1:y2, x1:x2] = small >= 128
    return full


def _paste_bytescale():
    ulp, negative, ties = bytescale_edge_masks()
    boxes = [(10, 20, 80, 120), (0, 0, 97, 131), (10, 20, 80, 120), (30, 40, 58, 68)]       # up, the whole image, up, identity (28 x 28)
    return PasteCase("bytescale_97x131", 97, 131, np.stack([ulp, negative, ties, ties]), boxes, ["ulp", "negative", "ties", "ties_identity"])


_PASTE = {
    "blocks_300x521": _paste_blocks,
    "rows_70001x3": _paste_tall,
    "cols_3x70001": _paste_wide,
    "taps_64x64": lambda: _paste_taps("taps_64x64", 64, 64, TAPS_BOXES_64x64),
    "taps_64x1": lambda: _paste_taps("taps_64x1", 64, 1, TAPS_BOXES_64x1),
    "taps_1x64": lambda: _paste_taps("taps_1x64", 1, 64, TAPS_BOXES_1x64),
    "production_1024": _paste_production,
    "bytescale_97x131": _paste_bytescale,
}
PASTE_NAMES = list(_PASTE)


@functools.lru_cache(maxsize=None)
def paste_case(name):
    return _PASTE[name]()
