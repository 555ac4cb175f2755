"""COCO's run-length encoding of a binary [H,W] mask, on the host in NumPy: what MaskRCNN.detect(mask_format="rle") returns per
detection, and the reference ops.mask_rle (dc_mask_rle_u32, include/dcap.h) is held to.

The uncompressed form.  Pixels are read column-major, pixel (y, x) at index x * H + y.  With t_0 < t_1 < ... the indices at which
bit[i] != bit[i-1] (bit[-1] = 0), counts are the differences of [0, t_0, t_1, ..., H * W]: runs of zeros and ones in turn, starting
with zeros, so counts[0] == 0 exactly when pixel (0, 0) is set.  T transitions give T + 1 counts and the last entry is the final run,
whatever its value: a mask whose last pixel is set ends on its run of ones, no zero-length run of zeros follows.  An all-zero mask is
[H * W]; sum(counts) == H * W always.  An RLE is {"size": [H, W], "counts": uint32 ndarray}.

The string form is pycocotools' rleToString / rleFrString: each count, from the fourth on minus the count two places before it, goes
out in 5-bit groups, low group first, bit 0x20 saying that more follow, each group as chr(group + 48).  to_coco gives the
{"size", "counts": str} entry of a COCO results file.

iou is pycocotools' rleIou on this form and to_bbox the box utils.extract_bboxes takes from the dense plane; ops.rle_iou
(dc_rle_iou_f64, include/dcap.h) is held to iou bit for bit."""
import numpy as np


def encode(mask):
    """[H,W] bool or uint8 (non-zero = set) -> {"size": [H, W], "counts": uint32 ndarray}."""
    m = np.asarray(mask)
    if m.ndim != 2 or m.dtype not in (np.dtype(bool), np.dtype(np.uint8)):
        raise ValueError("mask_rle.encode: mask must be a bool or uint8 [H,W] array, got %s %s" % (m.dtype, m.shape))
    H, W = m.shape
    bits = (m != 0).T.reshape(-1)                         # column-major: index x * H + y
    edges = np.flatnonzero(bits[1:] != bits[:-1]) + 1
    if bits.size and bits[0]:
        edges = np.concatenate([[0], edges])
    counts = np.diff(np.concatenate([[0], edges, [H * W]]))
    return {"size": [int(H), int(W)], "counts": counts.astype(np.uint32)}


def _size_and_counts(rle, who):
    H, W = (int(v) for v in rle["size"])
    counts = np.asarray(rle["counts"])
    if isinstance(rle["counts"], (str, bytes)):
        counts = from_string(rle["counts"])
    if H < 0 or W < 0 or counts.ndim != 1 or counts.size == 0 or (counts.astype(np.int64) < 0).any():
        raise ValueError("mask_rle.%s: size must be [H, W] and counts a non-empty list of run lengths, got size %r and %d counts"
                         % (who, rle["size"], counts.size))
    total = int(counts.astype(np.int64).sum())
    if total != H * W:
        raise ValueError("mask_rle.%s: the counts sum to %d, the mask of size %d x %d has %d pixels" % (who, total, H, W, H * W))
    return H, W, counts.astype(np.int64)


def decode(rle):
    """{"size", "counts"} (counts an array or the string form) -> uint8 [H,W] of 0 / 1.  Counts that do not sum to H * W are refused."""
    H, W, counts = _size_and_counts(rle, "decode")
    values = (np.arange(counts.size) & 1).astype(np.uint8)
    return np.repeat(values, counts).reshape(W, H).T.copy()


def area(rle):
    """The number of set pixels: the sum of the odd-indexed counts."""
    counts = rle["counts"]
    if isinstance(counts, (str, bytes)):
        counts = from_string(counts)
    return int(np.asarray(counts)[1::2].astype(np.int64).sum())


def to_string(counts):
    """uncompressed counts -> pycocotools' string."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    out = []
    for i, x in enumerate(c):
        if i > 2:
            x -= c[i - 2]
        more = True
        while more:
            g = x & 0x1f
            x >>= 5                                       # (Python's >> on a negative int is the arithmetic shift)
            more = x != -1 if g & 0x10 else x != 0
            if more:
                g |= 0x20
            out.append(chr(g + 48))
    return "".join(out)


def from_string(s):
    """pycocotools' string -> uint32 counts.  A string that ends inside a count, a character outside the alphabet and a negative count
    are refused."""
    if isinstance(s, bytes):
        s = s.decode("ascii")
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            if p >= len(s):
                raise ValueError("mask_rle.from_string: the string is truncated: it ends inside count %d" % len(counts))
            g = ord(s[p]) - 48
            if not 0 <= g < 64:
                raise ValueError("mask_rle.from_string: character %r at position %d is not part of an RLE string" % (s[p], p))
            x |= (g & 0x1f) << (5 * k)
            more = bool(g & 0x20)
            p += 1
            k += 1
            if not more and g & 0x10:
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        if not 0 <= x < 1 << 32:
            raise ValueError("mask_rle.from_string: count %d decodes to %d, which is no run length" % (len(counts), x))
        counts.append(x)
    return np.array(counts, np.uint32)


def to_coco(rle):
    """{"size", "counts": array} -> {"size": [H, W], "counts": str}: the "segmentation" of a COCO results entry."""
    H, W, counts = _size_and_counts(rle, "to_coco")
    return {"size": [H, W], "counts": to_string(counts)}


def _intersection(a, b):
    """The pixels set in both of two encodings of one size: a two-pointer walk over the runs (lists of Python ints)."""
    i = j = inter = 0
    ca, cb = a[0], b[0]
    while True:
        c = ca if ca < cb else cb
        if i & j & 1:
            inter += c
        ca -= c
        cb -= c
        if ca == 0:
            i += 1
            if i == len(a):
                return inter
            ca = a[i]
        if cb == 0:
            j += 1
            if j == len(b):
                return inter
            cb = b[j]


def iou(dt, gt, iscrowd=None):
    """pycocotools' rleIou: float64 [len(dt), len(gt)] for two lists of {"size", "counts"} of ONE size.  The intersection I is an
    exact integer, iou = I / (a_d + a_g - I) one float64 division; for a crowd gt (iscrowd[g] non-zero) iou = I / a_d; 0 where the
    denominator is 0.  Lists whose masks differ in size and counts that do not sum to H * W are refused."""
    sides = [_size_and_counts(r, "iou") for r in list(dt) + list(gt)]
    if len({(H, W) for H, W, _ in sides}) > 1:
        raise ValueError("mask_rle.iou: every mask must have one size, got %s" % sorted({(H, W) for H, W, _ in sides}))
    crowd = np.zeros(len(gt), bool) if iscrowd is None else np.asarray(iscrowd).reshape(-1) != 0
    if crowd.size != len(gt):
        raise ValueError("mask_rle.iou: iscrowd must hold one flag per gt mask, got %d for %d" % (crowd.size, len(gt)))
    runs = [[int(v) for v in c] for _, _, c in sides]
    areas = [sum(r[1::2]) for r in runs]
    D = len(dt)
    out = np.zeros((D, len(gt)), np.float64)
    for d in range(D):
        for g in range(len(gt)):
            inter = _intersection(runs[d], runs[D + g]) if areas[d] and areas[D + g] else 0
            den = areas[d] if crowd[g] else areas[d] + areas[D + g] - inter
            if den:
                out[d, g] = np.float64(inter) / np.float64(den)
    return out


def to_bbox(rle):
    """int32 [4] (y1, x1, y2, x2), the end exclusive: utils.extract_bboxes' box of the decoded plane, zeros for an empty mask."""
    H, W, counts = _size_and_counts(rle, "to_bbox")
    ends = np.cumsum(counts)
    s, e = (ends - counts)[1::2], ends[1::2]
    s, e = s[e > s], e[e > s]
    if s.size == 0:
        return np.zeros(4, np.int32)
    last = e - 1
    wraps = (s // H != last // H).any()                   # a run that leaves its column touches row H - 1 and row 0
    y1 = 0 if wraps else int((s % H).min())
    y2 = H if wraps else int((last % H).max()) + 1
    return np.array([y1, int(s[0] // H), y2, int(last[-1] // H) + 1], np.int32)
