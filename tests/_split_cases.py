"""The split-bf16 arithmetic, piece product by piece product (host only: NumPy, no torch, no GPU).

Every fp32 operand element is three bf16 pieces, x = p0 + p1 + p2, and a product is the six piece products of order 2^-16 or larger,
    p0 q0 + (p0 q1 + p1 q0) + (p0 q2 + p1 q1 + p2 q0)                                                  (csrc/igemm_bf16s.h)
A kernel's output is multilinear in the pieces, so the contribution D_ij of piece product (i, j) -- i the activation's piece, j the
weight's -- is computed here in float64, and the projection
    c_ij = <got - want, D_ij> / <D_ij, D_ij>            (want: float64 on the fp32 operands)
is about 0 where the kernel includes product (i, j), about -1 where it is missing and about +1 where it is counted twice: the sum over a
thousand or more outputs averages the fp32 accumulation noise away, where a max-norm error separates right from wrong by a factor of two.

Three forms: MatrixProblem (a convolution as im2col, a 1x1 layer, either layer of the chained 1x1 kernel), WinoProblem (Winograd
F(2x2, 3x3): the pieces are those of V = B^T d B and U = G g G^T) and chain_layer1 / chain_layer2 (layer 2 on the fp32 y that layer 1
produced, the operand the kernel actually split).  emulate() is the intended arithmetic -- one fp32 rounding per 16-deep product, the kernels' order of products --
or a wrong one on purpose; tests/test_split_cases.py proves the instrument on it, tests/test_gpu_split_products.py holds the kernels to it."""
import functools

import numpy as np

from oracle import np_oracle as O

F32, F64 = np.float32, np.float64

KEPT = ((0, 1), (1, 0), (0, 2), (1, 1), (2, 0))            # the five cross products a three-piece kernel keeps beside p0 q0
SECOND, THIRD = KEPT[:2], KEPT[2:]
# the order every kernel issues them in, smallest terms first (activation piece, weight piece)
ORDER = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))
MIN_STRATUM = 1024


def split3(x):
    """The three bf16 pieces of an fp32 array as float64 [3, *x.shape]: each rounded to nearest even, the remainders exact in fp32
    (split_pair of csrc/igemm_bf16s.h)."""
    r = np.ascontiguousarray(np.asarray(x, F32))
    out = np.empty((3,) + r.shape, F64)
    for p in range(3):
        out[p] = O.to_bf16(r)
        r = r - out[p].astype(F32)                         # exact: the piece holds the remainder's leading bits
    return out


def bf16_bits(pieces):
    """float64 values on the bf16 grid -> their 16-bit patterns (uint16)."""
    return (np.ascontiguousarray(np.asarray(pieces, F32)).view(np.uint32) >> 16).astype(np.uint16)


def products(pieces=3, drop=None, twice=None):
    """The piece products an emulation sums, in the kernels' order: those of a `pieces`-piece split, without `drop`, `twice` twice."""
    out = []
    for ij in ORDER:
        if ij[0] + ij[1] >= pieces or ij == drop:
            continue
        out += [ij, ij] if ij == twice else [ij]
    return out


def channel_strata(shape, whole=None):
    """32-output-channel blocks of an output [..., C] (one wave's / one slice's share), restricted to the boolean pixel mask `whole`."""
    C = shape[-1]
    out = []
    for c0 in range(0, C, 32):
        m = np.zeros(shape, bool)
        m[..., c0:c0 + 32] = True
        if whole is not None:
            m &= whole
        out.append(("channels %d-%d" % (c0, c0 + 31), m))
    return out


def coefficients(got, want, D, strata, whole=None):
    """{stratum: {(i, j): c_ij}} over the whole output ("all"; the boolean mask `whole` where only a part of it was computed) and over
    every stratum [(name, boolean mask or index)]."""
    err = np.asarray(got, F64) - want
    out = {}
    for name, idx in [("all", Ellipsis if whole is None else whole)] + list(strata):
        e = err[idx].ravel()
        out[name] = {}
        for ij, d in D.items():
            dd = d[idx].ravel()
            out[name][ij] = float(e @ dd) / float(dd @ dd)
    return out


def worst(coef, keys):
    """(largest |c|, stratum, (i, j)) over the products `keys`."""
    return max((abs(c[ij]), name, ij) for name, c in coef.items() for ij in keys)


def _affine(v, scale, shift, add):
    if scale is not None:
        v = v * scale
    if shift is not None:
        v = v + shift
    return v if add is None else v + add


class MatrixProblem(object):
    """out[M, N] = (A @ B^T) scale + shift + add with A [M, K] the activations (an im2col matrix, a 1x1 layer's pixels) and B [N, K] the
    packed kernel, both fp32.  out_shape: the shape the kernel's output has ([N, Ho, Wo, Cout] for a convolution)."""

    def __init__(self, A, B, scale=None, shift=None, add=None, out_shape=None, whole=None):
        self.A, self.B = np.ascontiguousarray(A, F32), np.ascontiguousarray(B, F32)
        self.scale = None if scale is None else np.asarray(scale, F32).astype(F64)
        self.shift = None if shift is None else np.asarray(shift, F32).astype(F64)
        self.out_shape = tuple(out_shape or (self.A.shape[0], self.B.shape[0]))
        self.add = None if add is None else np.asarray(add, F32).astype(F64).reshape(self.out_shape)
        self.whole = whole                                 # boolean mask of the computed part (list-driven launches), or None
        self.strata = channel_strata(self.out_shape, whole)
        self.K = self.A.shape[1]

    @functools.cached_property
    def pieces(self):
        return split3(self.A), split3(self.B)

    @functools.cached_property
    def want(self):
        return _affine((self.A.astype(F64) @ self.B.astype(F64).T).reshape(self.out_shape), self.scale, self.shift, self.add)

    @functools.cached_property
    def D(self):
        a, b = self.pieces
        return {(i, j): _affine((a[i] @ b[j].T).reshape(self.out_shape), self.scale, None, None) for i, j in KEPT}

    def emulate(self, drop=None, twice=None, pieces=3):
        a, b = self.pieces
        acc = np.zeros((self.A.shape[0], self.B.shape[0]), F32)
        todo = products(pieces, drop, twice)
        for k0 in range(0, self.K, 16):
            for i, j in todo:
                acc = (acc + a[i][:, k0:k0 + 16] @ b[j][:, k0:k0 + 16].T).astype(F32)     # float64 sum, ONE fp32 rounding: the MFMA's
        return _affine(acc.astype(F64).reshape(self.out_shape), self.scale, self.shift, self.add).astype(F32)


def im2col(x, kh, kw, stride, pad_t, pad_l, Ho, Wo):
    """x [N, H, W, C] -> [N Ho Wo, kh kw C] (tap-major, channels fastest: packing.pack_conv_kernel's K order), zero padded."""
    N, H, W, C = x.shape
    xp = np.zeros((N, pad_t + H + kh + stride, pad_l + W + kw + stride, C), x.dtype)
    xp[:, pad_t:pad_t + H, pad_l:pad_l + W] = x
    cols = [xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] for ky in range(kh) for kx in range(kw)]
    return np.stack(cols, 3).reshape(N * Ho * Wo, kh * kw * C)


def wino_U(w):
    """U = G g G^T of an HWIO kernel in float32, summed as wino_pack_kernel sums it: [4, 4, Cin, Cout]."""
    g = np.asarray(w, F32)
    h = F32(0.5)

    def rows(t):                                           # G t over the leading axis
        return np.stack([t[0], h * (t[0] + t[1] + t[2]), h * (t[0] - t[1] + t[2]), t[2]], 0)
    gg = rows(g)                                           # [4, 3, Cin, Cout]
    return np.ascontiguousarray(np.moveaxis(rows(np.moveaxis(gg, 1, 0)), 0, 1))


def wino_V(x):
    """V = B^T d B of every 2 x 2 output tile's 4 x 4 patch in float32 (each value the sum of two terms twice over: no summation order to
    choose): [N, th, tw, 4, 4, Cin]."""
    x = np.asarray(x, F32)
    N, H, W, C = x.shape
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((N, 2 * th + 2, 2 * tw + 2, C), F32)
    xp[:, 1:H + 1, 1:W + 1] = x
    d = np.stack([np.stack([xp[:, a:a + 2 * th:2, b:b + 2 * tw:2] for b in range(4)], 3) for a in range(4)], 3)    # [N, th, tw, 4a, 4b, C]

    def bt(t, ax):
        r = [np.take(t, k, ax) for k in range(4)]
        return np.stack([r[0] - r[2], r[1] + r[2], r[2] - r[1], r[1] - r[3]], ax)
    return bt(bt(d, 3), 4)


class WinoProblem(object):
    """A 3x3 / stride 1 / 'same' layer in the Winograd F(2x2, 3x3) form: out = A^T [sum_c V . U] A scale + shift."""

    def __init__(self, x, w, scale=None, shift=None, whole=None, strata=None):
        self.x, self.w = np.ascontiguousarray(x, F32), np.ascontiguousarray(w, F32)          # NHWC, HWIO
        self.scale = None if scale is None else np.asarray(scale, F32).astype(F64)
        self.shift = None if shift is None else np.asarray(shift, F32).astype(F64)
        N, H, W, self.Cin = self.x.shape
        self.out_shape = (N, H, W, self.w.shape[3])
        self.whole = whole
        self.strata = channel_strata(self.out_shape, whole) if strata is None else strata
        self.K = self.Cin

    @functools.cached_property
    def pieces(self):
        v = wino_V(self.x)
        N, th, tw = v.shape[:3]
        self._tiles = (N, th, tw)
        v = np.ascontiguousarray(np.moveaxis(v.reshape(N * th * tw, 16, self.Cin), 1, 0))     # [16, T, Cin]
        u = wino_U(self.w).reshape(16, self.Cin, -1)                                        # [16, Cin, Cout]
        return split3(v), split3(u)

    def _output(self, m):
        """M [16, T, Cout] -> A^T M A, cropped to the image."""
        N, th, tw = self._tiles
        m = m.reshape(4, 4, N, th, tw, -1)
        r = np.stack([m[0] + m[1] + m[2], m[1] - m[2] - m[3]], 0)                           # A^T over a
        y = np.stack([r[:, 0] + r[:, 1] + r[:, 2], r[:, 1] - r[:, 2] - r[:, 3]], 1)         # [2p, 2q, N, th, tw, Cout]
        y = np.transpose(y, (2, 3, 0, 4, 1, 5)).reshape(N, 2 * th, 2 * tw, -1)
        return y[:, :self.out_shape[1], :self.out_shape[2]]

    @functools.cached_property
    def want(self):
        N, H, W, _ = self.out_shape
        A = im2col(self.x.astype(F64), 3, 3, 1, 1, 1, H, W)
        B = np.transpose(self.w.astype(F64), (3, 0, 1, 2)).reshape(self.out_shape[3], -1)
        return _affine((A @ B.T).reshape(self.out_shape), self.scale, self.shift, None)

    @functools.cached_property
    def D(self):
        v, u = self.pieces
        return {(i, j): _affine(self._output(np.matmul(v[i], u[j])), self.scale, None, None) for i, j in KEPT}

    def emulate(self, drop=None, twice=None, pieces=3):
        v, u = self.pieces
        acc = np.zeros((16, v.shape[2], u.shape[3]), F32)
        todo = products(pieces, drop, twice)
        for k0 in range(0, self.Cin, 16):
            for i, j in todo:
                acc = (acc + np.matmul(v[i][:, :, k0:k0 + 16], u[j][:, k0:k0 + 16])).astype(F32)
        return _affine(self._output(acc).astype(F64), self.scale, self.shift, None).astype(F32)      # (the output transform in fp32)


# ---------------------------------------------------------------------------------------------------------------- the case table

def _rng(name):
    return np.random.default_rng(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


# name: (N, H, W, Cin, Cout, k, stride, pad, res_mode, tile of the split-bf16 kernels, their split-K factor)
CONV = {
    "pw 64x64 tile":        (1, 10, 12, 64, 64, 1, 1, 0, 0, (64, 64), 1),        # 120 pixels: M < 128 -> the 64 x 64 tile, ragged M, two K-tiles
    "3x3 ragged":           (2, 12, 20, 64, 64, 3, 1, 1, 0, (128, 64), 4),       # M = 480 (ragged), borders; 18 K-tiles in four slabs
    "3x3 128-wide":         (2, 64, 64, 64, 128, 3, 1, 1, 1, (128, 128), 4),     # CONV_CASES row 9 of test_gpu_kernels.py
    "pw residual":          (2, 16, 24, 64, 256, 1, 1, 0, 1, (128, 128), 1),
    "3x3 K=4608":           (1, 8, 8, 512, 512, 3, 1, 1, 0, (64, 64), 16),       # split-K slabs
}
STEM = ("stem 7x7/2", (1, 32, 32, 64), (128, 64), 1)
MEAN_PIXEL = (123.7, 116.8, 103.9)
TILES = ("pw tile list", (2, 16, 32, 256, 256), (0, 3, 5, 6))                     # conv2d_tiles: four of the eight 8 x 16-pixel groups

# N, H, W, Cin, Cout
WINO = {
    "one K pair":           (1, 16, 16, 32, 32),
    "two slices":           (2, 12, 20, 64, 64),
    "odd sizes":            (1, 9, 7, 32, 96),
    "four slices":          (1, 24, 40, 64, 128),          # two 64-channel items per group where those are forced, a ragged group column
    "two items per block":  (1, 90, 250, 32, 96),          # 12 x 16 groups x 3 slices = 576 items on 512 persistent blocks
}
WINO_MULTI = "two items per block"
WINO_GROUPS = ("group list", (2, 24, 40, 64, 64), (1, 2, 4, 7, 9, 14, 16))        # 3 x 3 groups per image: seven of eighteen, unordered below
WINO_LEVELS = ("two levels", ((1, 32, 48, 32, 64), (1, 16, 24, 32, 64)), ((0, 2, 5, 7, 10, 11), (1, 2)))

# M, K1, N1, N2
CHAIN = {
    "77 x 64-512-128":       (77, 64, 512, 128),
    "200 x 160-512-128":     (200, 160, 512, 128),
    "1000 x 256-1024-256":   (1000, 256, 1024, 256),
}
CHAIN_STREAM = ("1003 x 64-256-64", (1003, 64, 256, 64))                          # the stream form: fp32 products only, a control


def _conv_operands(name, N, H, W, Cin, Cout, k, res_mode, Ho, Wo):
    rng = _rng(name)
    x = rng.standard_normal((N, H, W, Cin)).astype(F32)
    w = (rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(F32)
    sc, sh = rng.uniform(0.5, 1.5, Cout).astype(F32), rng.standard_normal(Cout).astype(F32)
    res = None
    if res_mode == 1:
        res = rng.standard_normal((N, Ho, Wo, Cout)).astype(F32)
    elif res_mode == 2:
        res = rng.standard_normal((N, Ho // 2, Wo // 2, Cout)).astype(F32)
    return x, w, sc, sh, res


def pack(w):
    """HWIO -> [Cout][kh kw Cin] (packing.pack_conv_kernel, restated: this module imports nothing of the package)."""
    return np.ascontiguousarray(np.transpose(w, (3, 0, 1, 2)).reshape(w.shape[3], -1), dtype=F32)


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """-> (operands dict for the launch, MatrixProblem)."""
    N, H, W, Cin, Cout, k, stride, pad, res_mode, tile, split = CONV[name]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x, w, sc, sh, res = _conv_operands(name, N, H, W, Cin, Cout, k, res_mode, Ho, Wo)
    prob = MatrixProblem(im2col(x, k, k, stride, pad, pad, Ho, Wo), pack(w), sc, sh, res, (N, Ho, Wo, Cout))
    return dict(x=x, w=pack(w), k=k, stride=stride, pad=pad, Ho=Ho, Wo=Wo, scale=sc, shift=sh, residual=res, res_mode=res_mode,
                tile=tile, split_k=split), prob


@functools.lru_cache(maxsize=None)
def stem_case():
    name, (N, H, W, Cout), tile, split = STEM
    rng = _rng(name)
    img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    w = np.zeros((7, 7, 4, Cout), F32)                     # RGBX: the fourth channel is zero in the image and in the kernel
    w[:, :, :3] = rng.standard_normal((7, 7, 3, Cout)) / 12.0
    sc, sh = rng.uniform(0.5, 1.5, Cout).astype(F32), rng.standard_normal(Cout).astype(F32)
    x = np.zeros((N, H, W, 4), F32)
    x[..., :3] = img.astype(F32) - np.asarray(MEAN_PIXEL, F32)                             # mold_rgbx_kernel: one fp32 subtraction
    wp = np.zeros((Cout, 7, 8, 4), F32)                    # packing.pack_stem_kernel: kx padded to 8 taps
    wp[:, :, :7] = np.transpose(w, (3, 0, 1, 2))
    prob = MatrixProblem(im2col(x, 7, 7, 2, 3, 3, H // 2, W // 2), pack(w), sc, sh, None, (N, H // 2, W // 2, Cout))
    return dict(img=img, x=x, w=wp.reshape(Cout, 224), Ho=H // 2, Wo=W // 2, scale=sc, shift=sh, tile=tile, split_k=split), prob


def group_count(H, W):
    """8 x 16-pixel tile groups of one H x W map (dc_conv2d_winograd_group_count)."""
    return (((H + 1) // 2 + 3) // 4) * (((W + 1) // 2 + 7) // 8)


def group_mask(shape, groups):
    """The pixels of the listed 8 x 16-pixel tile groups (image-major, then group row, then group column) of an output [N, H, W, C]."""
    N, H, W, _ = shape
    gy, gx = ((H + 1) // 2 + 3) // 4, ((W + 1) // 2 + 7) // 8
    m = np.zeros(shape, bool)
    for g in groups:
        n, r = divmod(int(g), gy * gx)
        y, x = divmod(r, gx)
        m[n, 8 * y:8 * y + 8, 16 * x:16 * x + 16] = True
    return m


@functools.lru_cache(maxsize=None)
def tiles_case():
    name, (N, H, W, Cin, Cout), groups = TILES
    x, w, sc, sh, res = _conv_operands(name, N, H, W, Cin, Cout, 1, 2, H, W)
    up = np.repeat(np.repeat(res, 2, 1), 2, 2)             # the upsample-add of the FPN lateral layers
    prob = MatrixProblem(x.reshape(-1, Cin), pack(w), sc, sh, up, (N, H, W, Cout), whole=group_mask((N, H, W, Cout), groups))
    return dict(x=x, w=pack(w), scale=sc, shift=sh, residual=res, groups=groups), prob


def wino_item_strata(shape, min_elements=2 * MIN_STRATUM):
    """Every 32-tile x 32-channel work item of a layer with at least min_elements outputs: [((slice, group), mask index)].  (The two-row
    items of a ragged last group row hold 1024 outputs of 256 tiles: the four outputs of a tile share its products, so the D_ij of such an
    item are correlated at the 0.15 level and two dropped products disturb each other's coefficient by as much.)"""
    N, H, W, Cout = shape
    gy, gx = ((H + 1) // 2 + 3) // 4, ((W + 1) // 2 + 7) // 8
    out = []
    for s in range(Cout // 32):
        for g in range(N * gy * gx):
            n, r = divmod(g, gy * gx)
            y, x = divmod(r, gx)
            idx = (n, slice(8 * y, min(H, 8 * y + 8)), slice(16 * x, min(W, 16 * x + 16)), slice(32 * s, 32 * s + 32))
            if (idx[1].stop - idx[1].start) * (idx[2].stop - idx[2].start) * 32 >= min_elements:
                out.append(((s, g), idx))
    return out


def xcd_remap(bid, nblk):
    """dcap_internal.h's remap of a logical id onto the XCDs' shares."""
    q, r, xcd = nblk // 8, nblk % 8, bid % 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + bid // 8


def wino_second_items(shape, blocks=512):
    """The (slice, group) work items of a dense 32-tile / 32-channel launch that a persistent block takes as its SECOND item."""
    N, H, W, Cout = shape
    groups = N * (((H + 1) // 2 + 3) // 4) * (((W + 1) // 2 + 7) // 8)
    total = groups * (Cout // 32)
    return [divmod(xcd_remap(item, total), groups) for item in range(blocks, total)]


def _wino_operands(name, N, H, W, Cin, Cout):
    rng = _rng(name)
    x = rng.standard_normal((N, H, W, Cin)).astype(F32)
    w = (rng.standard_normal((3, 3, Cin, Cout)) / np.sqrt(9 * Cin)).astype(F32)
    return x, w, rng.uniform(0.5, 1.5, Cout).astype(F32), rng.standard_normal(Cout).astype(F32)


@functools.lru_cache(maxsize=None)
def wino_case(name):
    N, H, W, Cin, Cout = WINO[name]
    x, w, sc, sh = _wino_operands(name, N, H, W, Cin, Cout)
    strata = None
    if name == WINO_MULTI:
        strata = [("item slice %d group %d" % sg, idx) for sg, idx in wino_item_strata((N, H, W, Cout))]
    return dict(x=x, w=pack(w), scale=sc, shift=sh, shape=(N, H, W, Cin, Cout)), WinoProblem(x, w, sc, sh, strata=strata)


@functools.lru_cache(maxsize=None)
def wino_groups_case():
    name, (N, H, W, Cin, Cout), groups = WINO_GROUPS
    x, w, sc, sh = _wino_operands(name, N, H, W, Cin, Cout)
    order = [groups[i] for i in _rng(name).permutation(len(groups))]
    prob = WinoProblem(x, w, sc, sh, whole=group_mask((N, H, W, Cout), groups))
    return dict(x=x, w=pack(w), scale=sc, shift=sh, groups=order, shape=(N, H, W, Cin, Cout)), prob


@functools.lru_cache(maxsize=None)
def wino_levels_case():
    name, shapes, lists = WINO_LEVELS
    out = []
    for l, ((N, H, W, Cin, Cout), groups) in enumerate(zip(shapes, lists)):
        x, w, sc, sh = _wino_operands("%s %d" % (name, l), N, H, W, Cin, Cout)
        prob = WinoProblem(x, w, sc, sh, whole=group_mask((N, H, W, Cout), groups))
        out.append((dict(x=x, w=pack(w), scale=sc, shift=sh, groups=list(groups), shape=(N, H, W, Cin, Cout)), prob))
    return out


@functools.lru_cache(maxsize=None)
def chain_operands(name):
    M, K1, N1, N2 = dict(CHAIN, **{CHAIN_STREAM[0]: CHAIN_STREAM[1]})[name]
    rng = _rng(name)
    return dict(x=rng.standard_normal((M, K1)).astype(F32), w1=(rng.standard_normal((N1, K1)) / np.sqrt(K1)).astype(F32),
                w2=(rng.standard_normal((N2, N1)) / np.sqrt(N1)).astype(F32),
                scale1=rng.uniform(0.5, 1.5, N1).astype(F32), shift1=rng.standard_normal(N1).astype(F32),
                scale2=rng.uniform(0.5, 1.5, N2).astype(F32), shift2=rng.standard_normal(N2).astype(F32),
                residual=rng.standard_normal((M, N1)).astype(F32))


@functools.lru_cache(maxsize=None)
def chain_layer1(name):
    o = chain_operands(name)
    return MatrixProblem(o["x"], o["w1"], o["scale1"], o["shift1"], o["residual"])


def chain_layer2(name, y):
    """Layer 2 on the fp32 intermediate `y` the kernel (or the emulation) itself produced: judged on the operand it actually split."""
    o = chain_operands(name)
    return MatrixProblem(y, o["w2"], o["scale2"], o["shift2"])


def all_problems():
    """[(name, problem)] of every case, for the host test of the instrument: the chain's layer 2 on the emulated layer 1."""
    out = [("conv " + n, conv_case(n)[1]) for n in CONV] + [(STEM[0], stem_case()[1]), (TILES[0], tiles_case()[1])]
    out += [("wino " + n, wino_case(n)[1]) for n in WINO] + [("wino " + WINO_GROUPS[0], wino_groups_case()[1])]
    out += [("wino %s %d" % (WINO_LEVELS[0], l), p) for l, (_, p) in enumerate(wino_levels_case())]
    for n in CHAIN:
        p1 = chain_layer1(n)
        out += [("chain %s layer 1" % n, p1), ("chain %s layer 2" % n, chain_layer2(n, p1.emulate()))]
    return out
