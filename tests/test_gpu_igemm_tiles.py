"""The fp32 implicit-GEMM kernels of csrc/igemm_core.h on their 128-row tiles, against the float64 NumPy oracle (-m gpu).

dc_gemm_f32, dc_conv2d_nhwc_f32 (math 0, no Winograd weights) and dc_conv2d_wgrad_f32 each dispatch to 128 x 128, 128 x 64 and 64 x 64
block tiles; choose_tile takes a wide tile only for grids of >= 512 blocks or for K >= 8192 (the priced split-K rule).  The shapes of
test_gpu_kernels.py all resolve to 64 x 64 tiles, so the wide instantiations -- all four GEMM layouts, the weight gradient's
DenseMCT<true> / Im2colMC pair, the stem and im2col loaders on 128 rows, store_tile's row / column tails on a 128 tile, the priced
rule's ragged K slices -- were reached by the whole-model tests alone, at model tolerance.  Every case here FIRST asserts the tile and the
split-K factor the library's own rule reports (info= of the ops wrappers: dc_gemm_tile_config, dc_conv2d_tile_config,
dc_conv2d_wgrad_tile_config), then the values: a shape that silently ran 64 x 64 fails its case.

Tolerances are the sibling tests' (test_gpu_kernels.py): 2e-5 of the output scale for GEMM and forward convolution, 3e-5 for the weight
gradient, with the sibling `close` rule (divisor max(1, max|want|): operands are scaled so that outputs are of order 1 or larger).
Outputs start as NaN, so an element no block stored fails too.  References are computed once per shape and shared."""
import functools

import numpy as np
import pytest
import torch

from oracle import np_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def close(got, want, tol=2e-5):
    got = (got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)).astype(np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    assert err < tol, "max err %.3e (scaled) exceeds %.1e" % (err, tol)


def nan_out(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def ran_on(info, tile, split):
    assert (info["tile"], info["split_k"]) == (tile, split), "the library runs this case on %s tiles, split %d: not the %s / split %d it is here for" % (
        info["tile"], info["split_k"], tile, split)


# ------------------------------------------------------------------------------------------------------------------------------------
# dc_gemm_f32
# ------------------------------------------------------------------------------------------------------------------------------------
# name -> (M, N, K), tile, split.  M and N are no multiples of 128 / 64 (row and column tails on the last tiles) but keep the conditions
# of the fast loaders in every layout: K % 32 == 0, M % 4 == 0 (A transposed), N % 4 == 0 (B not transposed).
GEMM_SHAPES = {
    "128x128": ((2948, 2952, 64), (128, 128), 1),                # 24 x 24 = 576 blocks: fills the chip twice
    "128x64": ((4100, 1000, 96), (128, 64), 1),                  # 33 x 8 = 264 blocks of 128 x 128, 33 x 16 = 528 of 128 x 64
    "128x128-priced": ((388, 324, 8192), (128, 128), 19),        # 256 K-tiles over 19 slices: 18 of 14 and a last one of 4
    "128x64-priced": ((256, 256, 8192), (128, 64), 28),          # launched as 26 slices: 25 of 10 K-tiles and a last one of 6
    "128x64-priced-tails": ((204, 344, 8192), (128, 64), 19),    # ... with a 76-row and a 24-column tail, ragged slices
}
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
LAYOUT_IDS = ["NN", "NT", "TN", "TT"]


@functools.lru_cache(maxsize=None)
def gemm_data(M, N, K):
    """A [M, K], B [K, N] scaled to unit-variance outputs, and A @ B in float64 -- treat as read-only."""
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    A = rng.standard_normal((M, K))
    B = rng.standard_normal((K, N)) / np.sqrt(K)
    return A, B, A @ B


def operands(A, B, ta, tb):
    return dev(A.T if ta else A), dev(B.T if tb else B)


@pytest.mark.parametrize("ta,tb", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", list(GEMM_SHAPES))
def test_gemm_wide_tiles_every_layout(ops, name, ta, tb):
    """Each of the four operand layouts (the A-transposed ones are gemm_tn.hip's instantiations) on each wide tile, unsplit and with the
    priced split; a second call gives the same bits (the slabs are reduced in a fixed order)."""
    (M, N, K), tile, split = GEMM_SHAPES[name]
    A, B, want = gemm_data(M, N, K)
    a, b = operands(A, B, ta, tb)
    info = {}
    got = ops.gemm(a, b, out=nan_out(M, N), a_trans=bool(ta), b_trans=bool(tb), info=info)
    ran_on(info, tile, split)
    close(got, want)
    again = ops.gemm(a, b, out=nan_out(M, N), a_trans=bool(ta), b_trans=bool(tb))
    assert torch.equal(got, again)


# the shapes whose epilogue runs in the tile itself (store_tile; a split launch finishes in the slab reducer, whatever its tile)
UNSPLIT = [("128x128", 0, 1), ("128x64", 1, 0)]
UNSPLIT_IDS = ["128x128-NT", "128x64-TN"]


@pytest.mark.parametrize("name,ta,tb", UNSPLIT, ids=UNSPLIT_IDS)
def test_gemm_wide_tile_full_epilogue(ops, name, ta, tb):
    """scale, shift, residual, ReLU and accumulate at once, through store_tile's 16-byte path with its row-group prefetch."""
    (M, N, K), tile, split = GEMM_SHAPES[name]
    A, B, AB = gemm_data(M, N, K)
    rng = np.random.default_rng(101 + M)
    sc, sh = rng.uniform(0.5, 1.5, N), rng.standard_normal(N)
    R, C0 = rng.standard_normal((M, N)), rng.standard_normal((M, N))
    a, b = operands(A, B, ta, tb)
    out, info = dev(C0), {}
    ops.gemm(a, b, out=out, a_trans=bool(ta), b_trans=bool(tb), scale=dev(sc), shift=dev(sh), residual=dev(R), relu=True, accumulate=True, info=info)
    ran_on(info, tile, split)
    close(out, np.maximum(AB * sc + sh + R, 0) + C0)


@pytest.mark.parametrize("name,ta,tb", UNSPLIT, ids=UNSPLIT_IDS)
def test_gemm_wide_tile_per_roi_residual(ops, name, ta, tb):
    """res_rows: output row m takes residual row m % res_rows (a per-RoI term broadcast over timesteps), 67 rows against 128-row tiles."""
    (M, N, K), tile, split = GEMM_SHAPES[name]
    A, B, AB = gemm_data(M, N, K)
    R = np.random.default_rng(102 + M).standard_normal((67, N))
    a, b = operands(A, B, ta, tb)
    info = {}
    got = ops.gemm(a, b, out=nan_out(M, N), a_trans=bool(ta), b_trans=bool(tb), residual=dev(R), res_rows=67, info=info)
    ran_on(info, tile, split)
    close(got, AB + R[np.arange(M) % 67])


@pytest.mark.parametrize("name,ta,tb", [("128x128", 0, 0), ("128x64", 0, 1), ("128x128", 1, 0), ("128x64", 1, 1)],
                         ids=["128x128-NN", "128x64-NT", "128x128-TN", "128x64-TT"])
def test_gemm_wide_tile_row_gather_on_a(ops, name, ta, tb):
    """a_gather: tile row m is table row gather[m] (A not transposed: the embedding lookup); with A transposed, K row k is table row
    gather[k].  The table holds A's rows shuffled among rows of NaN, so a row fetched from the wrong place poisons the output."""
    (M, N, K), tile, split = GEMM_SHAPES[name]
    A, B, AB = gemm_data(M, N, K)
    rows = A.T if ta else A                                    # the rows the gather picks: [K, M] or [M, K]
    rng = np.random.default_rng(103 + M + ta)
    ids = rng.permutation(rows.shape[0] + 50)[:rows.shape[0]]
    table = np.full((rows.shape[0] + 50, rows.shape[1]), np.nan)
    table[ids] = rows
    info = {}
    got = ops.gemm(dev(table), dev(B.T if tb else B), out=nan_out(M, N), a_trans=bool(ta), b_trans=bool(tb), gather=dev(ids, torch.int32), info=info)
    ran_on(info, tile, split)
    close(got, AB)


@pytest.mark.parametrize("name,ta,tb", UNSPLIT, ids=UNSPLIT_IDS)
@pytest.mark.parametrize("c_off", [8, 2], ids=["C-aligned", "C-unaligned"])
def test_gemm_wide_tile_row_strided_views(ops, name, ta, tb, c_off):
    """A, B and C as column ranges of wider tensors (leading dimensions larger than the rows).  C 16-byte aligned: the vector epilogue;
    C at a column offset of 2: the scalar epilogue with its per-element column bound.  The columns beside C stay untouched."""
    (M, N, K), tile, split = GEMM_SHAPES[name]
    A, B, AB = gemm_data(M, N, K)
    As, Bs = (A.T if ta else A), (B.T if tb else B)
    wa = torch.full((As.shape[0], As.shape[1] + 24), float("nan"), device="cuda")
    wb = torch.full((Bs.shape[0], Bs.shape[1] + 12), float("nan"), device="cuda")
    wa[:, 16:16 + As.shape[1]] = dev(As)
    wb[:, 4:4 + Bs.shape[1]] = dev(Bs)
    wide = torch.full((M, N + 20), 7.0, device="cuda")
    info = {}
    ops.gemm(wa[:, 16:16 + As.shape[1]], wb[:, 4:4 + Bs.shape[1]], out=wide[:, c_off:c_off + N], a_trans=bool(ta), b_trans=bool(tb), info=info)
    ran_on(info, tile, split)
    close(wide[:, c_off:c_off + N], AB)
    assert bool((wide[:, :c_off] == 7.0).all()) and bool((wide[:, c_off + N:] == 7.0).all())


@pytest.mark.parametrize("name,ta,tb,force", [("128x128", 0, 0, 2), ("128x64", 1, 1, 3)], ids=["128x128-NN-2", "128x64-TT-3"])
def test_gemm_wide_tile_forced_split(ops, name, ta, tb, force):
    """A caller's split_k on a grid that fills the chip keeps the wide tile: one K-tile per slice (K = 64 in two, K = 96 in three), every
    slice written to its slab through store_tile's partial path, the epilogue applied by the reducer."""
    (M, N, K), tile, _ = GEMM_SHAPES[name]
    assert K == 32 * force
    A, B, AB = gemm_data(M, N, K)
    sh = np.random.default_rng(104 + M).standard_normal(N)
    a, b = operands(A, B, ta, tb)
    info = {}
    got = ops.gemm(a, b, out=nan_out(M, N), a_trans=bool(ta), b_trans=bool(tb), shift=dev(sh), relu=True, split_k=force, info=info)
    ran_on(info, tile, force)
    close(got, np.maximum(AB + sh, 0))


@pytest.mark.parametrize("ta,tb", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", ["128x128-priced", "128x64-priced-tails"])
def test_gemm_wide_tile_bulk_with_k_tail_launch(ops, name, ta, tb):
    """K = 8192 + 8: the first 8192 columns run on the wide tile with the priced split (dc_gemm_tile_config answers for that launch), the
    last 8 are accumulated onto its result by one launch of the range-checked kernel."""
    (M, N, K), tile, split = GEMM_SHAPES[name]
    A, B, AB = gemm_data(M, N, K + 8)
    sh = np.random.default_rng(105 + M).standard_normal(N)
    a, b = operands(A, B, ta, tb)
    info = {}
    got = ops.gemm(a, b, out=nan_out(M, N), a_trans=bool(ta), b_trans=bool(tb), shift=dev(sh), info=info)
    ran_on(info, tile, split)
    close(got, AB + sh)
    # the tail is worth finding: without it the result is off by far more than the tolerance
    assert float(np.abs(A[:, K:] @ B[K:]).max()) > 1e-3


# ------------------------------------------------------------------------------------------------------------------------------------
# dc_conv2d_wgrad_f32
# ------------------------------------------------------------------------------------------------------------------------------------
def same_pads(H, W, k, stride):
    return O.same_pad(H, k, stride), O.same_pad(W, k, stride)


# name -> (N, H, W, Cin, Cout, k, stride), (pad_t, pad_b, pad_l, pad_r) or None for TF 'SAME', tile, split
WGRAD_CASES = {
    # three images, non-square, a Cout tail of 8 rows; K = 8736 pixels = 273 K-tiles over the priced split
    "128x128-priced": ((3, 56, 52, 128, 136, 3, 1), None, (128, 128), 28),
    "128x64-priced": ((1, 100, 96, 256, 200, 1, 1), None, (128, 64), 28),
    # the grids that fill the chip without a split (8 x 72 = 576 and 29 x 18 = 522 blocks).  Such a grid needs 512 x 128 x 128 (x 64)
    # gradient elements, so these are the large cases; 1024 pixels in two images whose 32-pixel rows equal the K-tile
    "128x128": ((2, 16, 32, 1024, 904, 3, 1), None, (128, 128), 1),
    "128x64": ((2, 16, 32, 128, 3588, 3, 1), None, (128, 64), 1),
    # 16560 pixels = 16 mod 32: the wide tiles have no range-checked loader, so the rule falls back to 64 x 64 at long K, split
    "ragged-pixels": ((2, 90, 92, 128, 128, 3, 1), None, (64, 64), 15),
    "stem": ((1, 72, 88, 64, 64, 7, 2), (3, 3, 3, 3), (64, 64), 11),             # the stem's geometry on its 64 padded channels, non-square
    "1x1-stride2": ((2, 30, 44, 128, 132, 1, 2), (0, 0, 0, 0), (64, 64), 5),     # two images of 330 output pixels each
    "3x3-stride2": ((2, 40, 35, 64, 72, 3, 2), None, (64, 64), 5),               # 'SAME' paddings (0, 1) x (1, 1): top differs from left
    # Wo = 7 < 32: the incremental (ox, oy, n) walk wraps several rows per K-tile and crosses both image boundaries
    "narrow": ((3, 5, 7, 64, 68, 3, 1), None, (64, 64), 1),
}


@functools.lru_cache(maxsize=None)
def wgrad_data(name):
    """x, dy, the paddings and the packed float64 weight gradient of a WGRAD_CASES entry -- treat as read-only."""
    from image_captioning_amd.packing import pack_conv_kernel
    (N, H, W, Cin, Cout, k, stride), pads, _, _ = WGRAD_CASES[name]
    if pads is None:
        (pt, pb), (pl, pr) = same_pads(H, W, k, stride)
        pads = (pt, pb, pl, pr)
    pt, pb, pl, pr = pads
    Ho, Wo = (H + pt + pb - k) // stride + 1, (W + pl + pr - k) // stride + 1
    rng = np.random.default_rng(sum(WGRAD_CASES[name][0]) + len(name))
    x, dy = rng.standard_normal((N, H, W, Cin)), rng.standard_normal((N, Ho, Wo, Cout))
    _, dw, _ = O.conv2d_nhwc_backward(x, np.zeros((k, k, Cin, Cout)), dy, stride, pads)
    return x, dy, (pt, pl), pack_conv_kernel(dw)


@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_wgrad_tiles_and_geometries(ops, name):
    (N, H, W, Cin, Cout, k, stride), _, tile, split = WGRAD_CASES[name]
    x, dy, (pt, pl), want = wgrad_data(name)
    info = {}
    got = ops.conv2d_wgrad(dev(x), dev(dy), k, k, stride, pt, pl, out=nan_out(*want.shape), info=info)
    ran_on(info, tile, split)
    close(got, want, 3e-5)


# a caller's split_k switches the priced rule off, so only a grid that fills the chip keeps its wide tile under a forced split
@pytest.mark.parametrize("force", [1, 5, 32])
@pytest.mark.parametrize("name", ["128x128", "128x64"])
def test_wgrad_wide_tile_forced_split(ops, name, force):
    """32 K-tiles of pixels in 1 slice, in 5 (four of 7 K-tiles and one of 4) and in 32 of one K-tile each: every slice decodes its first
    pixel anew (Im2colMC's one division per block) and the slices meet image 1 at different places."""
    (N, H, W, Cin, Cout, k, stride), _, tile, _ = WGRAD_CASES[name]
    x, dy, (pt, pl), want = wgrad_data(name)
    info = {}
    got = ops.conv2d_wgrad(dev(x), dev(dy), k, k, stride, pt, pl, out=nan_out(*want.shape), split_k=force, info=info)
    ran_on(info, tile, force)
    close(got, want, 3e-5)


@pytest.mark.parametrize("name", ["128x128", "128x64", "128x128-priced", "128x64-priced"])
def test_wgrad_wide_tile_accumulates_and_repeats(ops, name):
    """accumulate=True onto a random base (in the tile's epilogue where unsplit, in the slab reducer where split); two plain calls give
    the same bits."""
    (N, H, W, Cin, Cout, k, stride), _, tile, split = WGRAD_CASES[name]
    x, dy, (pt, pl), want = wgrad_data(name)
    base = np.random.default_rng(106 + Cout).standard_normal(want.shape) * np.abs(want).max()
    xd, dyd = dev(x), dev(dy)
    out, info = dev(base), {}
    ops.conv2d_wgrad(xd, dyd, k, k, stride, pt, pl, out=out, accumulate=True, info=info)
    ran_on(info, tile, split)
    close(out, base + want, 3e-5)
    first = ops.conv2d_wgrad(xd, dyd, k, k, stride, pt, pl, out=nan_out(*want.shape))
    again = ops.conv2d_wgrad(xd, dyd, k, k, stride, pt, pl, out=nan_out(*want.shape))
    assert torch.equal(first, again)
    close(first, want, 3e-5)


# ------------------------------------------------------------------------------------------------------------------------------------
# dc_conv2d_nhwc_f32, math 0, no Winograd weights
# ------------------------------------------------------------------------------------------------------------------------------------
PC_128x64 = "igemm_pc_kernel<128, 64, dcap::Im2colKCT<false>, dcap::DenseKCT<true> >"
# (N, H, W, Cin, Cout, k, stride), epilogue, tile, split, kernel
CONV_TILE_CASES = {
    # 64 x 9 = 576 blocks of 128 x 64, the last column tile 8 wide; K = 576 >= 128 and Cout >= 128: the producer / consumer kernel
    "128x64-pc": ((2, 64, 64, 64, 520, 3, 1), True, (128, 64), 1, PC_128x64),
    # 32 x 16 = 512 blocks; K = 64 < 128 keeps it on the single-role kernel (and stride 2 off the pointwise kernels)
    "128x128": ((1, 128, 128, 64, 2048, 1, 2), False, (128, 128), 1, "igemm_kernel<128, 128, dcap::Im2colKCT<false>, dcap::DenseKCT<true> >"),
    # ... with a 127-row tail (63 x 65 output pixels of a non-square map) and a 4-column tail on a seventeenth column tile
    "128x128-tails": ((1, 126, 130, 64, 2052, 1, 2), True, (128, 128), 1, "igemm_kernel<128, 128, dcap::Im2colKCT<false>, dcap::DenseKCT<true> >"),
    "128x64": ((1, 256, 256, 64, 64, 3, 1), False, (128, 64), 1, "igemm_kernel<128, 64, dcap::Im2colKCT<false>, dcap::DenseKCT<true> >"),
    # M = 240 pixels, K = 9216: the priced split on 128-row tiles with a 112-row and an 8-column tail
    "128x64-priced": ((1, 12, 20, 1024, 200, 3, 1), True, (128, 64), 28, "igemm_kernel<128, 64, dcap::Im2colKCT<false>, dcap::DenseKCT<true> >"),
}


@pytest.mark.parametrize("name", list(CONV_TILE_CASES))
def test_conv2d_f32_wide_tiles(ops, name):
    """epilogue: frozen-BN scale and shift, a residual of the output's shape and ReLU; otherwise the bare convolution."""
    from image_captioning_amd.packing import pack_conv_kernel
    (N, H, W, Cin, Cout, k, stride), epilogue, tile, split, kernel = CONV_TILE_CASES[name]
    rng = np.random.default_rng(N + H * 3 + W * 5 + Cin * 7 + Cout * 11 + k)
    x = rng.standard_normal((N, H, W, Cin))
    w = rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)
    padding = 'same' if k == 3 else 'valid'
    y = O.conv2d_nhwc(x, w, None, stride, padding)
    Ho, Wo = y.shape[1:3]
    sc = sh = res = None
    if epilogue:
        sc, sh, res = rng.uniform(0.5, 1.5, Cout), rng.standard_normal(Cout), rng.standard_normal(y.shape)
        y = np.maximum(y * sc + sh + res, 0)
    pt, pl = (O.same_pad(H, k, stride)[0], O.same_pad(W, k, stride)[0]) if padding == 'same' else (0, 0)
    info = {}
    got = ops.conv2d(dev(x), dev(pack_conv_kernel(w)), k, k, stride, pt, pl, Ho, Wo, None if sc is None else dev(sc), None if sh is None else dev(sh),
                     None if res is None else dev(res), 1 if epilogue else 0, epilogue, out=nan_out(N, Ho, Wo, Cout), info=info)
    ran_on(info, tile, split)
    assert info["kernel"] == kernel
    close(got, y)


def test_stem_wide_tile_ragged_last_row_tile(ops):
    """The 7x7 / stride 2 stem on one 520 x 504 image, through mold_image_rgbx and pack_stem_kernel as the encoder drives it: 65520
    output pixels = 511 row tiles of 128 and one of 112, on StemKC's loader."""
    from image_captioning_amd.packing import pack_stem_kernel
    H, W = 520, 504
    rng = np.random.default_rng(H + W)
    img = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    mean = [123.7, 116.8, 103.9]
    w = rng.standard_normal((7, 7, 3, 64)) / 12.0
    sc, sh = rng.uniform(0.5, 1.5, 64), rng.standard_normal(64)
    y = np.maximum(O.conv2d_nhwc(O.mold_image(img, mean), w, None, 2, (3, 3, 3, 3)) * sc + sh, 0)
    rgbx = ops.mold_image_rgbx(dev(img, torch.uint8), mean)
    info = {}
    got = ops.conv2d(rgbx, dev(pack_stem_kernel(w)), 7, 7, 2, 3, 3, H // 2, W // 2, dev(sc), dev(sh), None, 0, True, out=nan_out(1, H // 2, W // 2, 64), info=info)
    ran_on(info, (128, 64), 1)
    assert info["kernel"] == "igemm_kernel<128, 64, dcap::StemKC, dcap::DenseKCT<true> >"
    close(got, y)


def test_data_gradient_as_forward_conv_accumulates_in_place_on_a_wide_tile(ops):
    """The data gradient of a 3x3 / stride 1 'same' convolution as the encoder's backward pass runs it: the forward kernel on dy with the
    rotated, transposed kernel (pack_conv_kernel_dgrad), res_mode 1 with the residual ALIASING the output (the gradient map already
    holds another path's contribution).  16560 pixels x 256 channels: 130 x 4 blocks of 128 x 64, the last row tile 48 rows."""
    from image_captioning_amd.packing import pack_conv_kernel_dgrad
    N, H, W, Cin, Cout, k = 2, 92, 90, 256, 64, 3
    rng = np.random.default_rng(107)
    x = np.zeros((N, H, W, Cin))
    w = rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cout)
    dy = rng.standard_normal((N, H, W, Cout))
    dx, _, _ = O.conv2d_nhwc_backward(x, w, dy, 1, 'same')
    held = rng.standard_normal(dx.shape)
    out, info = dev(held), {}
    ops.conv2d(dev(dy), dev(pack_conv_kernel_dgrad(w)), k, k, 1, 1, 1, H, W, residual=out, res_mode=1, out=out, info=info)
    ran_on(info, (128, 64), 1)
    assert info["kernel"] == PC_128x64
    close(out, held + dx)
