"""The bf16 matrix kernels on binary-grid operands: the case tables tests/test_gpu_bf16_exact.py runs on the device and
tests/test_bf16_exact_cases.py proves on the host.  Plain module, no fixtures; torch and the package are imported nowhere here (the
device side lives in the GPU test file), so importing it needs neither a GPU nor the built library.

dc_gemm_bf16, dc_conv2d_bf16 and dc_conv2d_wgrad_bf16 run seven MFMA kernels between them (KERNELS).  tests/test_gpu_bf16.py holds them
by tolerance on standard-normal operands: a single product lost, doubled or taken from the wrong k hides below 3e-5 of the output scale,
and a bf16 output that rounds ties away from zero -- or truncates, anywhere below the largest element's binade -- hides below 2^-8 of the
LARGEST element.  Here the operands are the grids
of tests/_placement_cases.py (A / x in steps of 1/8 within +-1, B / w / dy in steps of 1/256 within +-1/16, the epilogue operands on
grids as well), at the shapes where the kernels' main, vectorised paths run: full tiles, ragged edges, K tails, split-K slabs, gathers
and every tile size.

THE EXACTNESS BOUND.  A product is a multiple of 2^-11 of magnitude at most 1/16, so a sum of K of them -- the whole sum, any partial
sum in any order, any split-K slab -- is a multiple of 2^-11 below K / 16: exact in fp32's 24 bits while K / 16 / 2^-11 < 2^24, that is
K < 2^17 (K_LIMIT; for the weight gradient K is the pixel count N Ho Wo).  The epilogue (scale from {1/2, 1, 2}, shift in steps of 2^-11,
residual and accumulate base in steps of 1/8 within +-4) keeps every stage a multiple of 2^-12 below 2^12: _placement_cases.epilogue()
asserts each stage.  So the fp32 output of a correct kernel EQUALS the float64 result (`want`), and its bf16 output equals bf16_of(want),
the round-to-nearest-even of that value -- no tolerance.  A large share of the values are exact bf16 ties (low 16 bits 0x8000), about
half of them on either side of round-to-even (tie_shares): truncation, ties-away and round-half-up each show on many elements per case.

One cache per case (functools.lru_cache): computed once, never mutated -- every array handed out is read-only."""
import functools

import numpy as np

import _placement_cases as P
from _split_cases import im2col

F32, F64 = np.float32, np.float64
K_LIMIT = 1 << 17
TIE_SHARE = 0.01                  # of a bf16 output's elements: exact ties that round up, and as many that round down to even

# kernel -> the mechanisms it has, each of which some leg of the tables must reach (test_bf16_exact_cases.py).
#   "k tail": K % 64 != 0.  The convolution forward kernels have none (dc_conv2d_bf16 wants Cin % 64 == 0: a K-tile is 64 channels of
#   one tap); their nearest edge is an odd number of K-tiles per slice, the main loops running K-tiles in pairs ("odd k tiles").
#   bconv64_kernel runs the whole K loop in one block (no slabs); the weight gradient has no bf16 output.
KERNELS = {
    "bgemm_kernel":          {"slabs", "no slabs", "k tail", "ragged", "bf16 only"},
    "bgemm256_kernel":       {"slabs", "no slabs", "k tail", "ragged", "bf16 only"},
    "bconv64_kernel":        {"no slabs", "odd k tiles", "ragged", "bf16 only"},
    "bconv_kernel":          {"slabs", "no slabs", "odd k tiles", "ragged", "bf16 only"},
    "bconv256_kernel":       {"slabs", "no slabs", "odd k tiles", "ragged", "bf16 only"},
    "bgemm_wgrad_kernel":    {"slabs", "no slabs", "k tail", "ragged"},
    "bgemm256_wgrad_kernel": {"slabs", "no slabs", "k tail", "ragged"},
}
GEMM_KERNEL = {128: "bgemm_kernel", 256: "bgemm256_kernel"}
CONV_KERNEL = {64: "bconv64_kernel", 128: "bconv_kernel", 256: "bconv256_kernel"}
WGRAD_KERNEL = {128: "bgemm_wgrad_kernel", 256: "bgemm256_wgrad_kernel"}

LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]          # (a_trans, b_trans)


def _seed(*key):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(repr(key)))


def _frozen(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _mechanisms(M, N, K, tile, slices, outs=()):
    """What one launch of an M x N x K problem on `tile` in `slices` split-K slabs reaches, from the numbers alone."""
    ktiles = -(-K // 64)
    per_slice = -(-ktiles // slices)
    m = {"slabs" if slices > 1 else "no slabs"}
    if K % 64:
        m.add("k tail")
    if per_slice % 2 or (ktiles - per_slice * (slices - 1)) % 2:
        m.add("odd k tiles")
    if M % tile or N % tile:
        m.add("ragged")
    if "bf16" in outs:
        m.add("bf16 only")
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_gemm_bf16.  (M, N, K, split_k asked for, tile, slices): tile and slices are what the library reports for the launch
# (ops.gemm_bf16's info) -- the 256 rows as test_gemm_bf16_256_tile_layouts asserts them, the others as the 128-square kernel's own
# bgemm_split gives them; asserted on the device, so that a cost-model change cannot silently move a case off its kernel.

GEMM_PLAIN = [
    # the 128-square tile
    (264, 136, 72, 0, 128, 1),          # ragged M and N, one short K-tile pair (64 + 8)
    (200, 1024, 1024, 0, 128, 4),
    (8, 1000, 512, 0, 128, 2),
    (1024, 2048, 3000, 0, 128, 4),      # a K tail: 3000 % 64 = 56
    (200, 1024, 3136, 0, 128, 10),      # 49 K-tiles in slabs of 5: the last one short
    (200, 1024, 3136, 1, 128, 1),
    (200, 1024, 3136, 3, 128, 3),
    (200, 1024, 3136, 7, 128, 7),
    # the 256-square tile
    (3000, 4104, 200, 0, 256, 1),       # ragged M and N, a K tail (3 x 64 + 8)
    (1024, 1024, 8192, 16, 256, 16),    # slabs on request
    (3072, 4096, 512, 0, 256, 1),       # exact tiling
    (4096, 3072, 72, 0, 256, 1),        # one short K-tile pair
]

# The full epilogue -- scale, shift, residual ("full": [M, N]; an integer r: [r, N], row m % r), relu, accumulate -- on one shape per
# tile, without slabs (the epilogue runs in the main kernel's store) and with them (in splitk_reduce_kernel).
# (M, N, K, residual, split_k asked for, tile, slices)
GEMM_EPILOGUE = [
    (200, 1024, 3136, "full", 1, 128, 1),
    (200, 1024, 3136, 40, 0, 128, 10),
    (3072, 4096, 512, 768, 0, 256, 1),
    (1024, 1024, 8192, "full", 16, 256, 16),
]
# fp32 alone and fp32 + bf16 accumulate into C0; bf16 alone (C null: Epilogue::put's other branch, the path the bf16 model runs between
# consecutive layers) cannot -- dc_gemm_bf16 refuses accumulate without C
GEMM_OUTS = ["f32", "both", "bf16"]

# test_gemm_bf16_gather_rows_and_k's sizes: V table rows of E = 300 columns padded with zeros to Ep = 304, N ids, U outputs
GATHER = dict(V=1000, E=300, Ep=304, N=960, U=512)
GATHER_LEGS = [("rows", 960, 512, 304, 128, 1), ("k", 304, 512, 960, 128, 3)]      # (which, M, N, K, tile, slices)
# test_gemm_bf16_per_roi_residual_and_strided_views' sizes: B is the view W[64:, :N] of a [K + 64, N + 8] matrix
STRIDED = dict(Bn=24, T=5, K=512, N=256, tile=128, slices=2)


@functools.lru_cache(maxsize=None)
def gemm_plain(M, N, K):
    """A [M, K], B [K, N], want = A B (no epilogue); the splits of one shape share it."""
    assert K < K_LIMIT
    c = P.gemm_case(_seed("gemm", M, N, K), M, N, K, scale=False, shift=False, residual=None, relu=False, accumulate=False)
    c["want_bf16"] = P.bf16_of(c["want"])
    return _frozen(c)


@functools.lru_cache(maxsize=None)
def gemm_epilogue(M, N, K, residual):
    """P.gemm_case with the full epilogue but the accumulate: want = relu((A B scale + shift) + residual), what the bf16-only leg
    computes; C0 and want_acc = want + C0 for the legs with an fp32 output."""
    assert K < K_LIMIT
    c = P.gemm_case(_seed("gemm epilogue", M, N, K, residual), M, N, K, residual=residual, accumulate=False)
    c["C0"] = P.grid(np.random.default_rng(_seed("C0", M, N, K, residual)), (M, N), 1 / 8, 4.0)
    c["want_acc"] = P.epilogue(c["want"], base=c["C0"])
    c["want_bf16"], c["want_acc_bf16"] = P.bf16_of(c["want"]), P.bf16_of(c["want_acc"])
    return _frozen(c)


@functools.lru_cache(maxsize=None)
def gather_case():
    """table [V, Ep] (columns E.. zero), ids [N], W [Ep, U] (rows E.. zero), dz [N, U]:
    rows: table[ids] W [N, U];  k: table[ids]^T dz [Ep, U], rows E.. zero."""
    g = GATHER
    rng = np.random.default_rng(_seed("gather"))
    table = np.zeros((g["V"], g["Ep"]))
    table[:, :g["E"]] = P.grid(rng, (g["V"], g["E"]), 1 / 8, 1.0)
    W = np.zeros((g["Ep"], g["U"]))
    W[:g["E"]] = P.grid(rng, (g["E"], g["U"]), 1 / 256, 1 / 16)
    ids = rng.integers(0, g["V"], g["N"]).astype(np.int32)
    dz = P.grid(rng, (g["N"], g["U"]), 1 / 256, 1 / 16)
    c = {"table": table, "ids": ids, "W": W, "dz": dz}
    c["want_rows"] = P.epilogue(table[ids] @ W)
    c["want_k"] = P.epilogue(table[ids].T @ dz)
    assert not c["want_k"][g["E"]:].any()
    c["want_rows_bf16"], c["want_k_bf16"] = P.bf16_of(c["want_rows"]), P.bf16_of(c["want_k"])
    return _frozen(c)


@functools.lru_cache(maxsize=None)
def strided_case():
    """X [T Bn, K], the whole W [K + 64, N + 8] (B = W[64:, :N]), r [Bn, N]: want = X B + r[m % Bn]."""
    s = STRIDED
    rng = np.random.default_rng(_seed("strided"))
    X = P.grid(rng, (s["T"] * s["Bn"], s["K"]), 1 / 8, 1.0)
    W = P.grid(rng, (s["K"] + 64, s["N"] + 8), 1 / 256, 1 / 16)
    r = P.grid(rng, (s["Bn"], s["N"]), 1 / 8, 4.0)
    c = {"X": X, "W": W, "r": r, "want": P.epilogue(X @ W[64:, :s["N"]], residual=np.tile(r, (s["T"], 1)))}
    c["want_bf16"] = P.bf16_of(c["want"])
    return _frozen(c)


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_conv2d_bf16.  The rows of BCONV_CASES, BCONV_BIG and BCONV_SMALL of tests/test_gpu_bf16.py, copied as data:
# (N, H, W, Cin, Cout, k, stride, res_mode, relu), 'same' padding for the 3 x 3 rows and none for the 1 x 1 ones as there (P.conv_case's
# rule).  Each row keeps its own residual mode; between them the rows run modes 0, 1 and 2 on every tile.
# slabs: forced tile -> split-K slices the library reports there (1 where absent): the 128- and 256-square kernels' own rules, or the 16
# the Cin = 1024 3 x 3 row asks for as in the existing test.

CONV_ROWS = {
    # BCONV_CASES
    "pw 64-64":            ((1, 16, 16, 64, 64, 1, 1, 0, True), {}),
    "pw 64-256 res":       ((2, 16, 24, 64, 256, 1, 1, 1, True), {}),
    "pw stride 2":         ((1, 32, 32, 256, 128, 1, 2, 0, True), {}),                    # strided 1x1 (stage-entry branches)
    "3x3 ragged":          ((2, 12, 20, 64, 64, 3, 1, 0, True), {128: 2}),                # ragged pixel count (480), borders
    "3x3 128-128":         ((1, 16, 16, 128, 128, 3, 1, 0, False), {128: 4, 256: 2}),
    "3x3 K=4608":          ((1, 8, 8, 512, 512, 3, 1, 0, True), {128: 18, 256: 9}),       # small M, long K: split-K
    "pw upsample-add":     ((1, 16, 16, 256, 256, 1, 1, 2, False), {}),                   # FPN lateral + upsample-add
    "pw Cout 20":          ((2, 9, 7, 128, 20, 1, 1, 0, False), {}),                      # the padded RPN head: 126 pixels, Cout = 20
    "3x3 Cout 192":        ((1, 40, 40, 64, 192, 3, 1, 1, True), {128: 2}),               # two column tiles, the second partial
    # BCONV_BIG: the 256 x 256 tile (grids of >= 192 tiles)
    "3x3 big ragged":      ((1, 128, 135, 64, 768, 3, 1, 1, True), {}),                   # 68 x 3 tiles, ragged pixel count, borders, residual
    "pw big Cout 712":     ((2, 96, 128, 128, 712, 1, 1, 2, False), {}),                  # the third column tile 200 wide, upsample-add
    "3x3 K=9216":          ((1, 64, 64, 1024, 256, 3, 1, 0, True), {128: 16, 256: 16}),   # split_k = 16 asked for (not on the 64 tile)
    # BCONV_SMALL: the 64 x 64 tile (whole K loop per block)
    "3x3 res4 2b":         ((1, 64, 64, 256, 256, 3, 1, 0, True), {128: 8, 256: 4}),      # 36 K-tiles through the four-stage ring
    "pw res4 2a":          ((1, 64, 64, 1024, 256, 1, 1, 1, True), {128: 4, 256: 2}),
    "3x3 Cout 320":        ((1, 32, 32, 512, 320, 3, 1, 0, False), {128: 18, 256: 9}),    # 72 K-tiles, ragged columns
}
CONV_ASKS_16 = "3x3 K=9216"
# the library's own choice (tile = 0), where test_conv2d_bf16_matches_oracle asserts one
CONV_OWN_TILE = {"3x3 big ragged": 256, "pw big Cout 712": 256, "3x3 res4 2b": 64, "pw res4 2a": 64}
CONV_TILES = [0, 64, 128, 256]
CONV_OUTS = ["both", "bf16"]          # (fp32 alone adds nothing beyond `both` here)


def conv_geometry(name):
    """(M, N, K) of the implicit GEMM and (Ho, Wo)."""
    N, H, W, Cin, Cout, k, stride, _, _ = CONV_ROWS[name][0]
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return N * Ho * Wo, Cout, k * k * Cin, Ho, Wo


def conv_granted(name, tile):
    """The tile dc_conv2d_bf16_tile grants a forced one (test_conv2d_bf16_matches_oracle's rule): a sliver of one 256-square tile is
    refused and runs on the 128-square one."""
    M, Cout, _, _, _ = conv_geometry(name)
    if tile == 256 and M * Cout * 4 < -(-M // 256) * -(-Cout // 256) * 65536:
        return 128
    return tile


def conv_split_k(name, tile):
    """The split_k the call asks for: 16 on the Cin = 1024 3 x 3 row (the cost model would not split that shape), not on the 64 tile."""
    return 16 if name == CONV_ASKS_16 and tile != 64 else 0


@functools.lru_cache(maxsize=None)
def conv_case(name):
    N, H, W, Cin, Cout, k, stride, res_mode, relu = CONV_ROWS[name][0]
    assert k * k * Cin < K_LIMIT
    c = P.conv_case(_seed("conv", name), N, H, W, Cin, Cout, k, stride, res_mode=res_mode, relu=relu)
    c["want_bf16"] = P.bf16_of(c["want"])
    return _frozen(c)


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_conv2d_wgrad_bf16.  The eight rows of test_conv2d_wgrad_bf16_matches_oracle: (N, H, W, Cin, Cout, k, stride), tile, slices as
# the library reports them (the 256 tile from H >= 96 on, as asserted there); 'same' padding for 3 x 3.  Every one of those rows that
# reaches the 256-square kernel has a pixel count that is a multiple of 64 and runs in slabs, so two more rows -- this file's own -- give
# that kernel its K tail, under slabs (9504 = 148 x 64 + 32 pixels) and without (136 = 2 x 64 + 8: Cin = 2048 makes 144 tiles of 256,
# too many to split; the pixel count selects the mechanism, the channel counts the tile).

WGRAD_ROWS = {
    "3x3 128-64":          ((1, 16, 16, 128, 64, 3, 1), 128, 1),
    "3x3 ragged pixels":   ((2, 12, 20, 256, 256, 3, 1), 128, 2),        # pixel count not a multiple of the 64-deep K-tile
    "3x3 256-512":         ((1, 32, 32, 256, 512, 3, 1), 128, 4),        # automatic split-K over the pixels
    "pw lateral":          ((2, 8, 8, 1024, 256, 1, 1), 128, 1),         # an FPN lateral
    "3x3 P6":              ((1, 2, 2, 256, 256, 3, 1), 128, 1),          # a P6-sized level: every tap partly outside
    "3x3 P3 rpn":          ((1, 128, 128, 256, 512, 3, 1), 256, 14),     # the 256-square tile: one tap per column tile
    "3x3 two taps":        ((1, 96, 100, 128, 512, 3, 1), 256, 17),      # two taps per column tile, partial last column tile
    "pw two images":       ((2, 64, 64, 512, 256, 1, 1), 128, 32),       # a lateral over two images: long K, small output
    "3x3 two taps, tail":  ((1, 96, 99, 128, 512, 3, 1), 256, 17),
    "3x3 wide, no slabs":  ((1, 8, 17, 2048, 512, 3, 1), 256, 1),
}


@functools.lru_cache(maxsize=None)
def wgrad_case(name):
    """x [N, H, W, Cin] in steps of 1/8 within +-1, dy [N, Ho, Wo, Cout] in steps of 1/256 within +-1/16; dw packed [Cout, k k Cin] = the
    float64 sum over the pixels (oracle.np_oracle.conv2d_nhwc_backward); dw and 2 dw (the accumulate pass) exact in fp32."""
    from oracle import np_oracle as O
    (N, H, W, Cin, Cout, k, stride), _, _ = WGRAD_ROWS[name]
    assert stride == 1 and N * H * W < K_LIMIT
    rng = np.random.default_rng(_seed("wgrad", name))
    x = P.grid(rng, (N, H, W, Cin), 1 / 8, 1.0)
    dy = P.grid(rng, (N, H, W, Cout), 1 / 256, 1 / 16)
    pad = (k - 1) // 2
    _, dw, _ = O.conv2d_nhwc_backward(x, np.zeros((k, k, Cin, Cout)), dy, stride, (pad, pad, pad, pad))
    dw = P.assert_exact_f32(np.ascontiguousarray(np.transpose(dw, (3, 0, 1, 2)).reshape(Cout, k * k * Cin)), "dw")
    return _frozen({"x": x, "dy": dy, "k": k, "stride": stride, "pad": pad, "want": dw, "want_twice": P.assert_exact_f32(2 * dw, "2 dw")})


# ---------------------------------------------------------------------------------------------------------------------------------
# every launch of the tables, with what it reaches: (kernel, M, N, K, tile, slices, outs) -> _mechanisms

def legs():
    """[(what, kernel, mechanisms)] of every launch whose kernel the tables name (a convolution's tile = 0 leg only where the existing
    test asserts the library's choice)."""
    out = []
    for M, N, K, split_k, tile, slices in GEMM_PLAIN:
        out.append(("gemm %d x %d x %d split_k %d" % (M, N, K, split_k), GEMM_KERNEL[tile], _mechanisms(M, N, K, tile, slices, ("both",))))
    for M, N, K, residual, split_k, tile, slices in GEMM_EPILOGUE:
        for outs in GEMM_OUTS:
            out.append(("gemm epilogue %d x %d x %d %s %s" % (M, N, K, residual, outs), GEMM_KERNEL[tile], _mechanisms(M, N, K, tile, slices, (outs,))))
    for which, M, N, K, tile, slices in GATHER_LEGS:
        out.append(("gemm gather %s" % which, GEMM_KERNEL[tile], _mechanisms(M, N, K, tile, slices, ("both",))))
    s = STRIDED
    out.append(("gemm strided B", GEMM_KERNEL[s["tile"]], _mechanisms(s["T"] * s["Bn"], s["N"], s["K"], s["tile"], s["slices"], ("both",))))
    for name, (_, slabs) in CONV_ROWS.items():
        M, N, K, _, _ = conv_geometry(name)
        for tile in CONV_TILES:
            granted = CONV_OWN_TILE.get(name) if tile == 0 else conv_granted(name, tile)
            if granted is None:
                continue
            slices = 1 if tile == 0 else slabs.get(granted, 1)           # (the rows of CONV_OWN_TILE run unsplit)
            for outs in CONV_OUTS:
                out.append(("conv %s tile %d %s" % (name, tile, outs), CONV_KERNEL[granted], _mechanisms(M, N, K, granted, slices, (outs,))))
    for name, ((N, H, W, Cin, Cout, k, _), tile, slices) in WGRAD_ROWS.items():
        out.append(("wgrad %s" % name, WGRAD_KERNEL[tile], _mechanisms(Cout, k * k * Cin, N * H * W, tile, slices)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparison

def f32_bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def bf16_bits(a):
    """Values on the bf16 grid (float32 / float64) -> their 16-bit patterns."""
    u = f32_bits(a)
    assert not (u & 0xFFFF).any(), "not on the bf16 grid"
    return (u >> 16).astype(np.uint16)


def tie_shares(want):
    """(share of exact bf16 ties that round up -- the kept mantissa is odd --, share that round down to even) of an fp32-exact array."""
    u = f32_bits(want)
    tie = (u & 0xFFFF) == 0x8000
    odd = ((u >> 16) & 1) == 1
    return float((tie & odd).mean()), float((tie & ~odd).mean())


def _ordered(bits, width):
    """Sign-magnitude bit patterns as integers in value order: neighbouring values differ by one."""
    b = bits.astype(np.int64)
    sign = 1 << (width - 1)
    return np.where(b & sign, -(b & (sign - 1)), b)


def mismatch(got_bits, want, what, sentinel=None):
    """None when the output equals the exact result bit for bit, else the report.  got_bits: the output's bit patterns, uint32 for an
    fp32 output (want: the float64 exact result), uint16 for a bf16 one (want: its round-to-nearest-even, bf16_of).  The report says how
    many elements differ and where the first ones are, how many were never written (NaN, or still the sentinel), and what the
    differences look like: all of one bf16 ulp -- a rounding rule -- or larger -- a lost, doubled or misplaced product."""
    got_bits = np.asarray(got_bits)
    want = np.asarray(want, F64)
    assert got_bits.shape == want.shape, (what, got_bits.shape, want.shape)
    if got_bits.dtype == np.uint16:
        kind, want_bits, width = "bf16", bf16_bits(want), 16
        got = (got_bits.astype(np.uint32) << 16).view(F32).astype(F64)
    else:
        assert got_bits.dtype == np.uint32
        kind, want_bits, width = "fp32", f32_bits(P.assert_exact_f32(want, what)), 32
        got = got_bits.view(F32).astype(F64)
    if np.array_equal(got_bits, want_bits):
        return None
    bad = got_bits != want_bits
    where = np.argwhere(bad)
    unwritten = np.isnan(got)
    if sentinel is not None:                               # (a bf16 buffer holds the sentinel rounded to bf16)
        unwritten |= got_bits == (bf16_round(F32(sentinel)) if kind == "bf16" else f32_bits(F32(sentinel)))
    lines = ["%s (%s): %d of %d elements differ from the exact result; %d never written (NaN or sentinel)"
             % (what, kind, int(bad.sum()), bad.size, int((unwritten & bad).sum()))]
    for idx in where[:6]:
        at = tuple(int(i) for i in idx)
        lines.append("  at %s: got %.10g (0x%x) want %.10g (0x%x)" % (at, got[at], int(got_bits[at]), want[at], int(want_bits[at])))
    live = bad & ~unwritten
    if live.any():
        if kind == "bf16":
            step = np.abs(_ordered(got_bits[live], 16) - _ordered(want_bits[live], 16))
            if int(step.max()) == 1:
                lines.append("  every difference is ONE bf16 ulp: a rounding rule (truncation, ties away from zero, half up), not a product")
            else:
                lines.append("  differences of up to %d bf16 ulps (%d elements beyond one): a lost, doubled or misplaced product, not a rounding rule"
                             % (int(step.max()), int((step > 1).sum())))
        else:
            d = np.abs(got[live] - want[live])
            lines.append("  |got - want| from %.6g to %.6g, in units of the smallest product 2^-11: %.6g to %.6g -- a lost, doubled or "
                         "misplaced product, or an epilogue operand" % (d.min(), d.max(), d.min() * 2048, d.max() * 2048))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in fp32 NumPy, right or wrong on purpose (host only: proves that the comparison above sees each error)

def bf16_round(v, rule="even"):
    """fp32 values -> bf16 bit patterns by round-to-nearest-even, by truncation ("truncate"), with ties away from zero ("away") or with
    ties towards +infinity ("half up")."""
    u = f32_bits(v).astype(np.uint64)
    if rule == "even":
        u = u + 0x7FFF + ((u >> 16) & 1)
    elif rule == "away":
        u = u + 0x8000                                   # sign-magnitude: adding half an ulp to the magnitude rounds a tie outwards
    elif rule == "half up":
        u = u + np.where(u >> 31, 0x7FFF, 0x8000).astype(np.uint64)
    else:
        assert rule == "truncate"
    return (u >> 16).astype(np.uint16)


def emulate(A, B, scale=None, shift=None, residual=None, relu=False, drop=None, twice=None, rounding="even"):
    """relu((A B scale + shift) + residual) as the kernels compute it: fp32 accumulation of 64-deep K-tiles, the epilogue in fp32, the
    bf16 copy rounded from the fp32 value.  A [M, K], B [K, N] (a convolution: im2col and the packed kernel's transpose).
    drop = (m, n, k): the product A[m, k] B[k, n] is left out at output (m, n); twice = k0: the K-tile k0 .. k0 + 63 counts twice in the
    128 x 128 block at the origin; rounding: bf16_round's rule.  -> (fp32 bit patterns, bf16 bit patterns)."""
    A32, B32 = np.asarray(A, F32), np.asarray(B, F32)
    acc = np.zeros((A32.shape[0], B32.shape[1]), F32)
    for k0 in range(0, A32.shape[1], 64):
        acc = acc + (A32[:, k0:k0 + 64].astype(F64) @ B32[k0:k0 + 64].astype(F64)).astype(F32)
        if twice == k0:
            acc[:128, :128] += (A32[:128, k0:k0 + 64].astype(F64) @ B32[k0:k0 + 64, :128].astype(F64)).astype(F32)
    if drop is not None:
        m, n, k = drop
        acc[m, n] -= A32[m, k] * B32[k, n]
    v = acc
    if scale is not None:
        v = v * np.asarray(scale, F32)
    if shift is not None:
        v = v + np.asarray(shift, F32)
    if residual is not None:
        v = v + np.asarray(residual, F32).reshape(v.shape)
    if relu:
        v = np.maximum(v, F32(0))
    assert v.dtype == F32
    return f32_bits(v), bf16_round(v, rounding)


def smallest_product(A, B, want):
    """(m, n, k) of a product |A[m, k] B[k, n]| = 2^-11, the smallest a grid has, at the largest output that holds one (well above a
    relu's zero: the loss must show in the output)."""
    A, B = np.asarray(A, F64), np.asarray(B, F64)
    flat = np.asarray(want, F64).reshape(A.shape[0], B.shape[1])
    for at in np.argsort(-flat, axis=None)[:1000]:
        m, n = divmod(int(at), flat.shape[1])
        p = np.abs(A[m] * B[:, n])
        if (p == 2.0 ** -11).any():
            return m, n, int(np.argmax(p == 2.0 ** -11))
    raise AssertionError("no output holds a product of 2^-11")


def conv_as_gemm(c):
    """A P.conv_case as emulate()'s operands: (im2col [M, K], w^T [K, Cout], residual [M, Cout] or None)."""
    kh = c["kh"]
    A = im2col(c["x"], kh, kh, c["stride"], c["pad"], c["pad"], c["Ho"], c["Wo"])
    res = c["residual"]
    if c["res_mode"] == 2:
        res = res.repeat(2, axis=1).repeat(2, axis=2)
    return A, c["w"].T, None if res is None else res.reshape(A.shape[0], -1)
