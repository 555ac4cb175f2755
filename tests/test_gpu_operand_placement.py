"""Operands that are not "16-byte friendly" (-m gpu): the scalar, ragged and smaller-tile paths compute the right thing, silent route
changes are the ones the queries report, and every DC_EALIGN refusal refuses before anything is written.

The vector side of the ~70 host-side placement predicates (aligned16(...), & 3, & 7, Epilogue::vec4, gemm_is_fast, the Winograd and
streaming-pointwise applicability tests, bconv_tile, colsum_plan, ...) is what every other test file runs; this file runs the other
side.  Operands come from tests/_placement_cases.py on binary grids, so every expected value is the exact float64 result and the
comparison is equality (np.testing.assert_array_equal); where one placement sends the same problem down the vector path, both
outputs equal the exact result and therefore each other.  Every output is carved out of a sentinel-filled buffer: the ring around a
misplaced output and the padding columns of a strided one must be unchanged afterwards.  softmax_ce / vocab_ce cannot be made exact
(exp): they keep the tolerances of test_softmax_ce, test_masked_keras_sparse_ce and test_vocab_ce_bf16_* in the other files.

Routes asserted (entry point, placement -> kernel or tile reported):
  ops.conv2d 3x3 32->32 with w_wino / w_wino_b3   y, u, scale or shift + 4 bytes      wino*  ->  igemm_pc_kernel<.., Im2colKCT<false>, ..>
  ops.conv2d 1x1 64->64, 128->512 (+ residual)    y, residual, scale or shift + 4     pwconv_stream_kernel<Cin, r>  ->  igemm*<DenseKCT<true>, DenseKCT<true>>
  ops.conv2d math 1, 2, 3                         Cout % 4 != 0                       igemm_bs_kernel<bm, bn> (unchanged: the epilogue alone differs)
  ops.gemm_bf16                                   every scalar-epilogue placement     tile 128; scale + 4 at 512 x 512 x 2112 / 33 slices: 256 -> 128
  ops.conv2d_bf16                                 Cout 66 or residual + 4, tile 64 / 256 forced    tile 128 (tile 64 honoured when aligned)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _placement_cases as P
from image_captioning_amd._lib import DcapError

from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    from image_captioning_amd import _lib
    return _lib.load()


def exact(got, want, what):
    np.testing.assert_array_equal(P.host(got), np.asarray(want, np.float64), err_msg=what)


def close(got, want, tol):
    got, want = P.host(got), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
    assert err < tol, "max err %.3e (scaled) exceeds %.1e" % (err, tol)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def placed(a, how, name, ld_pad=6, dtype=None):
    """The operand `name` on the device: None stays None; "<name>+4" puts it 4 bytes past a 16-byte boundary, "ld<name>" gives a 2-D one a
    row stride of cols + ld_pad (not a multiple of 4 for the widths used here); any other placement leaves it aligned and contiguous."""
    if a is None:
        return None
    t = P.dev(a, dtype)
    if how == name + "+4":
        return P.misplaced(t)
    if how == "ld" + name:
        assert (t.shape[1] + ld_pad) % 4 != 0
        return P.restride(t, t.shape[1] + ld_pad)
    return P.carve(t, 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# ops.gemm: the scalar epilogue (store_tile's DC_TAIL / Epilogue::finish), the scalar slab store and reducer (Epilogue::apply), the
# guarded loaders

LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]


def run_gemm(ops, c, a_trans=False, b_trans=False, how=None, split_k=0, lda=None, ldb=None, gather=None, table=None):
    """c (P.gemm_case) through ops.gemm with the operands stored for the layout; `how` names the one misplaced operand."""
    A = table if table is not None else (c["A"].T if a_trans else c["A"])
    B = c["B"].T if b_trans else c["B"]
    # (lda and ldb are multiples of 4 by the validator's rule: a K-major operand with a ragged row length is a view of padded rows)
    lda = lda or (A.shape[1] + 3) // 4 * 4
    ldb = ldb or (B.shape[1] + 3) // 4 * 4
    A = P.dev(A) if lda == A.shape[1] else P.restride(P.dev(A), lda)
    B = P.dev(B) if ldb == B.shape[1] else P.restride(P.dev(B), ldb)
    out = placed(c["C0"], how, "C") if c["C0"] is not None else P.carve(P.sentinel_like((c["M"], c["N"])), 4 if how == "C+4" else 0,
                                                                           c["N"] + 6 if how == "ldC" else None)
    ops.gemm(A, B, out=out, a_trans=a_trans, b_trans=b_trans, gather=gather, scale=placed(c["scale"], how, "scale"),
             shift=placed(c["shift"], how, "shift"), residual=placed(c["residual"], how, "residual"), res_rows=c["res_rows"], relu=c["relu"],
             accumulate=c["C0"] is not None, split_k=split_k)
    torch.cuda.synchronize()
    assert P.untouched_outside(out), "gemm wrote outside its output (%s)" % how
    return out


@pytest.mark.parametrize("residual", ["full", 35])
@pytest.mark.parametrize("a_trans,b_trans", LAYOUTS)
@pytest.mark.parametrize("N", [65, 66, 67])
def test_gemm_width_not_a_multiple_of_4(ops, N, a_trans, b_trans, residual):
    """N % 4 != 0: vec4 = 0, every tile stores through DC_TAIL -- scale, shift, residual mode 1 / 3, relu and accumulate element by
    element, the last column quad of each row partly masked.  M = 70 (not a multiple of 4: A^T and B take the guarded loaders)."""
    c = P.gemm_case(N, 70, N, 64, residual=residual)
    exact(run_gemm(ops, c, a_trans, b_trans), c["want"], "gemm N=%d" % N)


GEMM_PLACEMENTS = ["C+4", "ldC", "residual+4", "ldresidual", "scale+4", "shift+4"]


@pytest.mark.parametrize("residual", ["full", 65])
@pytest.mark.parametrize("how", GEMM_PLACEMENTS)
def test_gemm_one_operand_misplaced(ops, how, residual):
    """N % 4 == 0 and one epilogue operand off its 16-byte rule: the scalar epilogue, bit for bit the vector path's result."""
    c = P.gemm_case(7, 130, 132, 64, residual=residual)
    got = run_gemm(ops, c, how=how)
    exact(got, c["want"], how)
    assert torch.equal(got, run_gemm(ops, c)), "the scalar and the vector epilogue differ (%s)" % how


@pytest.mark.parametrize("M,N", [(4098, 2052), (4098, 1028)])
def test_gemm_misplaced_output_on_the_128_row_tiles(ops, M, N):
    """choose_tile takes the 128 x 128 (N = 2052: 33 x 17 tiles) and 128 x 64 (N = 1028) kernels only where they fill the chip twice:
    their store_tile instantiations on the scalar path, ragged in M and N."""
    c = P.gemm_case(M + N, M, N, 32, residual=M // 2)
    exact(run_gemm(ops, c, how="C+4"), c["want"], "C+4 at %d x %d" % (M, N))


class _MisplacedWorkspace(object):
    """Stands in for ops.WORKSPACE: every scratch buffer 4 bytes past a 16-byte boundary, inside a sentinel ring."""

    def __init__(self):
        self.handed = []

    def get(self, nbytes, device):
        if nbytes == 0:
            return None, 0
        ws = P.carve(P.sentinel_like((int(nbytes),), torch.uint8), 4)
        self.handed.append(ws)
        return ws, int(nbytes)


@pytest.mark.parametrize("workspace", ["aligned", "misplaced"])
@pytest.mark.parametrize("split_k", [0, 2, 3])
@pytest.mark.parametrize("M,N,how", [(70, 67, None), (130, 132, "C+4")])
def test_gemm_split_k(ops, monkeypatch, M, N, how, split_k, workspace):
    """K = 128 in slabs.  N = 67: the scalar slab store of store_tile and the scalar half of splitk_reduce_kernel (any 4-byte-aligned
    workspace serves); N = 132 with a misplaced C: 16-byte slab stores and loads, Epilogue::apply / put per element -- and a workspace
    off the 16-byte boundary is refused there (DC_REQUIRE_SLAB_ALIGNED), not stored through."""
    c = P.gemm_case(M + split_k, M, N, 128, residual="full")
    if workspace == "misplaced":
        stub = _MisplacedWorkspace()
        monkeypatch.setattr(ops, "WORKSPACE", stub)
        if N % 4 == 0 and split_k > 1:
            with pytest.raises(DcapError, match=r"code -2.*igemm split-K: the workspace must be 16-byte aligned"):
                run_gemm(ops, c, how=how, split_k=split_k)
            return
    exact(run_gemm(ops, c, how=how, split_k=split_k), c["want"], "split_k=%d" % split_k)
    if workspace == "misplaced":
        assert len(stub.handed) == (1 if split_k > 1 else 0)
        assert all(P.untouched_outside(ws) for ws in stub.handed)


def test_gemm_k_tail_with_ragged_width(ops):
    """K = 136: gemm_split_tail runs K = 128 on the fast loaders and the last 8 columns through the range-checked kernel, accumulating
    into C -- both launches on the scalar epilogue (N = 67).  Additive epilogue only (no scale, no relu), as that path requires."""
    c = P.gemm_case(136, 70, 67, 136, scale=False, relu=False, residual="full")
    exact(run_gemm(ops, c, b_trans=True), c["want"], "K tail")


@pytest.mark.parametrize("M", [1, 2, 3, 37])
def test_gemm_guarded_loader_a_transposed(ops, M):
    """A^T with M % 4 != 0 or M < 4 (lda = 40): gemm_is_fast is false, DenseMC reads the last column quad of each K row guarded."""
    c = P.gemm_case(M, M, 8, 64, residual="full")
    exact(run_gemm(ops, c, a_trans=True, lda=40), c["want"], "A^T M=%d" % M)


@pytest.mark.parametrize("N", [1, 2, 3, 37])
def test_gemm_guarded_loader_b_k_major(ops, N):
    c = P.gemm_case(N, 9, N, 64, residual="full")
    exact(run_gemm(ops, c, ldb=40), c["want"], "B [K,N] N=%d" % N)


def test_gemm_gather_on_the_ragged_path(ops):
    """The embedding gather through the guarded loader (B [K,N] with N = 37): row m of A is table[ids[m]]."""
    c = P.gemm_case(5, 10, 37, 64, residual="full")
    rng = np.random.default_rng(5)
    ids = rng.permutation(20)[:10]
    table = P.grid(rng, (20, 64), 1 / 8, 1.0)
    table[ids] = c["A"]
    exact(run_gemm(ops, c, gather=P.dev(ids, torch.int32), table=table), c["want"], "gather")


# ---------------------------------------------------------------------------------------------------------------------------------
# ops.gemm_bf16

def run_gemm_bf16(ops, c, how=None, outs=("f32", "bf16"), split_k=0):
    """A [M,K] x B^T (stored [N,K]) in bf16; -> (fp32 output or None, bf16 output or None, info)."""
    M, N = c["M"], c["N"]
    out = out_b = None
    if "f32" in outs:
        out = placed(c["C0"], how, "C") if c["C0"] is not None else P.carve(P.sentinel_like((M, N)), 0)
    if "bf16" in outs:
        out_b = P.carve(P.sentinel_like((M, N), BF), 4 if how == "Cb+4" else 0, N + 6 if how == "ldCb" else None)
    info = {}
    ops.gemm_bf16(P.dev(c["A"], BF), P.dev(c["B"].T, BF), out=out, out_bf16=out_b, b_trans=True, scale=placed(c["scale"], how, "scale"),
                  shift=placed(c["shift"], how, "shift"), residual=placed(c["residual"], how, "residual"), res_rows=c["res_rows"], relu=c["relu"],
                  accumulate=c["C0"] is not None, split_k=split_k, info=info)
    torch.cuda.synchronize()
    for t in (out, out_b):
        assert t is None or P.untouched_outside(t), "gemm_bf16 wrote outside its output (%s)" % how
    return out, out_b, info


def check_gemm_bf16(c, out, out_b, what):
    if out is not None:
        exact(out, c["want"], what + " (fp32)")
    if out_b is not None:
        exact(out_b, P.bf16_of(c["want"]), what + " (bf16 copy)")


@pytest.mark.parametrize("N", [66, 67])
def test_gemm_bf16_width_not_a_multiple_of_8(ops, N):
    """b_trans with N % 8 != 0 (N % 4 != 0 too): the validator admits it, the epilogue is scalar, fp32 result and bf16 copy."""
    c = P.gemm_case(N, 72, N, 64, residual="full")
    out, out_b, info = run_gemm_bf16(ops, c)
    assert info["tile"] == 128
    check_gemm_bf16(c, out, out_b, "N=%d" % N)


@pytest.mark.parametrize("how", ["Cb+4", "ldCb", "C+4", "ldC", "residual+4", "ldresidual", "scale+4", "shift+4"])
def test_gemm_bf16_one_operand_misplaced(ops, how):
    """Cb on a 4-byte boundary (the & 7 rule), ldcb % 4 != 0, and each fp32 epilogue operand off its rule: scalar epilogue on the
    128 tile, both outputs bit for bit the vector path's."""
    c = P.gemm_case(11, 130, 132, 64, residual="full")
    out, out_b, info = run_gemm_bf16(ops, c, how)
    assert info["tile"] == 128
    check_gemm_bf16(c, out, out_b, how)
    ref, ref_b, _ = run_gemm_bf16(ops, c)
    assert torch.equal(out, ref) and torch.equal(out_b, ref_b), "the scalar and the vector epilogue differ (%s)" % how


@pytest.mark.parametrize("how", [None, "Cb+4", "ldCb"])
def test_gemm_bf16_copy_alone(ops, how):
    """out_bf16 with C null (no accumulate): Epilogue::put writes the bf16 copy only."""
    c = P.gemm_case(13, 130, 132, 64, residual=65, accumulate=False)
    out, out_b, info = run_gemm_bf16(ops, c, how, outs=("bf16",))
    assert out is None and info["tile"] == 128
    check_gemm_bf16(c, None, out_b, "bf16 alone, %s" % how)


def test_gemm_bf16_leaves_the_256_tile_for_a_misplaced_operand(ops):
    """512 x 512 x 2112 in 33 slices: the cost model prefers the 256 tile (16 x 33 blocks of the 128 tile no longer fit the chip at once);
    its epilogue is 16-byte accesses only, so a misplaced scale sends the problem to the 128 tile -- same exact result."""
    c = P.gemm_case(17, 512, 512, 2112, residual=256)
    out, out_b, info = run_gemm_bf16(ops, c, split_k=33)
    assert info["tile"] == 256 and info["split_k"] == 33
    check_gemm_bf16(c, out, out_b, "256 tile")
    got, got_b, info = run_gemm_bf16(ops, c, "scale+4", split_k=33)
    assert info["tile"] == 128 and info["split_k"] == 33
    check_gemm_bf16(c, got, got_b, "128 tile, scalar reducer operands")
    assert torch.equal(got, out) and torch.equal(got_b, out_b)


# ---------------------------------------------------------------------------------------------------------------------------------
# ops.conv2d: the four math modes on the scalar epilogue, placements, Winograd and streaming-pointwise route changes

MATHS = [0, 1, 2, 3]                          # DC_MATH_F32, BF16X3, BF16X2, BF16
KERNELS = {"1x1": (1, 1), "3x3": (3, 1), "1x1s2": (1, 2)}


def conv_args(c, how=None):
    x, w = P.dev(c["x"]), P.dev(c["w"])
    out = P.carve(P.sentinel_like(c["want"].shape), 4 if how == "y+4" else 0)
    kw = dict(scale=placed(c["scale"], how, "scale"), shift=placed(c["shift"], how, "shift"), residual=placed(c["residual"], how, "residual"),
              res_mode=c["res_mode"], relu=c["relu"], out=out)
    return (x, w, c["kh"], c["kh"], c["stride"], c["pad"], c["pad"], c["Ho"], c["Wo"]), kw


def run_conv(ops, c, math=0, how=None, split_k=0, **more):
    args, kw = conv_args(c, how)
    kw.update(more, math=math, split_k=split_k)
    name = ops.conv2d_kernel_name(*args, **kw)
    out = ops.conv2d(*args, **kw)
    torch.cuda.synchronize()
    assert P.untouched_outside(out), "conv2d wrote outside its output (%s)" % how
    return out, name


@pytest.mark.parametrize("Cout", [66, 35])
@pytest.mark.parametrize("shape", [(1, 8, 8, 32), (2, 9, 7, 64)])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("math", MATHS)
def test_conv2d_cout_not_a_multiple_of_4(ops, math, kernel, shape, Cout):
    """Cout % 4 != 0: DC_TAIL per element in every math mode, residual modes 0, 1 and (even output) 2, relu, with and without split-K
    (scalar slab store + Epilogue::apply, mode 2's parent-pixel index included)."""
    kh, stride = KERNELS[kernel]
    N, H, W, Cin = shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    for res_mode in (0, 1, 2):
        if res_mode == 2 and (Ho % 2 or Wo % 2):
            continue
        c = P.conv_case(100 * math + 10 * kh + res_mode, N, H, W, Cin, Cout, kh, stride, res_mode=res_mode)
        for split_k in (0, 2):
            out, name = run_conv(ops, c, math, split_k=split_k)
            assert name.startswith("igemm_bs_kernel<" if math else ("igemm_pc_kernel<", "igemm_kernel<")), name
            exact(out, c["want"], "%s math %d res_mode %d split_k %d" % (kernel, math, res_mode, split_k))


@pytest.mark.parametrize("how", ["y+4", "residual+4", "scale+4", "shift+4"])
@pytest.mark.parametrize("kernel", ["1x1", "3x3"])
@pytest.mark.parametrize("math", MATHS)
def test_conv2d_one_operand_misplaced(ops, math, kernel, how):
    """Cout = 64 with y, residual, scale or shift 4 bytes off: vec4 = 0 by placement alone; bit for bit the aligned call's output."""
    kh, stride = KERNELS[kernel]
    c = P.conv_case(7 + math, 1, 8, 8, 32, 64, kh, stride, res_mode=1)
    got, _ = run_conv(ops, c, math, how)
    exact(got, c["want"], "%s math %d %s" % (kernel, math, how))
    ref, _ = run_conv(ops, c, math)
    assert torch.equal(got, ref)
    got2, _ = run_conv(ops, c, math, how, split_k=2)
    exact(got2, c["want"], "%s math %d %s split_k 2" % (kernel, math, how))


@pytest.mark.parametrize("how", [None, "y+4", "scale+4", "shift+4", "u+4"])
@pytest.mark.parametrize("form", ["w_wino", "w_wino_b3"])
def test_conv2d_winograd_falls_to_the_direct_kernel(ops, form, how):
    """A 32 -> 32 3x3 / stride 1 / 'same' layer with pre-transformed weights runs in the Winograd form -- unless y, u, scale or shift
    is misplaced: then the direct kernel, which dc_conv2d_kernel_name must report.  Exact either way (the transforms' halves and
    quarters stay on the grid)."""
    c = P.conv_case(3, 1, 8, 8, 32, 32, 3, 1, res_mode=0)
    w = P.dev(c["w"])
    u = ops.winograd_pack(w, 32, 32) if form == "w_wino" else ops.winograd_pack_b3(w, 32, 32)
    if how == "u+4":
        u = P.misplaced(u)
    out, name = run_conv(ops, c, 0, how, **{form: u})
    if how is None:
        assert name.startswith("wino") and name.endswith("b_kernel") == (form == "w_wino_b3"), name
    else:
        assert not name.startswith("wino") and "Im2colKCT<false>" in name, name
    exact(out, c["want"], "%s %s via %s" % (form, how, name))


STREAM_LAYERS = [(64, 64, 0, how) for how in (None, "y+4", "scale+4", "shift+4")] + [
    (128, 512, 1, how) for how in (None, "y+4", "residual+4", "scale+4", "shift+4")]


@pytest.mark.parametrize("Cin,Cout,res_mode,how", STREAM_LAYERS)
def test_conv2d_streaming_pointwise_falls_to_the_generic_kernel(ops, Cin, Cout, res_mode, how):
    """Short-K 1x1 layers run on pwconv_stream_kernel while every epilogue operand takes 16-byte accesses; one misplaced operand
    (!ep.vec4) sends the layer to the generic pointwise kernel, and the name query says so."""
    c = P.conv_case(Cin + Cout, 2, 9, 7, Cin, Cout, 1, 1, res_mode=res_mode)
    out, name = run_conv(ops, c, 0, how)
    if how is None:
        assert name == "pwconv_stream_kernel<%d, %d>" % (Cin, res_mode), name
    else:
        assert name.startswith("igemm") and "dcap::DenseKCT<true>, dcap::DenseKCT<true>" in name, name
    exact(out, c["want"], "%d -> %d %s via %s" % (Cin, Cout, how, name))


# ---------------------------------------------------------------------------------------------------------------------------------
# ops.conv2d_bf16: bconv_tile falls from a forced 64 or 256 tile to 128 when the epilogue cannot be 16-byte accesses

@pytest.mark.parametrize("outs", [("f32",), ("bf16",), ("f32", "bf16")])
@pytest.mark.parametrize("tile", [0, 64, 256])
@pytest.mark.parametrize("Cout,how", [(66, None), (66, "residual+4"), (64, "residual+4"), (64, None)])
def test_conv2d_bf16_scalar_epilogue_on_the_128_tile(ops, Cout, how, tile, outs):
    c = P.conv_case(Cout + tile, 2, 9, 7, 64, Cout, 3, 1, res_mode=1)
    out = P.carve(P.sentinel_like(c["want"].shape), 0) if "f32" in outs else None
    out_b = P.carve(P.sentinel_like(c["want"].shape, BF), 0) if "bf16" in outs else None
    info = {}
    ops.conv2d_bf16(P.dev(c["x"], BF), P.dev(c["w"], BF), 3, 3, 1, 1, 1, c["Ho"], c["Wo"], scale=placed(c["scale"], how, "scale"),
                    shift=placed(c["shift"], how, "shift"), residual=placed(c["residual"], how, "residual"), res_mode=1, relu=True, out=out,
                    out_bf16=out_b, want_f32="f32" in outs, want_bf16="bf16" in outs, info=info, tile=tile)
    torch.cuda.synchronize()
    if Cout % 4 or how is not None:
        assert info["tile"] == 128, "a tile with a 16-byte-only epilogue was chosen: %r" % (info,)
    elif tile == 64:
        assert info["tile"] == 64                     # (a forced tile is honoured where the epilogue allows it)
    if out is not None:
        assert P.untouched_outside(out)
        exact(out, c["want"], "fp32 output")
    if out_b is not None:
        assert P.untouched_outside(out_b)
        exact(out_b, P.bf16_of(c["want"]), "bf16 output")


# ---------------------------------------------------------------------------------------------------------------------------------
# ops.colsum: colsum_kernel<1> for a misplaced x, and the no-workspace plan (chunks = 1) of the C entry point

def _colsum_case(M, N, seed):
    rng = np.random.default_rng(seed)
    x = P.grid(rng, (M, N), 1 / 8, 1.0)
    base = P.grid(rng, (N,), 1 / 8, 4.0)
    return x, base, P.assert_exact_f32(x.sum(axis=0), "column sums"), P.assert_exact_f32(x.sum(axis=0) + base, "column sums + base")


@pytest.mark.parametrize("M,N,ld", [(37, 20, 24), (4097, 512, 512)])
def test_colsum_misplaced_input(ops, M, N, ld):
    """x 4 bytes off with ld % 4 == 0 and N % 4 == 0: only the base sends colsum_plan to colsum_kernel<1>.  Sums of 1/8-grid values:
    exact, whatever the chunking (4097 x 512 runs over a hundred row chunks through the workspace)."""
    x, base, want, want_acc = _colsum_case(M, N, M)
    xd = P.carve(P.dev(x), 4, ld)
    out = P.carve(P.sentinel_like((N,)), 0)
    ops.colsum(xd, out=out)
    exact(out, want, "colsum")
    assert torch.equal(out, ops.colsum(P.carve(P.dev(x), 0, ld)))
    acc = P.carve(P.dev(base), 4)
    ops.colsum(xd, out=acc, accumulate=True)
    exact(acc, want_acc, "colsum accumulate")
    torch.cuda.synchronize()
    assert P.untouched_outside(out) and P.untouched_outside(acc)


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("accumulate", [False, True])
def test_colsum_without_workspace(lib, accumulate, offset):
    """workspace = NULL where the plan wants over a hundred chunks (4097 x 512): one block column walks all rows (chunks = 1), straight into out
    -- ops.WORKSPACE never hands out less than 1 MiB, so only the C entry point reaches this."""
    M, N = 4097, 512
    assert lib.dc_colsum_workspace_bytes(M, N, N) >= 64 * N * 4                  # the plan wants many chunks
    x, base, want, want_acc = _colsum_case(M, N, 9)
    xd = P.carve(P.dev(x), offset)
    out = P.carve(P.dev(base) if accumulate else P.sentinel_like((N,)), 0)
    rc = lib.dc_colsum_f32(C.c_void_p(xd.data_ptr()), M, N, N, C.c_void_p(out.data_ptr()), int(accumulate), None, 0, stream())
    assert rc == 0, lib.dc_last_error()
    exact(out, want_acc if accumulate else want, "colsum, no workspace")
    assert P.untouched_outside(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# ops.softmax_ce with ld % 4 != 0 (contiguous V = 1003 and V = 3): the scalar loops only, on any 4-byte boundary

@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("V", [1003, 3])
def test_softmax_ce_unpadded_rows(ops, V, sparse, offset):
    """Tolerances: test_softmax_ce's (1e-6 probabilities and gradients, 1e-5 loss) and test_masked_keras_sparse_ce's (2e-5)."""
    M = 6
    rng = np.random.default_rng(V + sparse)
    z = 3.0 * rng.standard_normal((M, V))
    t = rng.integers(0, V, M)
    z[0, t[0]] = -60.0                                    # target probability below 1e-7: clipped row
    z[1, :] = -50.0
    z[1, t[1]] = 50.0                                     # target probability above 1 - 1e-7: clipped row
    w = rng.random(M)
    w[2] = 0.0
    z = z.astype(np.float32).astype(np.float64)
    p = O.softmax(z)
    zd = P.carve(P.dev(z), offset)
    assert zd.stride(0) == V and V % 4 != 0
    probs, dl, loss = P.carve(P.sentinel_like((M, V)), offset), P.carve(P.sentinel_like((M, V)), offset), P.carve(P.sentinel_like((M,)), 0)
    if sparse:
        want_loss, want_d = O.sparse_cce_keras_with_grad(t, p, w)
        ops.softmax_ce(zd, P.dev(t, torch.int32), probs, loss, dl, grad_scale=1.0, row_weights=P.dev(w), keras_sparse=True)
        close(loss, want_loss, 2e-5)
        close(dl, want_d, 2e-5)
        close(probs, p, 2e-5)
    else:
        ops.softmax_ce(zd, P.dev(t, torch.int32), probs, loss, dl, grad_scale=1.0 / M, row_weights=P.dev(w))
        close(probs, p, 1e-6)
        close(loss, w * O.categorical_crossentropy(t, p), 1e-5)
        close(dl, O.softmax_ce_grad_logits(t, p, w / M), 1e-6)
        assert float(dl[0].abs().max()) == 0.0 and float(dl[1].abs().max()) == 0.0
    assert float(dl[2].abs().max()) == 0.0
    torch.cuda.synchronize()
    assert all(P.untouched_outside(o) for o in (probs, dl, loss))


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_vocab_ce: the materialised-logits route needs a 16-byte aligned bf16 gradient buffer; on an 8-byte boundary (all the validator
# asks) the call silently takes the recomputing passes

def test_vocab_ce_route_follows_the_gradient_buffer_placement(ops):
    """Two calls that differ only in where dlogits sits (3000 x 4104 x 256 bf16: the 256 tile, test_vocab_ce_bf16_materialised_logits'
    first case).  16-byte aligned: logits rounded to bf16 and parked in the buffer (that test's tolerances, reference = the oracle on
    the rounded logits).  8 bytes further: the recomputing route on fp32 logits (test_vocab_ce_bf16_on_the_256_tile's tolerance) --
    per element the arithmetic of an aligned call with materialize_bf16 off, so equal to it bit for bit."""
    M, V, K = 3000, 4104, 256
    rng = np.random.default_rng(V + K + M)
    X = rng.standard_normal((M, K))
    W = rng.standard_normal((K, V)) * (2.0 / np.sqrt(K)) * 0.25
    b = rng.standard_normal(V) * 0.5
    t = rng.integers(0, V, M)
    X[1] = 0
    Xd, Wd, bd, td = ops.to_bf16(P.dev(X)), ops.to_bf16(P.dev(W)), P.dev(b), P.dev(t, torch.int32)
    z = O.to_bf16(X) @ O.to_bf16(W) + b
    Vp = V + 8
    kw = dict(grad_scale=1.0 / M)

    def call(offset_bytes, materialize):
        loss = torch.empty(M, device="cuda")
        dl = P.carve(torch.full((M, Vp), 7.0, dtype=BF, device="cuda"), offset_bytes)
        db = torch.empty(V, device="cuda")
        ops.vocab_ce(Xd, Wd, bd, td, loss_rows=loss, dlogits=dl, dbias=db, materialize_bf16=materialize, **kw)
        torch.cuda.synchronize()
        assert P.untouched_outside(dl)
        return loss, dl, db

    # the recomputing route, reached by placement alone
    p = O.softmax(z)
    want_loss, want_d = O.categorical_crossentropy(t, p), O.softmax_ce_grad_logits(t, p, np.full(M, 1.0 / M)) * M
    loss8, dl8, db8 = call(8, True)
    got = P.host(dl8) * M
    close(loss8, want_loss, 3e-5)
    assert np.abs(got[:, :V] - want_d).max() <= 2.0 ** -8 * np.abs(want_d).max() + 1e-6 and not got[:, V:].any()
    loss0, dl0, db0 = call(0, False)
    assert torch.equal(loss8, loss0) and torch.equal(dl8, dl0) and torch.equal(db8, db0)
    # the materialised route at the aligned placement
    zmax = np.abs(z).max(axis=1)
    pr = O.softmax(O.to_bf16(z))
    want_loss, want_d = O.categorical_crossentropy(t, pr), O.softmax_ce_grad_logits(t, pr, np.full(M, 1.0 / M)) * M
    loss_m, dl_m, _ = call(0, True)
    got = P.host(dl_m) * M
    lerr = np.abs(P.host(loss_m) - want_loss)
    assert np.all(lerr <= 2.0 ** -7 * np.maximum(1.0, zmax) + 3e-5), float(lerr.max())
    assert not got[:, V:].any()
    assert np.abs(got[:, :V] - want_d).max() <= (2.0 ** -7 * max(1.0, float(zmax.max())) / 2 + 2.0 ** -8) * np.abs(want_d).max() + 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# every alignment refusal refuses

@pytest.mark.parametrize("literal,case", [pytest.param(lit, fn, id=case_id) for lit, case_id, fn in P.REFUSALS])
def test_alignment_refusal(ops, lib, literal, case):
    """One valid small call with exactly one thing wrong: DC_EALIGN (-2) with the site's message, and no output byte written."""
    h = P.Harness(ops, lib)
    try:
        with pytest.raises(DcapError) as e:
            case(h)
    finally:
        h.restore()
    assert "(code %d)" % P.DC_EALIGN in str(e.value), str(e.value)
    message = lib.dc_last_error().decode()
    assert P.literal_regex(literal).fullmatch(message), "dc_last_error() = %r, expected the site %r" % (message, literal)
    assert h.who is None or message.startswith(h.who + ":"), "refused by %r, expected %r" % (message, h.who)
    assert h.watched, "the case lists no output"
    assert h.unchanged(), "a refused call wrote to one of its outputs"
