"""The bf16 matrix kernels held to EXACT results on binary-grid operands (-m gpu): dc_gemm_bf16 (bgemm_kernel, bgemm256_kernel),
dc_conv2d_bf16 (bconv64_kernel, bconv_kernel, bconv256_kernel) and dc_conv2d_wgrad_bf16 (both tiles) on their main, vectorised paths --
full tiles, ragged edges, K tails, split-K slabs, gathers, every tile size.

tests/_bf16_exact_cases.py holds the cases and says why they are exact: every product, every partial sum in any order, every slab and
the whole epilogue fit fp32's 24 bits, so
  * the fp32 output equals the float64 result bit for bit, no element is left unwritten (the outputs start out filled with a
    sentinel) and nothing around the output changes (they sit in a sentinel ring);
  * every bf16 output -- the copy beside the fp32 one, or alone with C null, slabs or not -- equals the round-to-nearest-even of that
    value, element for element.  A few per cent of the elements of every case are exact ties on either side of round-to-even
    (tests/test_bf16_exact_cases.py), so truncation, ties-away and half-up each fail on thousands of elements.
tests/test_gpu_bf16.py holds the same kernels by tolerance on standard-normal operands, where one small product lost or doubled, or a
wrong rounding rule below the largest element's binade, passes.  A failure here reports how many elements differ, where, and whether
the differences are all one bf16 ulp (a rounding rule) or larger (a lost, doubled or misplaced product): X.mismatch.

Which tile and how many slabs run each case is asserted through the wrappers' info=, as the tables record it."""
import numpy as np
import pytest
import torch

import _bf16_exact_cases as X
import _placement_cases as P

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


_ON_DEVICE = {}


def dev(a, dtype=None, transposed=False):
    """The case's (cached, read-only) operand on the device, uploaded once: no kernel writes an input."""
    if a is None:
        return None
    key = (id(a), dtype, transposed)
    if key not in _ON_DEVICE:
        _ON_DEVICE[key] = (a, P.dev(a.T if transposed else a, dtype))            # (holds `a`: its id stays its own)
    return _ON_DEVICE[key][1]


def fresh(shape, dtype=None):
    """An output filled with the sentinel, inside a sentinel ring."""
    return P.carve(P.sentinel_like(shape, dtype), 0)


def host_bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).cpu().numpy().view(np.uint16 if t.dtype == BF else np.uint32)


def exact(what, out, want, out_b, want_bf16):
    """Both outputs (None: not asked for) equal the exact result bit for bit, and nothing outside them was written."""
    torch.cuda.synchronize()
    reports = []
    for t, w, kind in ((out, want, "float32"), (out_b, want_bf16, "bfloat16")):
        if t is None:
            continue
        assert P.untouched_outside(t), "%s: wrote outside its %s output" % (what, kind)
        reports.append(X.mismatch(host_bits(t), w, what, sentinel=P.SENTINEL[kind]))
    assert not any(reports), "\n".join(r for r in reports if r)


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_gemm_bf16

def run_gemm(ops, A, B, M, N, outs="both", C0=None, **kw):
    """-> (fp32 output or None, bf16 output or None, info); C0: the fp32 output starts as C0 and the call accumulates into it."""
    out = out_b = None
    if outs != "bf16":
        out = fresh((M, N)) if C0 is None else P.carve(P.dev(C0), 0)
    if outs != "f32":
        out_b = fresh((M, N), BF)
    info = {}
    ops.gemm_bf16(A, B, out=out, out_bf16=out_b, accumulate=C0 is not None, info=info, **kw)
    return out, out_b, info


@pytest.mark.parametrize("ta,tb", X.LAYOUTS)
@pytest.mark.parametrize("M,N,K,split_k,tile,slices", X.GEMM_PLAIN)
def test_gemm_bf16_layouts_exact(ops, M, N, K, split_k, tile, slices, ta, tb):
    """NN / NT / TN / TT on both tiles: ragged M and N, K tails, a single short K-tile pair, slabs by the library's rule and on request;
    the fp32 product and its bf16 copy."""
    c = X.gemm_plain(M, N, K)
    out, out_b, info = run_gemm(ops, dev(c["A"], BF, ta), dev(c["B"], BF, tb), M, N, a_trans=ta, b_trans=tb, split_k=split_k)
    assert info == {"tile": tile, "split_k": slices}, info
    exact("%d x %d x %d" % (M, N, K), out, c["want"], out_b, c["want_bf16"])


@pytest.mark.parametrize("outs", X.GEMM_OUTS)
@pytest.mark.parametrize("M,N,K,residual,split_k,tile,slices", X.GEMM_EPILOGUE)
def test_gemm_bf16_epilogue_exact(ops, M, N, K, residual, split_k, tile, slices, outs):
    """scale, shift, residual (whole or per row group), relu and accumulate, in the main kernel's store (one slice) and in the split-K
    reducer: fp32 alone, fp32 + bf16, and bf16 alone (C null, no accumulate) -- the output the bf16 model hands from layer to layer."""
    c = X.gemm_epilogue(M, N, K, residual)
    acc = outs != "bf16"
    out, out_b, info = run_gemm(ops, dev(c["A"], BF), dev(c["B"], BF), M, N, outs=outs, C0=c["C0"] if acc else None, scale=dev(c["scale"]),
                                shift=dev(c["shift"]), residual=dev(c["residual"]), res_rows=c["res_rows"], relu=True, split_k=split_k)
    assert info == {"tile": tile, "split_k": slices}, info
    exact("%d x %d x %d, %s" % (M, N, K, outs), out, c["want_acc"], out_b, c["want_acc_bf16" if acc else "want_bf16"])


@pytest.mark.parametrize("which,M,N,K,tile,slices", X.GATHER_LEGS)
def test_gemm_bf16_gather_exact(ops, which, M, N, K, tile, slices):
    """a_gather on the rows of A (the embedding lookup) and on the K rows of A^T (the embedding-side weight gradient), K padded from 300
    to 304 with zeros."""
    c = X.gather_case()
    ids = dev(c["ids"], torch.int32)
    if which == "rows":
        out, out_b, info = run_gemm(ops, dev(c["table"], BF), dev(c["W"], BF), M, N, gather=ids)
    else:
        out, out_b, info = run_gemm(ops, dev(c["table"], BF), dev(c["dz"], BF), M, N, a_trans=True, gather=ids)
    assert info == {"tile": tile, "split_k": slices}, info
    exact("gather " + which, out, c["want_" + which], out_b, c["want_%s_bf16" % which])


def test_gemm_bf16_strided_b_exact(ops):
    """B a view inside a larger matrix (row stride N + 8, 64 rows down), the per-RoI residual."""
    c, s = X.strided_case(), X.STRIDED
    out, out_b, info = run_gemm(ops, dev(c["X"], BF), dev(c["W"], BF)[64:, :s["N"]], s["T"] * s["Bn"], s["N"], residual=dev(c["r"]), res_rows=s["Bn"])
    assert info == {"tile": s["tile"], "split_k": s["slices"]}, info
    exact("strided B", out, c["want"], out_b, c["want_bf16"])


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_conv2d_bf16

@pytest.mark.parametrize("tile", X.CONV_TILES)
@pytest.mark.parametrize("outs", X.CONV_OUTS)
@pytest.mark.parametrize("name", list(X.CONV_ROWS))
def test_conv2d_bf16_exact(ops, name, outs, tile):
    """Every row of test_conv2d_bf16_matches_oracle on the library's own tile and on each tile it grants on request, fp32 + bf16 and
    bf16 alone: residual modes 0, 1 and 2, strides, borders, ragged pixel and channel counts, slabs."""
    c = X.conv_case(name)
    shape = c["want"].shape
    out = fresh(shape) if outs == "both" else None
    out_b = fresh(shape, BF)
    info = {}
    got = ops.conv2d_bf16(dev(c["x"], BF), dev(c["w"], BF), c["kh"], c["kh"], c["stride"], c["pad"], c["pad"], c["Ho"], c["Wo"], scale=dev(c["scale"]),
                          shift=dev(c["shift"]), residual=dev(c["residual"]), res_mode=c["res_mode"], relu=c["relu"], out=out, out_bf16=out_b,
                          want_f32=outs == "both", want_bf16=True, info=info, tile=tile, split_k=X.conv_split_k(name, tile))
    assert got[0] is out and got[1] is out_b
    if tile == 0:                                                  # the library's own choice
        assert info["tile"] == X.CONV_OWN_TILE.get(name, info["tile"]), info
    else:
        granted = X.conv_granted(name, tile)
        assert info == {"tile": granted, "split_k": X.CONV_ROWS[name][1].get(granted, 1)}, info
    exact("conv %s, tile %d, %s" % (name, tile, outs), out, c["want"], out_b, c["want_bf16"])


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_conv2d_wgrad_bf16

@pytest.mark.parametrize("name", list(X.WGRAD_ROWS))
def test_conv2d_wgrad_bf16_exact(ops, name):
    """The weight gradient over the pixels on both tiles, slabs by the library's rule: dw, then once more accumulating into it: 2 dw."""
    c = X.wgrad_case(name)
    _, tile, slices = X.WGRAD_ROWS[name]
    x, dy = dev(c["x"], BF), dev(c["dy"], BF)
    assert ops.wgrad_bf16_supported(x.shape, dy.shape)
    out = fresh(c["want"].shape)
    info = {}
    ops.conv2d_wgrad_bf16(x, dy, c["k"], c["k"], c["stride"], c["pad"], c["pad"], out=out, info=info)
    assert info == {"tile": tile, "split_k": slices}, info
    exact("wgrad " + name, out, c["want"], None, None)
    ops.conv2d_wgrad_bf16(x, dy, c["k"], c["k"], c["stride"], c["pad"], c["pad"], out=out, accumulate=True)
    exact("wgrad %s, accumulated" % name, out, c["want_twice"], None, None)
