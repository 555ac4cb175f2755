"""Thin torch-tensor wrappers over the C-ABI (include/dcap.h).  torch is plumbing here: device memory,
the current HIP stream and (elsewhere) torch.distributed; every arithmetic op is a dc_* kernel.
All wrappers enqueue on torch's current stream and never synchronise.
"""
import contextlib
import ctypes as C
import os

import numpy as np

import torch

from . import _lib
from ._lib import (RpnTargetsDesc, PwChainDesc, ConvBf16Desc, AmsgradDesc, DetectionTargetsDesc, BnReluDesc, ConvDesc, ConvWgradBf16Desc, GemmBf16Desc, VocabCeDesc, ProposalDesc, RpnLossDesc, GemmDesc, LstmBwdDesc, LstmFwdDesc, RoialignDesc, RoiGroupsDesc,
                   SoftmaxCeDesc, TagFocalDesc, VocabTop1Desc, VocabTopkDesc, VocabTop1Bf16Desc, VocabTopkBf16Desc, VocabSampleDesc, VocabSampleBf16Desc, BeamSelectDesc, BeamStepDesc, LstmStepDesc, RefineDesc, RefineDetDesc, ResizePadDesc, MaskHeadTailDesc, MaskPasteDesc, MaskRleDesc, RleIouDesc, DetectionApDesc, check)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t, dtype=torch.float32, name="tensor"):
    if not t.is_cuda:
        raise _lib.DcapError("%s must live on the GPU (no CPU path exists)" % name)
    if t.dtype != dtype:
        raise _lib.DcapError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.dim() > 0 and t.stride(-1) != 1:
        raise _lib.DcapError("%s must be contiguous along its last dimension" % name)
    return t


class no_gc_during_capture(object):
    """Context manager for hipGraph captures: collect garbage BEFORE the capture and keep the cyclic collector off while it lasts.  A
    collection that happens to run inside a capture finalises whatever cyclic garbage is pending -- a dropped model's CUDAGraph, its
    page-locked buffers, its events -- and runtime calls made by those finalisers (hipGraphExecDestroy, hipHostFree, ...) are illegal
    on a capturing thread: round 4 saw the full GPU test suite die with SIGABRT inside `gc` in the middle of an encoder-plan capture."""

    def __enter__(self):
        import gc
        gc.collect()
        self._was = gc.isenabled()
        gc.disable()
        return self

    def __exit__(self, *exc):
        import gc
        if self._was:
            gc.enable()
        return False


class _Workspace:
    """One grow-only scratch buffer per (device, stream) (kernels never allocate).  Per STREAM since round 4: the joint step runs its
    RPN backward on a side stream beside the proposals / decoder chain, and two streams must not scribble over one scratch buffer.
    A buffer that is first asked for DURING a hipGraph capture (a capture runs on a stream of its own, after eager steps have seen
    every size) starts at the largest size any stream of the device has asked for, so that the capture never has to grow (= free) a
    buffer whose address earlier nodes have baked; outside a capture a new stream's buffer is sized by what that stream asks for
    (round 5, ADVICE r4: side / pipeline streams no longer pin a copy of the device-wide high-water mark each).  release() drops the
    buffers of streams the caller has retired; replacing or releasing an entry never frees memory a captured graph points into, because
    the captured step holds what handed_out() saw during its capture."""

    def __init__(self):
        self.buf = {}
        self.hi = {}
        self._seen = None             # {(device, stream handle): [buffers]} while handed_out() lasts

    def get(self, nbytes, device):
        if nbytes == 0:
            return None, 0
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        hi = max(self.hi.get(device, 0), nbytes)
        self.hi[device] = hi
        b = self.buf.get(key)
        if b is None or b.numel() < nbytes:
            want = hi if torch.cuda.is_current_stream_capturing() else nbytes + nbytes // 4
            b = torch.empty(max(want, 1 << 20), dtype=torch.uint8, device=device)
            self.buf[key] = b
        if self._seen is not None:
            held = self._seen.setdefault(key, [])
            if not any(h is b for h in held):
                held.append(b)
        return b, b.numel()

    @contextlib.contextmanager
    def handed_out(self):
        """While it lasts (a hipGraph capture), collect every buffer get() hands out, on whichever stream: yields the dictionary
        {(device, stream handle): [buffers]} the captured step keeps."""
        self._seen = seen = {}
        try:
            yield seen
        finally:
            self._seen = None

    def release(self, stream):
        """Drop the scratch buffer of a torch.cuda.Stream the caller is done with."""
        for key in [k for k in self.buf if k[1] == stream.cuda_stream]:
            del self.buf[key]


WORKSPACE = _Workspace()


def _launch_ws(nbytes, device, fn, *args):
    """fn(*args, workspace, workspace_bytes, stream) on the current stream, with its scratch buffer of at least nbytes (what the
    entry point's own dc_*_workspace_bytes call returned)."""
    ws, wsb = WORKSPACE.get(nbytes, device)
    check(fn(*args, _ptr(ws), wsb, _stream()), fn.__name__)


def _tile_info(info, tile_fn, d):
    """info= of the bf16 wrappers (tests / benches): which block tile and how many split-K slices run the problem `d`."""
    if info is not None:
        sk = C.c_int(0)
        info["tile"] = int(tile_fn(C.byref(d), C.byref(sk)))
        info["split_k"] = int(sk.value)


def _tile_config_info(info, config_fn, d):
    """info= of the fp32 wrappers (tests / benches): the block tile (bm, bn) and the split-K factor the library's own rule picks for the
    problem `d` (dc_gemm_tile_config, dc_conv2d_tile_config, dc_conv2d_wgrad_tile_config: host-only queries, nothing is launched)."""
    if info is not None:
        bm, bn, sk = C.c_int(0), C.c_int(0), C.c_int(0)
        check(config_fn(C.byref(d), C.byref(bm), C.byref(bn), C.byref(sk)), config_fn.__name__)
        info["tile"] = (int(bm.value), int(bn.value))
        info["split_k"] = int(sk.value)


def _scale_shift(d, scale, shift):
    d.scale = None if scale is None else _chk(scale, name="scale").data_ptr()
    d.shift = None if shift is None else _chk(shift, name="shift").data_ptr()


def _gemm_shape(fn, A, B, a_trans, b_trans, gather):
    """(M, N, K) of op(A) @ op(B), A's rows (a_trans: its K rows) picked by `gather` when given."""
    if a_trans:
        K, M = (gather.numel() if gather is not None else A.shape[0]), A.shape[1]
    elif gather is not None:
        M, K = gather.numel(), A.shape[1]
    else:
        M, K = A.shape
    N = B.shape[0] if b_trans else B.shape[1]
    kb = B.shape[1] if b_trans else B.shape[0]
    if kb != K:
        raise _lib.DcapError("%s: inner dimensions differ (%d vs %d)" % (fn, K, kb))
    return M, N, K


def _gemm_operands(d, M, N, K, A, B, a_trans, b_trans, gather):
    """The problem and the A / B operand fields dc_gemm_desc and dc_gemm_bf16_desc share."""
    d.M, d.N, d.K = M, N, K
    d.A, d.lda, d.a_trans = A.data_ptr(), A.stride(0), int(a_trans)
    d.a_gather = None if gather is None else _chk(gather, torch.int32, "gather").data_ptr()
    d.B, d.ldb, d.b_trans = B.data_ptr(), B.stride(0), int(b_trans)


def _gemm_epilogue(d, scale, shift, residual, res_rows, relu, accumulate, split_k):
    """The epilogue and split_k fields the two GEMM descriptors share."""
    _scale_shift(d, scale, shift)
    if residual is not None:
        _chk(residual, name="residual")
        d.residual, d.ldr, d.res_rows = residual.data_ptr(), residual.stride(0), int(res_rows)
    d.relu, d.accumulate, d.split_k = int(relu), int(accumulate), int(split_k)


def gemm(A, B, out=None, a_trans=False, b_trans=False, gather=None, scale=None, shift=None,
         residual=None, res_rows=0, relu=False, accumulate=False, split_k=0, info=None):
    """out[M,N] = epilogue(op(A) @ op(B)); see dc_gemm_f32.  info: a dict that receives "tile" (bm, bn) and "split_k" of the launch."""
    lib = _lib.load()
    _chk(A, name="A"), _chk(B, name="B")
    M, N, K = _gemm_shape("gemm", A, B, a_trans, b_trans, gather)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    _chk(out, name="out")
    if tuple(out.shape) != (M, N):
        raise _lib.DcapError("gemm: out has shape %s, expected %s" % (tuple(out.shape), (M, N)))
    d = GemmDesc()
    _gemm_operands(d, M, N, K, A, B, a_trans, b_trans, gather)
    d.C, d.ldc = out.data_ptr(), out.stride(0)
    _gemm_epilogue(d, scale, shift, residual, res_rows, relu, accumulate, split_k)
    _tile_config_info(info, lib.dc_gemm_tile_config, d)
    _launch_ws(lib.dc_gemm_workspace_bytes(C.byref(d)), A.device, lib.dc_gemm_f32, C.byref(d))
    return out


BF16 = torch.bfloat16


def from_bf16(x, out):
    """bf16 -> fp32 (exact) into `out` (dc_cast_bf16_f32); both contiguous, one size."""
    lib = _lib.load()
    if not (x.is_contiguous() and out.is_contiguous()) or x.numel() != out.numel():
        raise _lib.DcapError("from_bf16: contiguous tensors of one size")
    check(lib.dc_cast_bf16_f32(_ptr(_chk(x, BF16, "x")), _ptr(_chk(out, name="out")), x.numel(), _stream()), "dc_cast_bf16_f32")
    return out


def to_bf16(x, out=None, pad_cols=None):
    """fp32 -> bf16 (round to nearest even) on the device.  pad_cols: for a 2-D x, the output's column count (>= x.shape[1],
    extra columns zero) -- pads a contraction dimension to the multiple of 8 dc_gemm_bf16 wants."""
    lib = _lib.load()
    _chk(x, name="x")
    if pad_cols is not None or (x.dim() == 2 and not x.is_contiguous()):
        rows, cols = x.shape
        co = cols if pad_cols is None else int(pad_cols)
        if out is None:
            out = torch.empty((rows, co), dtype=BF16, device=x.device)
        check(lib.dc_cast_f32_bf16_2d(_ptr(x), x.stride(0), _ptr(out), out.stride(0), rows, cols, co, _stream()), "dc_cast_f32_bf16_2d")
        return out
    if not x.is_contiguous():
        raise _lib.DcapError("to_bf16: x must be contiguous (or 2-D with unit column stride)")
    if out is None:
        out = torch.empty(x.shape, dtype=BF16, device=x.device)
    check(lib.dc_cast_f32_bf16(_ptr(x), _ptr(out), x.numel(), _stream()), "dc_cast_f32_bf16")
    return out


def gemm_bf16(A, B, out=None, out_bf16=None, a_trans=False, b_trans=False, gather=None, scale=None, shift=None,
              residual=None, res_rows=0, relu=False, accumulate=False, split_k=0, info=None):
    """op(A) @ op(B) with bf16 operands, fp32 accumulate (dc_gemm_bf16).  out: fp32 [M,N] result (allocated when neither
    out nor out_bf16 is given); out_bf16: optional bf16 [M,N] copy of the result.  Returns out if present else out_bf16."""
    lib = _lib.load()
    _chk(A, BF16, "A"), _chk(B, BF16, "B")
    M, N, K = _gemm_shape("gemm_bf16", A, B, a_trans, b_trans, gather)
    if out is None and out_bf16 is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    d = GemmBf16Desc()
    _gemm_operands(d, M, N, K, A, B, a_trans, b_trans, gather)
    if gather is not None:
        d.a_gather_rows = A.shape[0]
    for t, name, dt in ((out, "out", torch.float32), (out_bf16, "out_bf16", BF16)):
        if t is not None and tuple(_chk(t, dt, name).shape) != (M, N):
            raise _lib.DcapError("gemm_bf16: %s has shape %s, expected %s" % (name, tuple(t.shape), (M, N)))
    if out is not None:
        d.C, d.ldc = out.data_ptr(), out.stride(0)
    if out_bf16 is not None:
        d.Cb, d.ldcb = out_bf16.data_ptr(), out_bf16.stride(0)
    _gemm_epilogue(d, scale, shift, residual, res_rows, relu, accumulate, split_k)
    _tile_info(info, lib.dc_gemm_bf16_tile, d)
    _launch_ws(lib.dc_gemm_bf16_workspace_bytes(C.byref(d)), A.device, lib.dc_gemm_bf16, C.byref(d))
    return out if out is not None else out_bf16


def _conv_geometry(d, x, Cout, kh, kw, stride, pad_t, pad_l, Ho, Wo):
    """The twelve geometry fields every convolution descriptor starts with; x [N,H,W,Cin]."""
    d.N, d.H, d.W, d.Cin = x.shape
    d.Cout, d.kh, d.kw, d.stride, d.pad_t, d.pad_l, d.Ho, d.Wo = Cout, kh, kw, stride, pad_t, pad_l, Ho, Wo


def conv2d(x, w_packed, kh, kw, stride, pad_t, pad_l, Ho, Wo, scale=None, shift=None, residual=None,
           res_mode=0, relu=False, out=None, split_k=0, math=0, w_wino=None, w_wino_b3=None, _name_only=False, info=None):
    """NHWC conv forward with fused epilogue; see dc_conv2d_nhwc_f32.  x [N,H,W,Cin] contiguous.  w_wino: winograd_pack(w_packed)
    of a frozen 3x3 / stride 1 / pad 1 kernel -> the layer runs in the Winograd F(2x2, 3x3) form (fp32, math=0 only).
    info: a dict that receives "tile" (bm, bn), "split_k" and "kernel" (dc_conv2d_kernel_name's answer) of the launch."""
    lib = _lib.load()
    _chk(x, name="x"), _chk(w_packed, name="w")
    N, H, W, Cin = x.shape
    Cout = w_packed.shape[0]
    if not x.is_contiguous() or not w_packed.is_contiguous():
        raise _lib.DcapError("conv2d: x and w must be contiguous")
    if out is None:
        out = torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    d = ConvDesc()
    _conv_geometry(d, x, Cout, kh, kw, stride, pad_t, pad_l, Ho, Wo)
    d.x, d.w, d.y = x.data_ptr(), w_packed.data_ptr(), _chk(out, name="out").data_ptr()
    _scale_shift(d, scale, shift)
    d.residual = None if residual is None else _chk(residual, name="residual").data_ptr()
    d.res_mode, d.relu, d.split_k, d.math = int(res_mode), int(relu), int(split_k), int(math)
    if w_wino is not None:
        if not w_wino.is_contiguous() or w_wino.numel() != 16 * Cin * Cout:
            raise _lib.DcapError("conv2d: w_wino must be the contiguous winograd_pack() of this layer's kernel (16*Cin*Cout floats)")
        d.w_wino = _chk(w_wino, name="w_wino").data_ptr()
    if w_wino_b3 is not None:
        if not w_wino_b3.is_contiguous() or w_wino_b3.numel() != 48 * Cin * Cout:
            raise _lib.DcapError("conv2d: w_wino_b3 must be the contiguous winograd_pack_b3() of this layer's kernel (48*Cin*Cout bf16)")
        d.w_wino_b3 = _chk(w_wino_b3, torch.int16, "w_wino_b3").data_ptr()
    if _name_only or info is not None:
        buf = C.create_string_buffer(128)
        check(lib.dc_conv2d_kernel_name(C.byref(d), buf, 128), "dc_conv2d_kernel_name")
        if _name_only:
            return buf.value.decode()
        info["kernel"] = buf.value.decode()
    _tile_config_info(info, lib.dc_conv2d_tile_config, d)
    _launch_ws(lib.dc_conv2d_workspace_bytes(C.byref(d)), x.device, lib.dc_conv2d_nhwc_f32, C.byref(d))
    return out


def conv2d_kernel_name(*args, **kw):
    """The kernel template instantiation conv2d(*args, **kw) would launch (dc_conv2d_kernel_name); nothing is launched."""
    return conv2d(*args, _name_only=True, **kw)


def pw_chain_supported(k1, n1, n2):
    return bool(_lib.load().dc_pw_chain_supported(int(k1), int(n1), int(n2)))


def _pw_chain_pack(fn, w_packed, out, pack, dtype, pieces):
    _chk(w_packed, name="w")
    if w_packed.dim() != 2 or not w_packed.is_contiguous():
        raise _lib.DcapError("%s: w must be the contiguous packed 1x1 kernel [Cout, Cin]" % fn)
    if out is None:
        out = torch.empty((w_packed.shape[0], pieces * w_packed.shape[1]), dtype=dtype, device=w_packed.device)
    check(pack(_ptr(w_packed), _ptr(out), w_packed.shape[0], w_packed.shape[1], _stream()), pack.__name__)
    return out


def pw_chain_pack(w_packed, out=None):
    """A packed 1x1 kernel [Cout, Cin] in the fragment order dc_pw_chain_f32 reads (same size)."""
    return _pw_chain_pack("pw_chain_pack", w_packed, out, pack=_lib.load().dc_pw_chain_pack_f32, dtype=torch.float32, pieces=1)


def pw_chain_pack_b3(w_packed, out=None):
    """A packed 1x1 kernel [Cout, Cin] as three bf16 pieces per element in the fragment order of the split-bf16 chain kernel:
    int16 [Cout, 3 * Cin] (dc_pw_chain_pack_b3)."""
    return _pw_chain_pack("pw_chain_pack_b3", w_packed, out, pack=_lib.load().dc_pw_chain_pack_b3, dtype=torch.int16, pieces=3)


def pw_chain(x, w1f, shift1, w2f, shift2, scale1=None, scale2=None, residual=None, relu1=True, relu2=True, y=None, z=None):
    """y = act1((x W1^T) scale1 + shift1 [+ residual]); z = act2((y W2^T) scale2 + shift2) in one launch (dc_pw_chain_f32).
    x [M, K1] (any leading dims), w1f / w2f: pw_chain_pack() of the packed kernels [N1, K1] / [N2, N1] (fp32 MFMA products), or both
    pw_chain_pack_b3() (int16 [N, 3 K]: the products on the bf16 pipe in split arithmetic).  Returns (y, z)."""
    lib = _lib.load()
    K1 = x.shape[-1]
    M = x.numel() // K1
    N1, N2 = w1f.shape[0], w2f.shape[0]
    b3 = w1f.dtype == torch.int16
    if b3 != (w2f.dtype == torch.int16):
        raise _lib.DcapError("pw_chain: both kernels in the same form (pw_chain_pack or pw_chain_pack_b3)")
    if w1f.shape[1] != (3 if b3 else 1) * K1 or w2f.shape[1] != (3 if b3 else 1) * N1:
        raise _lib.DcapError("pw_chain: kernel shapes do not chain: x [.., %d], w1 %s, w2 %s" % (K1, tuple(w1f.shape), tuple(w2f.shape)))
    if y is None:
        y = torch.empty(tuple(x.shape[:-1]) + (N1,), dtype=torch.float32, device=x.device)
    if z is None:
        z = torch.empty(tuple(x.shape[:-1]) + (N2,), dtype=torch.float32, device=x.device)
    for t in (x, y, z) + (() if residual is None else (residual,)):
        if not t.is_contiguous():
            raise _lib.DcapError("pw_chain: tensors must be contiguous")
    d = PwChainDesc()
    d.M, d.K1, d.N1, d.N2 = M, K1, N1, N2
    d.x, d.shift1, d.y = _chk(x, name="x").data_ptr(), _chk(shift1, name="shift1").data_ptr(), _chk(y, name="y").data_ptr()
    d.shift2, d.z = _chk(shift2, name="shift2").data_ptr(), _chk(z, name="z").data_ptr()
    if b3:
        d.w1_b3, d.w2_b3 = _chk(w1f, torch.int16, "w1").data_ptr(), _chk(w2f, torch.int16, "w2").data_ptr()
    else:
        d.w1, d.w2 = _chk(w1f, name="w1").data_ptr(), _chk(w2f, name="w2").data_ptr()
    d.scale1 = None if scale1 is None else _chk(scale1, name="scale1").data_ptr()
    d.scale2 = None if scale2 is None else _chk(scale2, name="scale2").data_ptr()
    d.residual = None if residual is None else _chk(residual, name="residual").data_ptr()
    d.relu1, d.relu2 = int(relu1), int(relu2)
    check(lib.dc_pw_chain_f32(C.byref(d), _stream()), "dc_pw_chain_f32")
    return y, z


def _winograd_pack(fn, w_packed, cin, cout, out, weight_bytes, pack, dtype):
    _chk(w_packed, name="w")
    if not w_packed.is_contiguous() or w_packed.numel() != 9 * cin * cout:
        raise _lib.DcapError("%s: w must be the contiguous packed 3x3 kernel [Cout, 9*Cin]" % fn)
    nbytes = weight_bytes(cin, cout)
    if nbytes == 0:
        raise _lib.DcapError("%s: Cin and Cout must be multiples of 32" % fn)
    if out is None:
        out = torch.empty((nbytes // dtype.itemsize,), dtype=dtype, device=w_packed.device)
    check(pack(_ptr(w_packed), _ptr(out), cin, cout, _stream()), pack.__name__)
    return out


def winograd_pack_b3(w_packed, cin, cout, out=None):
    """U = G g G^T of a packed 3x3 kernel [Cout, 9*Cin], every element as three bf16 pieces, in the fragment order of the split-bf16
    Winograd kernel: int16 [48*Cin*Cout] (dc_conv2d_winograd_pack_b3)."""
    lib = _lib.load()
    return _winograd_pack("winograd_pack_b3", w_packed, cin, cout, out, dtype=torch.int16,
                          weight_bytes=lib.dc_conv2d_winograd_b3_weight_bytes, pack=lib.dc_conv2d_winograd_pack_b3)


def winograd_pack(w_packed, cin, cout, out=None):
    """U = G g G^T of a packed 3x3 kernel [Cout, 9*Cin] in the fragment order the Winograd kernel reads: fp32 [16*Cin*Cout]."""
    lib = _lib.load()
    return _winograd_pack("winograd_pack", w_packed, cin, cout, out, dtype=torch.float32,
                          weight_bytes=lib.dc_conv2d_winograd_weight_bytes, pack=lib.dc_conv2d_winograd_pack_f32)


def split_bf16x3(x, out=None):
    """fp32 tensor -> int16 tensor [3, *x.shape] of bf16 bit patterns with x = p0 + p1 + p2 (pre-split conv weights)."""
    lib = _lib.load()
    _chk(x, name="x")
    if not x.is_contiguous():
        raise _lib.DcapError("split_bf16x3: x must be contiguous")
    if out is None:
        out = torch.empty((3,) + tuple(x.shape), dtype=torch.int16, device=x.device)
    check(lib.dc_split_bf16x3_f32(_ptr(x), _ptr(out), x.numel(), _stream()), "dc_split_bf16x3_f32")
    return out


def conv2d_wgrad(x, dy, kh, kw, stride, pad_t, pad_l, out=None, split_k=0, accumulate=False, info=None):
    """dw packed [Cout][kh*kw*Cin] = sum_pixels dy (x) im2col(x); x [N,H,W,Cin], dy [N,Ho,Wo,Cout] contiguous.
    info: a dict that receives "tile" (bm, bn) and "split_k" of the launch."""
    lib = _lib.load()
    _chk(x, name="x"), _chk(dy, name="dy")
    N, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    if not x.is_contiguous() or not dy.is_contiguous():
        raise _lib.DcapError("conv2d_wgrad: x and dy must be contiguous")
    if out is None:
        out = torch.empty((Cout, kh * kw * Cin), dtype=torch.float32, device=x.device)
    d = ConvDesc()
    _conv_geometry(d, x, Cout, kh, kw, stride, pad_t, pad_l, Ho, Wo)
    d.x, d.y, d.w, d.split_k = x.data_ptr(), dy.data_ptr(), _chk(out, name="dw").data_ptr(), int(split_k)
    d.accumulate = int(accumulate)
    _tile_config_info(info, lib.dc_conv2d_wgrad_tile_config, d)
    _launch_ws(lib.dc_conv2d_wgrad_workspace_bytes(C.byref(d)), x.device, lib.dc_conv2d_wgrad_f32, C.byref(d))
    return out


def conv2d_wgrad_bf16(x, dy, kh, kw, stride, pad_t, pad_l, out=None, split_k=0, accumulate=False, info=None):
    """conv2d_wgrad on the bf16 pipe: x [N,H,W,Cin] and dy [N,Ho,Wo,Cout] contiguous bf16; dw fp32 packed [Cout][kh*kw*Cin]."""
    lib = _lib.load()
    _chk(x, BF16, "x"), _chk(dy, BF16, "dy")
    N, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    if not x.is_contiguous() or not dy.is_contiguous():
        raise _lib.DcapError("conv2d_wgrad_bf16: x and dy must be contiguous")
    if out is None:
        out = torch.empty((Cout, kh * kw * Cin), dtype=torch.float32, device=x.device)
    d = ConvWgradBf16Desc()
    _conv_geometry(d, x, Cout, kh, kw, stride, pad_t, pad_l, Ho, Wo)
    d.x, d.dy, d.dw = x.data_ptr(), dy.data_ptr(), _chk(out, name="dw").data_ptr()
    d.accumulate, d.split_k = int(accumulate), int(split_k)
    _tile_info(info, lib.dc_conv2d_wgrad_bf16_tile, d)
    _launch_ws(lib.dc_conv2d_wgrad_bf16_workspace_bytes(C.byref(d)), x.device, lib.dc_conv2d_wgrad_bf16, C.byref(d))
    return out


def conv2d_bf16(x, w, kh, kw, stride, pad_t, pad_l, Ho, Wo, scale=None, shift=None, residual=None, res_mode=0, relu=False,
                out=None, out_bf16=None, want_f32=True, want_bf16=False, split_k=0, info=None, tile=0):
    """conv2d with bf16 storage (dc_conv2d_bf16): x [N,H,W,Cin] bf16 (Cin % 64 == 0), w packed [Cout, kh*kw*Cin] bf16; the fp32
    epilogue operands as in conv2d.  Returns (fp32 output or None, bf16 output or None)."""
    lib = _lib.load()
    _chk(x, BF16, "x"), _chk(w, BF16, "w")
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    if not x.is_contiguous() or not w.is_contiguous() or w.shape[1] != kh * kw * Cin:
        raise _lib.DcapError("conv2d_bf16: x must be contiguous NHWC, w contiguous [Cout, kh*kw*Cin]")
    if out is None and want_f32:
        out = torch.empty((N, Ho, Wo, Cout), dtype=torch.float32, device=x.device)
    if out_bf16 is None and want_bf16:
        out_bf16 = torch.empty((N, Ho, Wo, Cout), dtype=BF16, device=x.device)
    d = ConvBf16Desc()
    _conv_geometry(d, x, Cout, kh, kw, stride, pad_t, pad_l, Ho, Wo)
    d.x, d.w = x.data_ptr(), w.data_ptr()
    d.y = None if out is None else _chk(out, name="out").data_ptr()
    d.y_bf16 = None if out_bf16 is None else _chk(out_bf16, BF16, "out_bf16").data_ptr()
    _scale_shift(d, scale, shift)
    d.residual = None if residual is None else _chk(residual, name="residual").data_ptr()
    d.res_mode, d.relu, d.split_k, d.tile = int(res_mode), int(relu), int(split_k), int(tile)
    _tile_info(info, lib.dc_conv2d_bf16_tile, d)
    _launch_ws(lib.dc_conv2d_bf16_workspace_bytes(C.byref(d)), x.device, lib.dc_conv2d_bf16, C.byref(d))
    return out, out_bf16


def conv_bf16_supported(cin):
    return cin % 64 == 0


def wgrad_bf16_supported(x_shape, dy_shape):
    return x_shape[-1] % 128 == 0 and dy_shape[-1] % 8 == 0


def downsample2x_sum(fine, out=None, accumulate=False, out_bf16=None):
    """out (+)= the 2x2 block sums of fine [N,H,W,C] (the adjoint of UpSampling2D(2)); out_bf16: the bf16 copy of out, same pass."""
    lib = _lib.load()
    _chk(fine, name="fine")
    N, H, W, Cc = fine.shape
    if out is None:
        out = torch.empty((N, H // 2, W // 2, Cc), dtype=torch.float32, device=fine.device)
    check(lib.dc_downsample2x_sum_dual_f32(_ptr(fine), _ptr(out), None if out_bf16 is None else _ptr(_chk(out_bf16, BF16, "out_bf16")), N, H // 2, W // 2, Cc,
                                           int(accumulate), _stream()), "dc_downsample2x_sum_dual_f32")
    return out


def roi_align_pyramid_bwd(dmaps, boxes, image_area, dout, pool=7):
    """dmaps: four zero-initialised gradient maps [B,H,W,C] (accumulated into); dout [B,R,pool,pool,C]."""
    lib = _lib.load()
    B, R, _ = boxes.shape
    d = RoialignDesc()
    d.B, d.R, d.C, d.pool = B, R, dmaps[0].shape[-1], pool
    for i, m in enumerate(dmaps):
        if not _chk(m, name="dmap").is_contiguous():
            raise _lib.DcapError("roi_align_bwd: gradient maps must be contiguous")
        d.maps[i] = m.data_ptr()
        d.Hs[i], d.Ws[i] = m.shape[1], m.shape[2]
    d.boxes, d.image_area = _chk(boxes, name="boxes").data_ptr(), float(image_area)
    d.out = _chk(dout, name="dout").data_ptr()
    check(lib.dc_roi_align_pyramid_bwd_f32(C.byref(d), _stream()), "dc_roi_align_pyramid_bwd_f32")
    return dmaps


def maxpool3x3s2_same(x, out=None):
    lib = _lib.load()
    _chk(x, name="x")
    N, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((N, (H + 1) // 2, (W + 1) // 2, Cc), dtype=torch.float32, device=x.device)
    check(lib.dc_maxpool3x3s2_same_f32(_ptr(x), _ptr(out), N, H, W, Cc, _stream()), "dc_maxpool3x3s2_same_f32")
    return out


def maxpool2x2s2(x, out=None):
    """MaxPooling2D((2, 2), strides 2) on NHWC float32 (even H, W)."""
    lib = _lib.load()
    _chk(x, name="x")
    N, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((N, H // 2, W // 2, Cc), dtype=torch.float32, device=x.device)
    check(lib.dc_maxpool2x2s2_f32(_ptr(x), _ptr(out), N, H, W, Cc, _stream()), "dc_maxpool2x2s2_f32")
    return out


def mold_image_rgbx(img_u8, mean_pixel, out=None):
    lib = _lib.load()
    _chk(img_u8, torch.uint8, "images")
    N, H, W, c = img_u8.shape
    if c != 3 or not img_u8.is_contiguous():
        raise _lib.DcapError("mold_image: images must be contiguous [N,H,W,3] uint8")
    if out is None:
        out = torch.empty((N, H, W, 4), dtype=torch.float32, device=img_u8.device)
    check(lib.dc_mold_image_rgbx_f32(_ptr(img_u8), _ptr(out), N, H, W, float(mean_pixel[0]), float(mean_pixel[1]),
                                     float(mean_pixel[2]), _stream()), "dc_mold_image_rgbx_f32")
    return out


def mold_image_padded(img_u8, mean_pixel, out):
    """mold_image into pixels zero-padded to out.shape[-1] channels (a multiple of 4)."""
    lib = _lib.load()
    _chk(img_u8, torch.uint8, "images"), _chk(out, name="out")
    N, H, W, c = img_u8.shape
    if c != 3 or not img_u8.is_contiguous() or not out.is_contiguous() or tuple(out.shape[:3]) != (N, H, W):
        raise _lib.DcapError("mold_image_padded: images contiguous [N,H,W,3] uint8, out contiguous [N,H,W,C]")
    check(lib.dc_mold_image_padded_f32(_ptr(img_u8), _ptr(out), N, H, W, out.shape[3], float(mean_pixel[0]), float(mean_pixel[1]),
                                       float(mean_pixel[2]), _stream()), "dc_mold_image_padded_f32")
    return out


def _resize_flips(flips, B, who):
    """flips= of the resize wrappers: None, or one boolean per image -> int32 [B] of 0 / 1."""
    if flips is None:
        return None
    f = np.asarray(flips)
    if f.ndim != 1 or f.shape[0] != B:
        raise ValueError("%s: flips must hold one flag per image (%d), got shape %s" % (who, B, tuple(f.shape)))
    return np.ascontiguousarray(f.astype(bool), np.int32)


def pack_resize_batch(images, placements, flips=None):
    """The one host buffer of a resize_pad_packed() call: `images` (uint8 [h,w,3] arrays of any sizes) and, per image, its placement
    (new_h, new_w, top, left) -> (packed uint8 [bytes], records int32 [B,_lib.RESIZE_RECORD_INTS]).  `packed` starts with the records
    {byte offset, h, w, new_h, new_w, top, left, the intermediate's byte offset in the workspace} and holds the raw bytes end to
    end behind them; `records` is the host's own copy.  Anything but a uint8 [h,w,3] array is refused (ValueError: mold="host").
    flips (one boolean per image, or None: today's buffer): the flags of dc_resize_pad_flip_u8 travel as an int32 [B] block between
    the records and the first image, at byte B * _lib.RESIZE_RECORD_INTS * 4."""
    from . import utils
    images = [utils.check_device_mold_image(im) for im in images]
    B, R = len(images), _lib.RESIZE_RECORD_INTS
    if B < 1 or len(placements) != B:
        raise ValueError("pack_resize_batch: one placement (new_h, new_w, top, left) per image and at least one image")
    flags = _resize_flips(flips, B, "pack_resize_batch")
    records = np.zeros((B, R), np.int32)
    head = B * R * 4
    pos, mid = head + (0 if flags is None else B * 4), 0
    for b, (im, (new_h, new_w, top, left)) in enumerate(zip(images, placements)):
        h, w = im.shape[:2]
        if max(pos + h * w * 3, mid + h * int(new_w) * 3) >= 1 << 31:
            raise ValueError("pack_resize_batch: the batch's bytes must stay below 2^31; split it, or pass mold=\"host\"")
        records[b] = (pos, h, w, new_h, new_w, top, left, mid)
        pos += h * w * 3
        mid += h * int(new_w) * 3
    packed = np.empty(pos, np.uint8)
    packed[:head] = records.view(np.uint8).reshape(-1)
    if flags is not None:
        packed[head:head + B * 4] = flags.view(np.uint8)
    for im, r in zip(images, records):
        packed[r[0]:r[0] + im.size].reshape(im.shape)[...] = im
    return packed, records


def resize_pad_packed(packed, records, canvas=None, out=None, flips=None):
    """dc_resize_pad_u8 on an already uploaded batch: `packed` the device copy of pack_resize_batch()'s buffer, `records` its host
    records.  Writes EVERY byte of out (uint8 [B,H,W,3], contiguous; made from canvas=(H, W) when not given): image b resampled as
    PIL.Image.resize(BILINEAR) does it, at its (top, left), zeros elsewhere.  Enqueue-only on the current stream.
    flips (the sequence pack_resize_batch(flips=) was given; None: the call above): dc_resize_pad_flip_u8 -- a flagged image's canvas
    is mirrored left to right, padding included (load_image_gt's image[:, ::-1])."""
    lib = _lib.load()
    records = np.ascontiguousarray(records, np.int32)
    B = records.shape[0]
    if _chk(packed, torch.uint8, "packed").dim() != 1 or records.ndim != 2 or records.shape[1] != _lib.RESIZE_RECORD_INTS:
        raise _lib.DcapError("resize_pad_packed: packed must be a 1-D uint8 tensor and records int32 [B,%d]" % _lib.RESIZE_RECORD_INTS)
    flags = _resize_flips(flips, B, "resize_pad_packed")
    if out is None:
        out = torch.empty((B, int(canvas[0]), int(canvas[1]), 3), dtype=torch.uint8, device=packed.device)
    if not _chk(out, torch.uint8, "out").is_contiguous() or out.dim() != 4 or out.shape[0] != B or out.shape[3] != 3 or out.device != packed.device:
        raise _lib.DcapError("resize_pad_packed: out must be a contiguous uint8 [%d,H,W,3] tensor on packed's device" % B)
    d = ResizePadDesc()
    d.B, d.packed, d.packed_bytes, d.records = B, packed.data_ptr(), packed.numel(), records.ctypes.data
    d.out, d.H, d.W = out.data_ptr(), out.shape[1], out.shape[2]
    need = lib.dc_resize_pad_u8_workspace_bytes(C.byref(d))
    if flags is None:
        _launch_ws(need, packed.device, lib.dc_resize_pad_u8, C.byref(d))
    else:
        _launch_ws(need, packed.device, lib.dc_resize_pad_flip_u8, C.byref(d), flags.ctypes.data, B * _lib.RESIZE_RECORD_INTS * 4)
    return out


def resize_pad_images(images, min_dim=None, max_dim=None, padding=True, placements=None, canvas=None, out=None, device=None, flips=None):
    """utils.resize_image + np.pad + np.stack on the device, bit for bit: `images` (a list of uint8 [h,w,3] arrays of any sizes) are
    packed (pack_resize_batch), uploaded in ONE blocking copy and resampled into a uint8 [B,H,W,3] device tensor (returned; `out`
    is filled when given, every byte of it).  The geometry is utils.resize_geometry's for (min_dim, max_dim) with the canvas
    max_dim x max_dim, or explicit: placements [(new_h, new_w, top, left)] and canvas (H, W) or out.
    flips: one boolean per image (None: none) -- a flagged image's square is mirrored left to right (resize_pad_packed).
    Refused with a ValueError that names mold="host": images that are not uint8 [h,w,3], and padding=False."""
    from . import utils
    utils.check_mold("device", padding)
    images = [utils.check_device_mold_image(im) for im in images]
    if placements is None:
        geo = [utils.resize_geometry(im.shape, min_dim, max_dim, True) for im in images]
        placements, canvas = [(g[0], g[1], g[2][0], g[2][1]) for g in geo], (max_dim, max_dim)
    packed, records = pack_resize_batch(images, placements, flips)
    dev = out.device if out is not None else torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
    return resize_pad_packed(torch.from_numpy(packed).to(dev), records, canvas, out, flips)


def roi_align_pyramid(maps, boxes, image_area, pool=7, out=None, levels_out=None):
    """maps: [P2,P3,P4,P5] each [B,H,W,C]; boxes [B,R,4] normalised float32 -> [B,R,pool,pool,C]."""
    lib = _lib.load()
    B, R, _ = boxes.shape
    Cc = maps[0].shape[-1]
    _chk(boxes, name="boxes")
    if not boxes.is_contiguous():
        raise _lib.DcapError("roi_align: boxes must be contiguous")
    if out is None:
        out = torch.empty((B, R, pool, pool, Cc), dtype=torch.float32, device=boxes.device)
    d = RoialignDesc()
    d.B, d.R, d.C, d.pool = B, R, Cc, pool
    for i, m in enumerate(maps):
        _chk(m, name="map")
        if not m.is_contiguous() or m.shape[0] != B or m.shape[-1] != Cc:
            raise _lib.DcapError("roi_align: feature maps must be contiguous [B,H,W,C]")
        d.maps[i] = m.data_ptr()
        d.Hs[i], d.Ws[i] = m.shape[1], m.shape[2]
    d.boxes, d.image_area, d.out = boxes.data_ptr(), float(image_area), out.data_ptr()
    d.levels_out = None if levels_out is None else _chk(levels_out, torch.int32, "levels").data_ptr()
    check(lib.dc_roi_align_pyramid_f32(C.byref(d), _stream()), "dc_roi_align_pyramid_f32")
    return out


class RoiTileGroups(object):
    """Device buffers of dc_roi_tile_groups for a batch of B images whose pyramid levels have the extents `hw` [(H, W)] * 4: per level a
    list of tile-group indices (int32, as long as the level has groups) and, in counts[level], how many of them the last
    roi_tile_groups() call listed.  lat_list / lat_count: the tiles of the level-2 lateral map the list-driven fpn_p2 reads (the listed
    level-2 groups and their neighbours in the group grid), written by roi_tile_groups(..., lateral=True) only.  Nothing here is ever
    read by the host on the hot path."""

    def __init__(self, B, hw, device):
        lib = _lib.load()
        self.B, self.hw = int(B), [(int(h), int(w)) for h, w in hw]
        if len(self.hw) != 4:
            raise _lib.DcapError("RoiTileGroups: four pyramid levels expected")
        self.per_image = [lib.dc_conv2d_winograd_group_count(h, w) for h, w in self.hw]
        self.lists = [torch.zeros(self.B * n, dtype=torch.int32, device=device) for n in self.per_image]
        self.counts = torch.zeros(4, dtype=torch.int32, device=device)
        self.marks = torch.zeros(self.B * sum(self.per_image), dtype=torch.int32, device=device)
        self.lat_list = torch.zeros(self.B * self.per_image[0], dtype=torch.int32, device=device)
        self.lat_count = torch.zeros(1, dtype=torch.int32, device=device)

    def count_ptr(self, level):
        return C.c_void_p(self.counts.data_ptr() + 4 * level)


def roi_tile_groups(boxes, groups, image_area, pool=7, lateral=False):
    """The tile groups of P2..P5 that roi_align_pyramid(maps, boxes, image_area, pool) reads, into `groups` (RoiTileGroups): the same
    routing and sampling decisions, taken by the same device functions.  boxes [B,R,4] normalised float32.  lateral: the same launch
    also lists, in groups.lat_list / lat_count, the level-2 tiles within one pixel of a listed level-2 group (dc_roi_tile_groups_lateral)."""
    lib = _lib.load()
    _chk(boxes, name="boxes")
    B, R, _ = boxes.shape
    if not boxes.is_contiguous() or B != groups.B:
        raise _lib.DcapError("roi_tile_groups: boxes must be contiguous [B,R,4] with the B the group buffers were made for")
    d = RoiGroupsDesc()
    d.B, d.R, d.pool = B, R, pool
    for i, (h, w) in enumerate(groups.hw):
        d.Hs[i], d.Ws[i] = h, w
        d.lists[i] = groups.lists[i].data_ptr()
    d.boxes, d.image_area = boxes.data_ptr(), float(image_area)
    d.marks, d.counts = groups.marks.data_ptr(), groups.counts.data_ptr()
    if lateral:
        check(lib.dc_roi_tile_groups_lateral(C.byref(d), _ptr(groups.lat_list), _ptr(groups.lat_count), _stream()), "dc_roi_tile_groups_lateral")
    else:
        check(lib.dc_roi_tile_groups(C.byref(d), _stream()), "dc_roi_tile_groups")
    return groups


def conv2d_tiles(x, w_packed, tile_list, count, out, scale=None, shift=None, residual=None, res_mode=0, relu=False, split_k=1,
                 math=_lib.MATH_BF16X3):
    """The 1x1 / stride 1 layer of conv2d(x, w_packed, 1, 1, 1, 0, 0, H, W, ..., split_k=1, math=1) on the 8 x 16-pixel tile groups of
    `tile_list` only (int32 device tensor of group indices; `count`: int32 device tensor whose first element is the list's length).
    Listed tiles of `out` get conv2d's values bit for bit, nothing else of it is written.  dc_conv2d_nhwc_tiles_f32."""
    lib = _lib.load()
    _chk(x, name="x"), _chk(w_packed, name="w"), _chk(out, name="out")
    _chk(tile_list, torch.int32, "tile_list"), _chk(count, torch.int32, "count")
    N, H, W, Cin = x.shape
    Cout = w_packed.shape[0]
    if not x.is_contiguous() or not w_packed.is_contiguous() or not out.is_contiguous() or tuple(out.shape) != (N, H, W, Cout):
        raise _lib.DcapError("conv2d_tiles: x, w and out must be contiguous, out [N,H,W,Cout]")
    if tuple(w_packed.shape) != (Cout, Cin):
        raise _lib.DcapError("conv2d_tiles: w must be the packed kernel of a 1x1 layer, [Cout][Cin]")
    if tile_list.numel() < N * lib.dc_conv2d_winograd_group_count(H, W) or count.numel() < 1:
        raise _lib.DcapError("conv2d_tiles: the list must have room for every tile group of the map")
    if residual is not None and (not _chk(residual, name="residual").is_contiguous() or tuple(residual.shape) != (N, H // 2, W // 2, Cout)):
        raise _lib.DcapError("conv2d_tiles: the upsample-add operand must be contiguous [N,H/2,W/2,Cout]")
    d = ConvDesc()
    _conv_geometry(d, x, Cout, 1, 1, 1, 0, 0, H, W)
    d.x, d.w, d.y = x.data_ptr(), w_packed.data_ptr(), out.data_ptr()
    _scale_shift(d, scale, shift)
    d.residual = None if residual is None else residual.data_ptr()
    d.res_mode, d.relu, d.split_k, d.math = int(res_mode), int(relu), int(split_k), int(math)
    check(lib.dc_conv2d_nhwc_tiles_f32(C.byref(d), _ptr(tile_list), _ptr(count), _stream()), "dc_conv2d_nhwc_tiles_f32")
    return out


def _nhwc_same_out(fn, x, w, out):
    """The operand checks of the list-driven Winograd wrappers: x [N,H,W,Cin], packed kernel w, out [N,H,W,Cout] -> (N, H, W, Cin, Cout)."""
    _chk(x, name="x"), _chk(w, name="w"), _chk(out, name="out")
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    if not x.is_contiguous() or not out.is_contiguous() or tuple(out.shape) != (N, H, W, Cout):
        raise _lib.DcapError("%s: x and out must be contiguous [N,H,W,C]" % fn)
    return N, H, W, Cin, Cout


def _wino_b3_fill(d, x, w, u, out, scale, shift, relu):
    """d: the 3x3 / stride 1 / 'same' layer the split-bf16 Winograd kernel runs on listed tile groups (u: its winograd_pack_b3)."""
    _conv_geometry(d, x, w.shape[0], 3, 3, 1, 1, 1, x.shape[1], x.shape[2])
    d.x, d.w, d.y = x.data_ptr(), w.data_ptr(), out.data_ptr()
    _scale_shift(d, scale, shift)
    d.relu = int(relu)
    d.w_wino_b3 = _chk(u, torch.int16, "w_wino_b3").data_ptr()


def conv2d_winograd_groups(x, w_packed, w_wino_b3, group_list, count, out, scale=None, shift=None, relu=False):
    """The 3x3 / stride 1 / 'same' layer of conv2d(..., w_wino_b3=...) on the tile groups of `group_list` only (int32 device tensor;
    `count`: int32 device tensor whose first element is the list's length).  Listed groups of `out` get conv2d's values bit for bit,
    nothing else of it is written.  dc_conv2d_winograd_groups_f32."""
    lib = _lib.load()
    _chk(group_list, torch.int32, "group_list"), _chk(count, torch.int32, "count")
    N, H, W, Cin, Cout = _nhwc_same_out("conv2d_winograd_groups", x, w_packed, out)
    if not w_wino_b3.is_contiguous() or w_wino_b3.numel() != 48 * Cin * Cout:
        raise _lib.DcapError("conv2d_winograd_groups: w_wino_b3 must be the contiguous winograd_pack_b3() of this layer's kernel")
    if group_list.numel() < N * lib.dc_conv2d_winograd_group_count(H, W) or count.numel() < 1:
        raise _lib.DcapError("conv2d_winograd_groups: the list must have room for every tile group of the layer")
    d = ConvDesc()
    _wino_b3_fill(d, x, w_packed, w_wino_b3, out, scale, shift, relu)
    check(lib.dc_conv2d_winograd_groups_f32(C.byref(d), _ptr(group_list), _ptr(count), _stream()), "dc_conv2d_winograd_groups_f32")
    return out


def conv2d_winograd_levels(xs, ws_packed, ws_wino_b3, lists, counts, outs, scales=None, shifts=None, relu=False):
    """conv2d_winograd_groups for up to four layers of equal Cin, Cout and relu in ONE launch: per level l the input xs[l], the packed
    kernel, its winograd_pack_b3, the group list lists[l] and the output outs[l]; counts: int32 device tensor, level l's count at
    counts[l].  dc_conv2d_winograd_levels_f32."""
    lib = _lib.load()
    n = len(xs)
    if not 1 <= n <= 4 or any(len(v) != n for v in (ws_packed, ws_wino_b3, lists, outs)):
        raise _lib.DcapError("conv2d_winograd_levels: one to four levels, every argument one entry per level")
    _chk(counts, torch.int32, "counts")
    if counts.numel() < n:
        raise _lib.DcapError("conv2d_winograd_levels: counts must hold one entry per level")
    descs, ptrs = (ConvDesc * n)(), (C.c_void_p * n)()
    for l in range(n):
        x, w, u, out = xs[l], ws_packed[l], ws_wino_b3[l], outs[l]
        _chk(lists[l], torch.int32, "list")
        N, H, W, Cin, Cout = _nhwc_same_out("conv2d_winograd_levels", x, w, out)
        if not u.is_contiguous() or u.numel() != 48 * Cin * Cout:
            raise _lib.DcapError("conv2d_winograd_levels: w_wino_b3 must be the contiguous winograd_pack_b3() of the layer's kernel")
        if lists[l].numel() < N * lib.dc_conv2d_winograd_group_count(H, W):
            raise _lib.DcapError("conv2d_winograd_levels: a list must have room for every tile group of its layer")
        _wino_b3_fill(descs[l], x, w, u, out, None if scales is None else scales[l], None if shifts is None else shifts[l],
                      relu[l] if isinstance(relu, (list, tuple)) else relu)
        ptrs[l] = lists[l].data_ptr()
    check(lib.dc_conv2d_winograd_levels_f32(descs, n, ptrs, _ptr(counts), _stream()), "dc_conv2d_winograd_levels_f32")
    return outs


def subsample2(x, out=None):
    lib = _lib.load()
    _chk(x, name="x")
    N, H, W, Cc = x.shape
    if out is None:
        out = torch.empty((N, (H + 1) // 2, (W + 1) // 2, Cc), dtype=torch.float32, device=x.device)
    check(lib.dc_subsample2_f32(_ptr(x), _ptr(out), N, H, W, Cc, _stream()), "dc_subsample2_f32")
    return out


def rpn_proposals(heads, anchors, image_hw, proposal_count, nms_threshold, std_dev=(0.1, 0.1, 0.2, 0.2), pre_nms_limit=6000,
                  anchors_per_loc=3, out=None, debug=False, head_stride=0):
    """heads: per-level fused RPN head outputs [B,H,W,A*6]; anchors [A_total,4] float32 device tensor.
    Returns proposals [B,count,4] (normalised, zero padded) and, with debug, (scores, order, keep)."""
    lib = _lib.load()
    B = heads[0].shape[0]
    d = ProposalDesc()
    d.B, d.levels, d.anchors_per_loc = B, len(heads), anchors_per_loc
    for i, h in enumerate(heads):
        if not _chk(h, name="head").is_contiguous() or h.shape[-1] != (head_stride or anchors_per_loc * 6):
            raise _lib.DcapError("rpn_proposals: heads must be contiguous [B,H,W,A*6] (or [B,H,W,head_stride])")
        d.heads[i] = h.data_ptr()
        d.Hs[i], d.Ws[i] = h.shape[1], h.shape[2]
    d.head_stride = int(head_stride)
    d.anchors, d.A_total = _chk(anchors, name="anchors").data_ptr(), anchors.shape[0]
    for i in range(4):
        d.std_dev[i] = float(std_dev[i])
    d.image_h, d.image_w = float(image_hw[0]), float(image_hw[1])
    d.pre_nms_limit, d.proposal_count, d.nms_threshold = int(pre_nms_limit), int(proposal_count), float(nms_threshold)
    dev = heads[0].device
    if out is None:
        out = torch.empty((B, proposal_count, 4), dtype=torch.float32, device=dev)
    d.proposals = out.data_ptr()
    extra = None
    if debug:
        k = min(pre_nms_limit, anchors.shape[0])
        extra = (torch.empty((B, anchors.shape[0]), dtype=torch.float32, device=dev),
                 torch.empty((B, k), dtype=torch.int32, device=dev),
                 torch.empty((B, proposal_count), dtype=torch.int32, device=dev))
        d.scores_out, d.order_out, d.keep_out = (t.data_ptr() for t in extra)
    _launch_ws(lib.dc_proposals_workspace_bytes(C.byref(d)), dev, lib.dc_proposals_f32, C.byref(d))
    return (out, extra) if debug else out


def refine_generations(rois, image_consts, threshold, max_instances, word_scores=None, caption_scores=None):
    """GenerationMatchLayer + unmold_generations for B images x N RoIs on the device (dc_refine_generations_f64), in float64 by the host
    path's operations: rois float32 [B,N,4] normalised; exactly one of word_scores float32 [B*N,T] (caption score = sum of log p in index
    order) and caption_scores float32 [B*N] with any element stride (column 0 of the beam decoder's [B*N,k] scores); image_consts
    float64 [B,_lib.REFINE_CONSTS] (per image: window y1 x1 y2 x2, IMAGE_SHAPE h w, unmold_generations' shift y x and scale, one unused
    word).  Returns device tensors (boxes int32 [B,max_instances,4] in the original image's pixels, keep int32 [B,max_instances]: each
    survivor's RoI index in score order, -1 after the last, count int32 [B], scores float64 [B,N]).  N <= _lib.REFINE_MAX_ROIS.  No host
    synchronisation; B = 0 or N = 0 returns the empty result without a launch."""
    lib = _lib.load()
    if not _chk(rois, name="rois").is_contiguous() or rois.dim() != 3 or rois.shape[2] != 4:
        raise _lib.DcapError("refine_generations: rois must be a contiguous float32 [B,N,4] tensor")
    B, N = rois.shape[0], rois.shape[1]
    if (word_scores is None) == (caption_scores is None):
        raise _lib.DcapError("refine_generations: exactly one of word_scores and caption_scores")
    if isinstance(max_instances, bool) or int(max_instances) != max_instances or max_instances < 1:
        raise _lib.DcapError("refine_generations: max_instances must be a positive integer, got %r" % (max_instances,))
    if N > _lib.REFINE_MAX_ROIS:
        raise _lib.DcapError("refine_generations: N = %d exceeds the NMS scan's limit of %d RoIs per image" % (N, _lib.REFINE_MAX_ROIS))
    d = RefineDesc()
    if word_scores is not None:
        if not _chk(word_scores, name="word_scores").is_contiguous() or word_scores.dim() != 2 or word_scores.shape[0] != B * N or (
                word_scores.shape[1] < 1 and B * N > 0):
            raise _lib.DcapError("refine_generations: word_scores must be a contiguous float32 [B*N,T] tensor, T >= 1")
        d.T, d.word_scores = word_scores.shape[1], word_scores.data_ptr()
    else:
        c = caption_scores
        if not c.is_cuda:
            raise _lib.DcapError("caption_scores must live on the GPU (no CPU path exists)")
        if c.dtype != torch.float32 or c.dim() != 1 or c.shape[0] != B * N or (B * N > 1 and c.stride(0) < 1):
            raise _lib.DcapError("refine_generations: caption_scores must be a float32 [B*N] tensor (any positive element stride)")
        d.caption_stride, d.caption_scores = (c.stride(0) if B * N > 1 else 1), c.data_ptr()
    if not _chk(image_consts, torch.float64, "image_consts").is_contiguous() or tuple(image_consts.shape) != (B, _lib.REFINE_CONSTS):
        raise _lib.DcapError("refine_generations: image_consts must be a contiguous float64 [B,%d] tensor" % _lib.REFINE_CONSTS)
    M, dev = int(max_instances), rois.device
    scores = torch.empty((B, N), dtype=torch.float64, device=dev)
    if B == 0 or N == 0:
        return (torch.zeros((B, M, 4), dtype=torch.int32, device=dev), torch.full((B, M), -1, dtype=torch.int32, device=dev),
                torch.zeros((B,), dtype=torch.int32, device=dev), scores)
    boxes = torch.empty((B, M, 4), dtype=torch.int32, device=dev)
    keep = torch.empty((B, M), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    d.B, d.N, d.rois, d.image_consts, d.threshold, d.max_instances = B, N, rois.data_ptr(), image_consts.data_ptr(), float(threshold), M
    d.boxes_out, d.keep_out, d.count_out, d.scores_out = boxes.data_ptr(), keep.data_ptr(), count.data_ptr(), scores.data_ptr()
    _launch_ws(lib.dc_refine_generations_workspace_bytes(C.byref(d)), dev, lib.dc_refine_generations_f64, C.byref(d))
    return boxes, keep, count, scores


def _rec_masks(rec_masks, B, U):
    if rec_masks is None:
        return None
    if tuple(_chk(rec_masks, name="rec_masks").shape) != (4, B, U) or not rec_masks.is_contiguous():
        raise _lib.DcapError("rec_masks must be a contiguous float32 [4,B,U] tensor")
    return rec_masks.data_ptr()


def _lstm_step_info(info, B, U, direction, rec_masks):
    """info= of the LSTM wrappers (tests / benches): the block of the fused step kernel the library's own rule picks for (B, U) --
    "rows" batch rows and "waves" waves per block, both 0 where the step is not fused (dc_lstm_step_tile_config: a host-only query)."""
    if info is not None:
        rows, waves = C.c_int(0), C.c_int(0)
        check(_lib.load().dc_lstm_step_tile_config(B, U, direction, int(rec_masks), C.byref(rows), C.byref(waves)), "dc_lstm_step_tile_config")
        info["rows"] = int(rows.value)
        info["waves"] = int(waves.value)


def lstm_seq_fwd(z, U_rec, mask, B, T, h_seq=None, c_seq=None, rec_masks=None, info=None):
    """z [T*B,4U] (x-projection + bias, overwritten with the full pre-activation) -> h_seq, c_seq [T*B,U].
    rec_masks [4,B,U]: Keras recurrent_dropout masks (training phase); None = no dropout.
    info: a dict that receives "rows" and "waves" of the fused step's block (0, 0: not fused at this U)."""
    lib = _lib.load()
    U = U_rec.shape[0]
    _chk(z, name="z"), _chk(U_rec, name="U_rec")
    if not z.is_contiguous() or not U_rec.is_contiguous() or tuple(z.shape) != (T * B, 4 * U):
        raise _lib.DcapError("lstm_seq_fwd: z must be contiguous [T*B,4U], U_rec contiguous [U,4U]")
    if h_seq is None:
        h_seq = torch.empty((T * B, U), dtype=torch.float32, device=z.device)
    if c_seq is None:
        c_seq = torch.empty((T * B, U), dtype=torch.float32, device=z.device)
    d = LstmFwdDesc()
    d.B, d.T, d.U = B, T, U
    d.z, d.U_rec = z.data_ptr(), U_rec.data_ptr()
    d.mask = None if mask is None else _chk(mask, torch.uint8, "mask").data_ptr()
    d.h_seq, d.c_seq = h_seq.data_ptr(), c_seq.data_ptr()
    d.rec_masks = _rec_masks(rec_masks, B, U)
    _lstm_step_info(info, B, U, 0, rec_masks is not None)
    _launch_ws(lib.dc_lstm_seq_workspace_bytes(B, T, U), z.device, lib.dc_lstm_seq_fwd_f32, C.byref(d))
    return h_seq, c_seq


def lstm_pack_urec(U_rec, out=None):
    """The line-contiguous copy of the recurrent kernel [U,4U] that lstm_step's fused step reads (dc_lstm_pack_urec_f32; U % 32 == 0):
    made once per decode instead of once per step."""
    _chk(U_rec, name="U_rec")
    lib = _lib.load()
    U = U_rec.shape[0]
    if not U_rec.is_contiguous() or tuple(U_rec.shape) != (U, 4 * U):
        raise _lib.DcapError("lstm_pack_urec: U_rec must be contiguous [U,4U]")
    if out is None:
        out = torch.empty((U, 4 * U), dtype=torch.float32, device=U_rec.device)
    if not _chk(out, name="out").is_contiguous() or out.numel() != 4 * U * U:
        raise _lib.DcapError("lstm_pack_urec: out must be a contiguous tensor of 4*U*U floats")
    check(lib.dc_lstm_pack_urec_f32(_ptr(U_rec), U, _ptr(out), _stream()), "dc_lstm_pack_urec_f32")
    return out


def lstm_step(z, U_rec, h_prev=None, c_prev=None, mask=None, h=None, c=None, U_packed=None, info=None):
    """ONE LSTM timestep with carried state (dc_lstm_step_f32): z [B,4U] (x-projection + bias, overwritten with the full pre-activation),
    h_prev / c_prev [B,U] (None: zeros), mask uint8 [B] (None: every row live; rows with 0 copy h_prev / c_prev) -> h, c [B,U].
    U_packed: lstm_pack_urec(U_rec) (None: repacked on every call when U % 32 == 0).
    info: a dict that receives "rows" and "waves" of the fused step's block, as lstm_seq_fwd's does at the same B."""
    _chk(z, name="z"), _chk(U_rec, name="U_rec")
    lib = _lib.load()
    U = U_rec.shape[0]
    B = z.shape[0]
    if not z.is_contiguous() or not U_rec.is_contiguous() or tuple(z.shape) != (B, 4 * U) or tuple(U_rec.shape) != (U, 4 * U):
        raise _lib.DcapError("lstm_step: z must be contiguous [B,4U], U_rec contiguous [U,4U]")
    if (h_prev is None) != (c_prev is None):
        raise _lib.DcapError("lstm_step: h_prev and c_prev are both given or both None")
    h = torch.empty((B, U), dtype=torch.float32, device=z.device) if h is None else h
    c = torch.empty((B, U), dtype=torch.float32, device=z.device) if c is None else c
    for name, t in (("h_prev", h_prev), ("c_prev", c_prev), ("h", h), ("c", c)):
        if t is not None and (not _chk(t, name=name).is_contiguous() or tuple(t.shape) != (B, U)):
            raise _lib.DcapError("lstm_step: %s must be contiguous [B,U]" % name)
    if mask is not None and (not _chk(mask, torch.uint8, "mask").is_contiguous() or mask.numel() != B):
        raise _lib.DcapError("lstm_step: mask must be a contiguous uint8 [B] tensor")
    if U_packed is not None and (not _chk(U_packed, name="U_packed").is_contiguous() or U_packed.numel() != 4 * U * U):
        raise _lib.DcapError("lstm_step: U_packed must be lstm_pack_urec's contiguous 4*U*U floats")
    if B == 0:
        return h, c
    d = LstmStepDesc()
    d.B, d.U = B, U
    d.z, d.U_rec, d.U_packed = z.data_ptr(), U_rec.data_ptr(), _ptr(U_packed)
    d.h_prev, d.c_prev, d.mask = _ptr(h_prev), _ptr(c_prev), _ptr(mask)
    d.h, d.c = h.data_ptr(), c.data_ptr()
    _lstm_step_info(info, B, U, 0, False)
    _launch_ws(lib.dc_lstm_step_workspace_bytes(B, U), z.device, lib.dc_lstm_step_f32, C.byref(d))
    return h, c


def lstm_seq_bwd(z, U_rec, mask, h_seq, c_seq, B, T, dh_seq=None, dh_last=None, dz=None, dU=None, accumulate_dU=False, rec_masks=None, info=None):
    """info: a dict that receives "rows" and "waves" of the fused backward step's block (0, 0: not fused at this U)."""
    lib = _lib.load()
    U = U_rec.shape[0]
    if dz is None:
        dz = torch.empty((T * B, 4 * U), dtype=torch.float32, device=z.device)
    if dU is None:
        dU = torch.empty((U, 4 * U), dtype=torch.float32, device=z.device)
    elif dU is False:                                  # the caller forms the recurrent kernel's gradient itself (returns (dz, None))
        dU = None
    d = LstmBwdDesc()
    d.B, d.T, d.U = B, T, U
    d.z, d.U_rec = _chk(z, name="z").data_ptr(), _chk(U_rec, name="U_rec").data_ptr()
    d.mask = None if mask is None else _chk(mask, torch.uint8, "mask").data_ptr()
    d.h_seq, d.c_seq = h_seq.data_ptr(), c_seq.data_ptr()
    for name, t in (("dh_seq", dh_seq), ("dh_last", dh_last)):
        if t is not None and not _chk(t, name=name).is_contiguous():
            raise _lib.DcapError("lstm_seq_bwd: %s must be contiguous" % name)
    d.dh_seq = None if dh_seq is None else dh_seq.data_ptr()
    d.dh_last = None if dh_last is None else dh_last.data_ptr()
    d.dz, d.dU_rec, d.accumulate_dU = dz.data_ptr(), (None if dU is None else _chk(dU, name="dU").data_ptr()), int(accumulate_dU)
    d.rec_masks = _rec_masks(rec_masks, B, U)
    _lstm_step_info(info, B, U, 1, rec_masks is not None)
    _launch_ws(lib.dc_lstm_seq_workspace_bytes(B, T, U), z.device, lib.dc_lstm_seq_bwd_f32, C.byref(d))
    return dz, dU


def softmax_ce(logits, targets=None, probs=None, loss_rows=None, dlogits=None, grad_scale=1.0, row_weights=None,
               keras_sparse=False):
    lib = _lib.load()
    _chk(logits, name="logits")
    d = SoftmaxCeDesc()
    d.M, d.V, d.ld = logits.shape[0], logits.shape[1], logits.stride(0)
    d.logits = logits.data_ptr()
    d.targets = None if targets is None else _chk(targets, torch.int32, "targets").data_ptr()
    for name, t in (("probs", probs), ("dlogits", dlogits)):
        if t is not None and (_chk(t, name=name).stride(0) != logits.stride(0)):
            raise _lib.DcapError("softmax_ce: %s must share the logits' row stride" % name)
    d.probs = None if probs is None else probs.data_ptr()
    d.loss_rows = None if loss_rows is None else _chk(loss_rows, name="loss_rows").data_ptr()
    d.dlogits = None if dlogits is None else dlogits.data_ptr()
    d.grad_scale = float(grad_scale)
    d.row_weights = None if row_weights is None else _chk(row_weights, name="row_weights").data_ptr()
    d.keras_sparse = int(keras_sparse)
    check(lib.dc_softmax_ce_f32(C.byref(d), _stream()), "dc_softmax_ce_f32")


def _tag_rows(fn, name, t, dtype, M, C):
    """A [M,C] device matrix with any row stride -> its stride as the kernels take it (a single row has none)."""
    if _chk(t, dtype, name).dim() != 2 or tuple(t.shape) != (M, C):
        raise _lib.DcapError("%s: %s must be a %s [%d,%d] matrix, got %s" % (fn, name, dtype, M, C, tuple(t.shape)))
    return t.stride(0) if M > 1 else C


def tag_focal(logits, targets, alpha=0.25, gamma=2.0, grad_scale=1.0, loss_rows=None, dlogits=None):
    """Sigmoid + focal loss + gradient of the RoI tag head in one launch (dc_tag_focal_f32): logits float32 [M,C] and targets int32 [M,C]
    (multi-hot), any row strides.  loss_rows float32 [M] receives each live row's summed loss (a row is live when it has a target equal
    to 1; dead rows give exact zeros), dlogits float32 [M,C] (may be logits) grad_scale * d(sum of loss_rows)/d(logits).  Both are
    optional; with neither given, loss_rows is allocated.  Returns (loss_rows, dlogits).  alpha in [0, 1], gamma 0, 1 or 2."""
    lib = _lib.load()
    if _chk(logits, name="logits").dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise _lib.DcapError("tag_focal: logits must be a float32 [M,C] matrix with M, C >= 1, got %s" % (tuple(logits.shape),))
    M, Cn = logits.shape
    d = TagFocalDesc()
    d.M, d.C, d.z, d.ldz = M, Cn, logits.data_ptr(), _tag_rows("tag_focal", "logits", logits, torch.float32, M, Cn)
    d.t, d.ldt = targets.data_ptr(), _tag_rows("tag_focal", "targets", targets, torch.int32, M, Cn)
    if loss_rows is None and dlogits is None:
        loss_rows = torch.empty((M,), dtype=torch.float32, device=logits.device)
    if loss_rows is not None:
        if not _chk(loss_rows, name="loss_rows").is_contiguous() or tuple(loss_rows.shape) != (M,):
            raise _lib.DcapError("tag_focal: loss_rows must be a contiguous float32 [%d] vector" % M)
        d.loss_rows = loss_rows.data_ptr()
    if dlogits is not None:
        d.dz, d.lddz = dlogits.data_ptr(), _tag_rows("tag_focal", "dlogits", dlogits, torch.float32, M, Cn)
    d.alpha, d.gamma, d.grad_scale = float(alpha), float(gamma), float(grad_scale)
    check(lib.dc_tag_focal_f32(C.byref(d), _stream()), "dc_tag_focal_f32")
    return loss_rows, dlogits


def tag_scores(logits, min_confidence, probs=None, scores=None):
    """The RoI tag head at inference (dc_tag_scores_f32): probs float32 [M,C] = sigmoid(logits) and scores float32 [M] = the sum of log p
    over the classes with p > min_confidence (float64 accumulation, rounded once), float32(-3.4e38) for a row with none.  Both are
    allocated when not given.  Returns (probs, scores)."""
    lib = _lib.load()
    if _chk(logits, name="logits").dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise _lib.DcapError("tag_scores: logits must be a float32 [M,C] matrix with M, C >= 1, got %s" % (tuple(logits.shape),))
    M, Cn = logits.shape
    if probs is None:
        probs = torch.empty((M, Cn), dtype=torch.float32, device=logits.device)
    if scores is None:
        scores = torch.empty((M,), dtype=torch.float32, device=logits.device)
    if not _chk(scores, name="scores").is_contiguous() or tuple(scores.shape) != (M,):
        raise _lib.DcapError("tag_scores: scores must be a contiguous float32 [%d] vector" % M)
    check(lib.dc_tag_scores_f32(_ptr(logits), _tag_rows("tag_scores", "logits", logits, torch.float32, M, Cn), M, Cn, float(min_confidence),
                                _ptr(probs), _tag_rows("tag_scores", "probs", probs, torch.float32, M, Cn), _ptr(scores), _stream()),
          "dc_tag_scores_f32")
    return probs, scores


def _on_gpu(fn, **tensors):
    """The detection wrappers' last check before the library is loaded: every tensor lives on the device."""
    for name, t in tensors.items():
        if not t.is_cuda:
            raise _lib.DcapError("%s: %s must live on the GPU (no CPU path exists)" % (fn, name))


def class_select(logits, deltas, class_ids=None, scores=None, deltas_out=None):
    """The detection head's per-RoI selection (dc_class_select_f32): logits float32 [R,C] and box deltas float32 [R,4C] (or [R,C,4]
    contiguous), each with any row stride -> (class_ids int32 [R]: the lowest index of the maximal logit; scores float32 [R]: that
    class's softmax probability 1 / sum exp(z - z_max); deltas float32 [R,4]: the class's four words, copied).  C >= 2, any value.
    Outputs are allocated when not given.  The shapes are checked before the library is loaded."""
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 2:
        raise _lib.DcapError("class_select: logits must be a float32 [R,C] matrix with R >= 1 and C >= 2, got %s" % (tuple(logits.shape),))
    R, Cn = logits.shape
    if deltas.dim() == 3:
        if tuple(deltas.shape) != (R, Cn, 4) or not deltas.is_contiguous():
            raise _lib.DcapError("class_select: 3-D deltas must be a contiguous [%d,%d,4] tensor, got %s" % (R, Cn, tuple(deltas.shape)))
        deltas = deltas.view(R, 4 * Cn)
    if deltas.dim() != 2 or tuple(deltas.shape) != (R, 4 * Cn):
        raise _lib.DcapError("class_select: deltas must be a float32 [%d,%d] matrix, got %s" % (R, 4 * Cn, tuple(deltas.shape)))
    for name, t in (("logits", logits), ("deltas", deltas)):
        if t.dtype != torch.float32:
            raise _lib.DcapError("class_select: %s must be torch.float32, got %s" % (name, t.dtype))
        if t.stride(1) != 1 or (R > 1 and t.stride(0) < t.shape[1]):
            raise _lib.DcapError("class_select: %s must be contiguous along its rows with a row stride of at least %d, got strides %s"
                                 % (name, t.shape[1], tuple(t.stride())))
    dev = logits.device
    if class_ids is None:
        class_ids = torch.empty((R,), dtype=torch.int32, device=dev)
    if scores is None:
        scores = torch.empty((R,), dtype=torch.float32, device=dev)
    if deltas_out is None:
        deltas_out = torch.empty((R, 4), dtype=torch.float32, device=dev)
    for name, t, dtype, shape in (("class_ids", class_ids, torch.int32, (R,)), ("scores", scores, torch.float32, (R,)),
                                  ("deltas_out", deltas_out, torch.float32, (R, 4))):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.DcapError("class_select: %s must be a contiguous %s %s tensor, got %s %s" % (name, dtype, list(shape), t.dtype, tuple(t.shape)))
    _on_gpu("class_select", logits=logits, deltas=deltas, class_ids=class_ids, scores=scores, deltas_out=deltas_out)
    lib = _lib.load()
    check(lib.dc_class_select_f32(_ptr(logits), logits.stride(0) if R > 1 else Cn, _ptr(deltas), deltas.stride(0) if R > 1 else 4 * Cn, R, Cn,
                                  _ptr(class_ids), _ptr(scores), _ptr(deltas_out), _stream()), "dc_class_select_f32")
    return class_ids, scores, deltas_out


def refine_detections(rois, class_ids, scores, deltas, image_consts, std, min_confidence, threshold, max_instances, image_hw):
    """refine_detections from the line after the class selection + the box part of unmold_detections for B images x N RoIs in ONE launch
    (dc_refine_detections_f32), by the host path's operations (mask_rcnn_model.refine_detections / unmold_boxes): rois float32 [B,N,4]
    normalised; class_ids int32 [B,N], scores float32 [B,N] and deltas float32 [B,N,4] as ops.class_select leaves them; image_consts
    float64 [B,_lib.REFINE_CONSTS] (mask_rcnn_model.detection_constants: the window, the unmolding's shift and scale); std the four
    BBOX_STD_DEV; image_hw IMAGE_SHAPE's (h, w).  Returns seven device tensors of max_instances rows per image -- (count int32 [B],
    boxes int32 [B,M,4] in the molded image, rois int32 [B,M,4] in the original image, norm float32 [B,M,4] = boxes / (h,w,h,w),
    class_ids int32 [B,M], scores float32 [B,M], keep int32 [B,M]: the RoI's index) -- best first; rows behind the last survivor hold a
    zero box, class id -1, score 0 and keep -1.  Equal scores: the higher RoI index first.  N <= _lib.REFINE_DET_MAX_ROIS.  No
    workspace, no host synchronisation; B = 0 or N = 0 returns the empty result without a launch.  Everything is checked before the
    library is loaded."""
    if rois.dim() != 3 or rois.shape[2] != 4:
        raise _lib.DcapError("refine_detections: rois must be a float32 [B,N,4] tensor, got %s" % (tuple(rois.shape),))
    B, N = int(rois.shape[0]), int(rois.shape[1])
    for name, t, dtype, shape in (("rois", rois, torch.float32, (B, N, 4)), ("class_ids", class_ids, torch.int32, (B, N)),
                                  ("scores", scores, torch.float32, (B, N)), ("deltas", deltas, torch.float32, (B, N, 4)),
                                  ("image_consts", image_consts, torch.float64, (B, _lib.REFINE_CONSTS))):
        if t.dtype != dtype:
            raise _lib.DcapError("refine_detections: %s must be %s, got %s" % (name, dtype, t.dtype))
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.DcapError("refine_detections: %s must be a contiguous %s tensor, got shape %s strides %s"
                                 % (name, list(shape), tuple(t.shape), tuple(t.stride())))
    if N > _lib.REFINE_DET_MAX_ROIS:
        raise _lib.DcapError("refine_detections: N = %d exceeds the limit of %d RoIs per image" % (N, _lib.REFINE_DET_MAX_ROIS))
    if isinstance(max_instances, bool) or int(max_instances) != max_instances or max_instances < 1:
        raise _lib.DcapError("refine_detections: max_instances must be a positive integer, got %r" % (max_instances,))
    if len(std) != 4 or len(image_hw) != 2:
        raise _lib.DcapError("refine_detections: std must hold four values and image_hw two, got %r and %r" % (std, image_hw))
    _on_gpu("refine_detections", rois=rois, class_ids=class_ids, scores=scores, deltas=deltas, image_consts=image_consts)
    M, dev = int(max_instances), rois.device
    if B == 0 or N == 0:
        return (torch.zeros((B,), dtype=torch.int32, device=dev), torch.zeros((B, M, 4), dtype=torch.int32, device=dev),
                torch.zeros((B, M, 4), dtype=torch.int32, device=dev), torch.zeros((B, M, 4), dtype=torch.float32, device=dev),
                torch.full((B, M), -1, dtype=torch.int32, device=dev), torch.zeros((B, M), dtype=torch.float32, device=dev),
                torch.full((B, M), -1, dtype=torch.int32, device=dev))
    lib = _lib.load()
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    boxes, final = (torch.empty((B, M, 4), dtype=torch.int32, device=dev) for _ in range(2))
    norm = torch.empty((B, M, 4), dtype=torch.float32, device=dev)
    ids_out, keep = (torch.empty((B, M), dtype=torch.int32, device=dev) for _ in range(2))
    scores_out = torch.empty((B, M), dtype=torch.float32, device=dev)
    d = RefineDetDesc()
    d.B, d.N, d.max_instances = B, N, M
    d.rois, d.class_ids, d.scores, d.deltas, d.image_consts = (rois.data_ptr(), class_ids.data_ptr(), scores.data_ptr(), deltas.data_ptr(),
                                                               image_consts.data_ptr())
    for i in range(4):
        d.std_dev[i] = float(std[i])
    d.image_h, d.image_w, d.min_confidence, d.threshold = float(image_hw[0]), float(image_hw[1]), float(min_confidence), float(threshold)
    d.count_out, d.boxes_out, d.rois_out, d.norm_out, d.class_ids_out, d.scores_out, d.keep_out = (
        count.data_ptr(), boxes.data_ptr(), final.data_ptr(), norm.data_ptr(), ids_out.data_ptr(), scores_out.data_ptr(), keep.data_ptr())
    check(lib.dc_refine_detections_f32(C.byref(d), _stream()), "dc_refine_detections_f32")
    return count, boxes, final, norm, ids_out, scores_out, keep


def mask_head_tail(x, wd, bd, wm_t, bm, class_ids, out=None):
    """mrcnn_mask_deconv + ReLU + mrcnn_mask + sigmoid for each RoI's own class (dc_mask_head_tail_f32).  x float32 [N,P,P,Cin]
    contiguous (P <= 16); wd the Keras Conv2DTranspose kernel [2,2,Cmid,Cin]; bd [Cmid]; wm_t [C,Cmid], the mrcnn_mask kernel
    transposed (packing.pack_mask_tail); bm [C]; class_ids int32 [N] on the device.  Cin a multiple of 32 up to 256, Cmid a multiple
    of 32.  Returns out float32 [N,2P,2P]; a class id outside [0,C) gives that RoI zeros.  No alignment rule beyond float32's own (bases off
    a 16-byte boundary are read 4 bytes at a time).  Shapes, dtypes and strides are checked before the library is loaded."""
    if x.dim() != 4 or x.shape[0] < 1 or x.shape[1] != x.shape[2] or not 1 <= x.shape[1] <= 16:
        raise _lib.DcapError("mask_head_tail: x must be [N,P,P,Cin] with N >= 1 and P in 1..16, got %s" % (tuple(x.shape),))
    N, P, _, Cin = x.shape
    if Cin % 32 or not 32 <= Cin <= 256:
        raise _lib.DcapError("mask_head_tail: Cin must be a multiple of 32 in 32..256, got %d" % Cin)
    if wd.dim() != 4 or tuple(wd.shape[:2]) != (2, 2) or wd.shape[3] != Cin or wd.shape[2] % 32 or wd.shape[2] < 32:
        raise _lib.DcapError("mask_head_tail: wd must be the Keras deconvolution kernel [2,2,Cmid,%d] with Cmid a multiple of 32, got %s"
                             % (Cin, tuple(wd.shape)))
    Cmid = wd.shape[2]
    if wm_t.dim() != 2 or wm_t.shape[1] != Cmid or wm_t.shape[0] < 1:
        raise _lib.DcapError("mask_head_tail: wm_t must be [C,%d] (the mrcnn_mask kernel transposed), got %s" % (Cmid, tuple(wm_t.shape)))
    Cn = wm_t.shape[0]
    if out is None:
        out = torch.empty((N, 2 * P, 2 * P), dtype=torch.float32, device=x.device)
    for name, t, dtype, shape in (("x", x, torch.float32, (N, P, P, Cin)), ("wd", wd, torch.float32, (2, 2, Cmid, Cin)),
                                  ("bd", bd, torch.float32, (Cmid,)), ("wm_t", wm_t, torch.float32, (Cn, Cmid)),
                                  ("bm", bm, torch.float32, (Cn,)), ("class_ids", class_ids, torch.int32, (N,)),
                                  ("out", out, torch.float32, (N, 2 * P, 2 * P))):
        if t.dtype != dtype:
            raise _lib.DcapError("mask_head_tail: %s must be %s, got %s" % (name, dtype, t.dtype))
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.DcapError("mask_head_tail: %s must be a contiguous %s tensor, got shape %s strides %s"
                                 % (name, list(shape), tuple(t.shape), tuple(t.stride())))
    _on_gpu("mask_head_tail", x=x, wd=wd, bd=bd, wm_t=wm_t, bm=bm, class_ids=class_ids, out=out)
    lib = _lib.load()
    d = MaskHeadTailDesc()
    d.N, d.P, d.Cin, d.Cmid, d.C = N, P, Cin, Cmid, Cn
    d.x, d.wd, d.bd, d.wm_t, d.bm, d.class_ids, d.out = (x.data_ptr(), wd.data_ptr(), bd.data_ptr(), wm_t.data_ptr(), bm.data_ptr(),
                                                         class_ids.data_ptr(), out.data_ptr())
    check(lib.dc_mask_head_tail_f32(C.byref(d), _stream()), "dc_mask_head_tail_f32")
    return out


def mask_paste(masks, boxes, H, W, out=None):
    """utils.unmold_mask for the M detections of one image (dc_mask_paste_u8): masks float32 [M,h,w] (h, w <= 64), boxes int32 [M,4]
    (y1, x1, y2, x2) in the original H x W image, both on the device -> uint8 [M,H,W]: scipy's bytescale on each mask's own range,
    PIL's 8-bit bilinear resize to the box, 1 where the byte is >= 128, 0 elsewhere -- every byte written.  An empty box or one that
    leaves the image gives zeros.  M = 0 returns an empty tensor.  Shapes and dtypes are checked before the library is loaded."""
    H, W = int(H), int(W)
    if masks.dim() != 3 or not (1 <= masks.shape[1] <= 64 and 1 <= masks.shape[2] <= 64):
        raise _lib.DcapError("mask_paste: masks must be [M,h,w] with h, w in 1..64, got %s" % (tuple(masks.shape),))
    M, h, w = masks.shape
    if H < 1 or W < 1 or max(H, W) > 1 << 24 or H * W >= 1 << 31 or M > 65535:
        raise _lib.DcapError("mask_paste: an image of at least 1 x 1 and below 2^31 pixels and at most 65535 detections, got %d x %d, M %d" % (H, W, M))
    if out is None:
        out = torch.empty((M, H, W), dtype=torch.uint8, device=masks.device)
    for name, t, dtype, shape in (("masks", masks, torch.float32, (M, h, w)), ("boxes", boxes, torch.int32, (M, 4)),
                                  ("out", out, torch.uint8, (M, H, W))):
        if t.dtype != dtype:
            raise _lib.DcapError("mask_paste: %s must be %s, got %s" % (name, dtype, t.dtype))
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.DcapError("mask_paste: %s must be a contiguous %s tensor, got shape %s strides %s"
                                 % (name, list(shape), tuple(t.shape), tuple(t.stride())))
    _on_gpu("mask_paste", masks=masks, boxes=boxes, out=out)
    if M == 0:
        return out
    lib = _lib.load()
    d = MaskPasteDesc()
    d.M, d.h, d.w, d.H, d.W = M, h, w, H, W
    d.masks, d.boxes, d.out = masks.data_ptr(), boxes.data_ptr(), out.data_ptr()
    _launch_ws(lib.dc_mask_paste_u8_workspace_bytes(C.byref(d)), masks.device, lib.dc_mask_paste_u8, C.byref(d))
    return out


def mask_rle_capacity(M, H, W):
    """ops.mask_rle's default capacity in words for M detections in an H x W image: one word per detection and image column, at least
    4096 (DESIGN.md section 6.1m has the run counts it was sized from).  The whole capacity is what rles() copies, and only the cost
    of a second launch depends on it, never a result."""
    return max(4096, int(M) * int(W))


class MaskRle(object):
    """What ops.mask_rle returns: `pack`, ONE int32 device tensor [M + 1 + capacity] -- `offsets` [M + 1] and `counts` [capacity]
    (uint32 bits) are views of it -- so that a caller holding several can bring them down in one copy (torch.cat of the packs).
    rles() makes the host list; nothing reads the device before it."""

    def __init__(self, masks, boxes, H, W, capacity):
        self.masks, self.boxes, self.size, self.capacity = masks, boxes, (int(H), int(W)), int(capacity)
        self.M = int(masks.shape[0])
        self.launches = 0
        self._launch()

    def _launch(self):
        M, (H, W) = self.M, self.size
        self.pack = torch.empty((M + 1 + self.capacity,), dtype=torch.int32, device=self.masks.device)
        self.offsets, self.counts = self.pack[:M + 1], self.pack[M + 1:]
        lib = _lib.load()
        d = MaskRleDesc()
        d.M, d.h, d.w, d.H, d.W, d.capacity = M, int(self.masks.shape[1]), int(self.masks.shape[2]), H, W, self.capacity
        d.masks, d.boxes, d.offsets, d.counts = self.masks.data_ptr(), self.boxes.data_ptr(), self.offsets.data_ptr(), self.counts.data_ptr()
        ws, wsb = WORKSPACE.get(lib.dc_mask_rle_workspace_bytes(C.byref(d)), self.masks.device)
        d.workspace, d.workspace_bytes = None if ws is None else ws.data_ptr(), wsb
        check(lib.dc_mask_rle_u32(C.byref(d), _stream()), "dc_mask_rle_u32")
        self.launches += 1

    def relaunch(self, capacity):
        """Run the entry again with `capacity` words (a caller that read offsets[M] itself, as MaskRCNN.evaluate does from ops.rle_iou's
        status): pack, offsets and counts are new tensors afterwards."""
        self.capacity = int(capacity)
        self._launch()

    def rles(self, host=None):
        """The M encodings as a list of {"size": [H, W], "counts": uint32 ndarray}.  host: this object's pack as an int32 host array,
        where the caller has copied it already; otherwise the pack is copied here (the one device-to-host copy).  When the
        encodings need more words than `capacity`, the entry runs a second time with exactly the capacity offsets[M] asks for and
        that result is copied: the list is always complete."""
        M = self.M
        if host is None:
            host = self.pack.cpu().numpy()
        need = int(host[M])
        if need > self.capacity:
            self.capacity = need
            self._launch()
            host = self.pack.cpu().numpy()
            if int(host[M]) != need:
                raise _lib.DcapError("mask_rle: the second run needs %d words where the first asked for %d" % (int(host[M]), need))
        offsets, counts = host[:M + 1], host[M + 1:].view(np.uint32)
        return [{"size": list(self.size), "counts": counts[offsets[m]:offsets[m + 1]].copy()} for m in range(M)]


def mask_rle(masks, boxes, H, W, capacity=None):
    """The planes ops.mask_paste would write, as COCO run-length encodings built on the device without the planes (dc_mask_rle_u32;
    the format: mask_rle.py).  masks float32 [M,h,w] (h, w <= 64), boxes int32 [M,4] (y1, x1, y2, x2) in the original H x W image,
    both on the device.  Returns a MaskRle: .offsets int32 [M+1] and .counts int32 [capacity] (uint32 bits) on the device, views of
    its .pack, and .rles(), which copies the pack once and returns the list of {"size", "counts"} -- after a second launch with
    capacity = offsets[M] where the first capacity was too small, so no result depends on `capacity` (default:
    mask_rle_capacity(M, H, W)).  An empty box or one that leaves the image encodes as [H * W].  No host synchronisation before
    rles().  Shapes and dtypes are checked before the library is loaded."""
    H, W = int(H), int(W)
    if masks.dim() != 3 or not (1 <= masks.shape[1] <= 64 and 1 <= masks.shape[2] <= 64):
        raise _lib.DcapError("mask_rle: masks must be [M,h,w] with h, w in 1..64, got %s" % (tuple(masks.shape),))
    M, h, w = masks.shape
    if H < 1 or W < 1 or max(H, W) > 1 << 24 or H * W >= 1 << 31 or M > 65535 or M * (H * W + 1) >= 1 << 31:
        raise _lib.DcapError("mask_rle: an image of at least 1 x 1 and below 2^31 pixels, at most 65535 detections and M * (H * W + 1) below 2^31, "
                             "got %d x %d, M %d" % (H, W, M))
    if capacity is None:
        capacity = mask_rle_capacity(M, H, W)
    if isinstance(capacity, bool) or int(capacity) != capacity or not 0 <= capacity < (1 << 31) - M - 1:
        raise _lib.DcapError("mask_rle: capacity must be an integer in 0..2^31 - M - 2, got %r" % (capacity,))
    for name, t, dtype, shape in (("masks", masks, torch.float32, (M, h, w)), ("boxes", boxes, torch.int32, (M, 4))):
        if t.dtype != dtype:
            raise _lib.DcapError("mask_rle: %s must be %s, got %s" % (name, dtype, t.dtype))
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.DcapError("mask_rle: %s must be a contiguous %s tensor, got shape %s strides %s"
                                 % (name, list(shape), tuple(t.shape), tuple(t.stride())))
    _on_gpu("mask_rle", masks=masks, boxes=boxes)
    return MaskRle(masks, boxes, H, W, capacity)


EVAL_MAX = 1024      # include/dcap.h, dc_rle_iou_f64 / dc_box_iou_f64 / dc_detection_ap_f64: masks, boxes or predictions per set


def _eval_tensors(fn, specs):
    """(name, tensor or None, dtype, shape) rows: a given tensor is a contiguous device tensor of that dtype and shape."""
    given = {}
    for name, t, dtype, shape in specs:
        if t is None:
            continue
        if t.dtype != dtype:
            raise _lib.DcapError("%s: %s must be %s, got %s" % (fn, name, dtype, t.dtype))
        if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise _lib.DcapError("%s: %s must be a contiguous %s tensor, got shape %s strides %s" % (fn, name, list(shape), tuple(t.shape), tuple(t.stride())))
        given[name] = t
    _on_gpu(fn, **given)


def _eval_rows(fn, name, t, rows, cols):
    """An IoU matrix given as `out`: float64 [..., rows, cols] on the device, unit stride along the columns, dense above the rows.
    Returns the row stride."""
    if t.dtype != torch.float64 or tuple(t.shape[-2:]) != (rows, cols):
        raise _lib.DcapError("%s: %s must be a float64 [..., %d, %d] tensor, got %s %s" % (fn, name, rows, cols, t.dtype, tuple(t.shape)))
    ld = t.stride(-2) if rows > 1 else max(cols, 1)
    if rows * cols and ((cols > 1 and t.stride(-1) != 1) or ld < cols or (t.dim() == 3 and t.shape[0] > 1 and t.stride(0) != rows * ld)):
        raise _lib.DcapError("%s: %s needs unit stride along its columns and images one behind the other, got strides %s" % (fn, name, tuple(t.stride())))
    _on_gpu(fn, **{name: t})
    return int(ld)


def rle_iou(offsets_d, counts_d, offsets_g, counts_g, H, W, n_det=None, iscrowd=None, out=None, status=None):
    """pycocotools' rleIou on the device (dc_rle_iou_f64; the host statement: mask_rle.iou): two packed sets of run-length encodings as
    ops.mask_rle leaves them -- offsets int32 [D+1] / [G+1] and counts int32 (uint32 bits) [capacity] -- of masks of one size H x W.
    n_det: int32 [1] on the device, rows at or beyond it are 0; iscrowd: uint8 [G] on the device.  Returns (iou float64 [D,G], inter int32
    [D,G], area int32 [D+G], status int32 [4]) on the device: `out` (a float64 [D,G] view with any row stride) and `status` are used
    when given.  status[0] / status[1] non-zero: that set needs so many words, everything is NaN / -1 and the caller reruns ops.mask_rle;
    status[2]: masks whose counts do not sum to H * W (their row or column is NaN).  With D = 0 or G = 0 only status is computed (area
    is -1).  No host synchronisation.  Shapes and dtypes are checked before the library is loaded."""
    fn = "rle_iou"
    H, W = int(H), int(W)
    if offsets_d.dim() != 1 or offsets_g.dim() != 1 or offsets_d.numel() < 1 or offsets_g.numel() < 1 or counts_d.dim() != 1 or counts_g.dim() != 1:
        raise _lib.DcapError("rle_iou: offsets must be int32 [D+1] and [G+1] and counts one-dimensional, got %s, %s, %s, %s"
                             % (tuple(offsets_d.shape), tuple(offsets_g.shape), tuple(counts_d.shape), tuple(counts_g.shape)))
    D, G = offsets_d.numel() - 1, offsets_g.numel() - 1
    if D > EVAL_MAX or G > EVAL_MAX or H < 1 or W < 1 or H * W >= 1 << 31 or max(counts_d.numel(), counts_g.numel()) >= 1 << 31:
        raise _lib.DcapError("rle_iou: at most %d masks a set and an image of at least 1 x 1 and below 2^31 pixels, got D %d, G %d, %d x %d"
                             % (EVAL_MAX, D, G, H, W))
    _eval_tensors(fn, (("offsets_d", offsets_d, torch.int32, (D + 1,)), ("counts_d", counts_d, torch.int32, (counts_d.numel(),)),
                       ("offsets_g", offsets_g, torch.int32, (G + 1,)), ("counts_g", counts_g, torch.int32, (counts_g.numel(),)),
                       ("n_det", n_det, torch.int32, (1,)), ("iscrowd", iscrowd, torch.uint8, (G,)), ("status", status, torch.int32, (4,))))
    dev = offsets_d.device
    if out is None:
        out = torch.empty((D, G), dtype=torch.float64, device=dev)
    ld = _eval_rows(fn, "out", out, D, G)
    if out.dim() != 2:
        raise _lib.DcapError("rle_iou: out must be a [D,G] tensor, got shape %s" % (tuple(out.shape),))
    if status is None:
        status = torch.empty((4,), dtype=torch.int32, device=dev)
    empty = D == 0 or G == 0
    inter = torch.empty((D, ld), dtype=torch.int32, device=dev)[:, :G]            # (`out` may be a view with its own row stride)
    area = torch.full((D + G,), -1, dtype=torch.int32, device=dev) if empty else torch.empty((D + G,), dtype=torch.int32, device=dev)
    lib = _lib.load()
    d = RleIouDesc()
    d.D, d.G, d.H, d.W, d.capacity_d, d.capacity_g, d.ld = D, G, H, W, counts_d.numel(), counts_g.numel(), ld
    d.offsets_d, d.offsets_g, d.status = offsets_d.data_ptr(), offsets_g.data_ptr(), status.data_ptr()
    d.counts_d, d.counts_g = (counts_d.data_ptr() if counts_d.numel() else None), (counts_g.data_ptr() if counts_g.numel() else None)
    d.n_det, d.iscrowd = (None if n_det is None else n_det.data_ptr()), (None if iscrowd is None or G == 0 else iscrowd.data_ptr())
    if not empty:
        d.iou, d.inter, d.area = out.data_ptr(), inter.data_ptr(), area.data_ptr()
    ws, wsb = WORKSPACE.get(lib.dc_rle_iou_workspace_bytes(C.byref(d)), dev)
    d.workspace, d.workspace_bytes = None if ws is None else ws.data_ptr(), wsb
    check(lib.dc_rle_iou_f64(C.byref(d), _stream()), "dc_rle_iou_f64")
    return out, inter, area, status


def box_iou(boxes, gt_boxes, out=None):
    """utils.compute_overlaps for B images in one launch (dc_box_iou_f64): boxes int32 [B,Dmax,4] and gt_boxes int32 [B,Gmax,4] as
    (y1, x1, y2, x2) on the device -> float64 [B,Dmax,Gmax], every entry written (`out`: a view of that shape with any row stride).
    NumPy's int32 formula in int64 with one float64 division; a zero union gives NaN as NumPy's 0 / 0 does.  No host synchronisation;
    an empty result launches nothing."""
    fn = "box_iou"
    if boxes.dim() != 3 or gt_boxes.dim() != 3 or boxes.shape[2] != 4 or gt_boxes.shape[2] != 4 or boxes.shape[0] != gt_boxes.shape[0]:
        raise _lib.DcapError("box_iou: boxes must be [B,Dmax,4] and gt_boxes [B,Gmax,4], got %s and %s" % (tuple(boxes.shape), tuple(gt_boxes.shape)))
    B, Dmax, Gmax = int(boxes.shape[0]), int(boxes.shape[1]), int(gt_boxes.shape[1])
    if B > 65535 or Dmax > EVAL_MAX or Gmax > EVAL_MAX:
        raise _lib.DcapError("box_iou: at most 65535 images and %d boxes a set, got B %d, Dmax %d, Gmax %d" % (EVAL_MAX, B, Dmax, Gmax))
    _eval_tensors(fn, (("boxes", boxes, torch.int32, (B, Dmax, 4)), ("gt_boxes", gt_boxes, torch.int32, (B, Gmax, 4))))
    if out is None:
        out = torch.empty((B, Dmax, Gmax), dtype=torch.float64, device=boxes.device)
    ld = _eval_rows(fn, "out", out, Dmax, Gmax)
    if out.dim() != 3 or out.shape[0] != B:
        raise _lib.DcapError("box_iou: out must be a [%d,%d,%d] tensor, got shape %s" % (B, Dmax, Gmax, tuple(out.shape)))
    if B * Dmax * Gmax == 0:
        return out
    lib = _lib.load()
    check(lib.dc_box_iou_f64(_ptr(boxes), _ptr(gt_boxes), B, Dmax, Gmax, ld, _ptr(out), _stream()), "dc_box_iou_f64")
    return out


def detection_ap(overlaps, n_det, n_gt, pred_class, pred_score, gt_class, thresholds, ap=None, pred_match=None, gt_match=None, order=None):
    """utils.compute_ap's matching and average precision on given IoU matrices, for B images and T thresholds in ONE launch
    (dc_detection_ap_f64; the host statement and the rules: detection_eval.ap_from_overlaps).  overlaps float64 [B,Dmax,Gmax] (any row
    stride); n_det, n_gt int32 [B] ON THE DEVICE: the block of an image that counts; pred_class int32 [B,Dmax], pred_score float32
    [B,Dmax], gt_class int32 [B,Gmax]; thresholds float64 [T] on the device, T in 1..16.  Returns (ap float64 [B,T] -- NaN for an image
    without ground truth --, pred_match int32 [B,T,Dmax], gt_match int32 [B,T,Gmax], order int32 [B,Dmax]), -1 behind the counts; the
    four are allocated when not given.  No workspace, no host synchronisation; B = 0 launches nothing."""
    fn = "detection_ap"
    if overlaps.dim() != 3 or thresholds.dim() != 1:
        raise _lib.DcapError("detection_ap: overlaps must be [B,Dmax,Gmax] and thresholds [T], got %s and %s" % (tuple(overlaps.shape), tuple(thresholds.shape)))
    (B, Dmax, Gmax), T = (int(v) for v in overlaps.shape), int(thresholds.numel())
    if B > 65535 or Dmax > EVAL_MAX or Gmax > EVAL_MAX or not 1 <= T <= 16:
        raise _lib.DcapError("detection_ap: at most 65535 images, %d predictions and ground truths an image and 1..16 thresholds, got B %d, Dmax %d, "
                             "Gmax %d, T %d" % (EVAL_MAX, B, Dmax, Gmax, T))
    ld = _eval_rows(fn, "overlaps", overlaps, Dmax, Gmax)
    dev = overlaps.device
    made = {}
    for name, t, dtype, shape in (("ap", ap, torch.float64, (B, T)), ("pred_match", pred_match, torch.int32, (B, T, Dmax)),
                                  ("gt_match", gt_match, torch.int32, (B, T, Gmax)), ("order", order, torch.int32, (B, Dmax))):
        made[name] = torch.empty(shape, dtype=dtype, device=dev) if t is None else t
    ap, pred_match, gt_match, order = made["ap"], made["pred_match"], made["gt_match"], made["order"]
    _eval_tensors(fn, (("n_det", n_det, torch.int32, (B,)), ("n_gt", n_gt, torch.int32, (B,)), ("pred_class", pred_class, torch.int32, (B, Dmax)),
                       ("pred_score", pred_score, torch.float32, (B, Dmax)), ("gt_class", gt_class, torch.int32, (B, Gmax)),
                       ("thresholds", thresholds, torch.float64, (T,)), ("ap", ap, torch.float64, (B, T)),
                       ("pred_match", pred_match, torch.int32, (B, T, Dmax)), ("gt_match", gt_match, torch.int32, (B, T, Gmax)),
                       ("order", order, torch.int32, (B, Dmax))))
    for name, t in (("n_det", n_det), ("n_gt", n_gt), ("pred_class", pred_class), ("pred_score", pred_score), ("gt_class", gt_class)):
        if t is None:
            raise _lib.DcapError("detection_ap: %s is missing" % name)
    if B == 0:
        return ap, pred_match, gt_match, order
    lib = _lib.load()
    d = DetectionApDesc()
    d.B, d.Dmax, d.Gmax, d.ld, d.T = B, Dmax, Gmax, ld, T
    d.overlaps, d.n_det, d.n_gt, d.thresholds, d.ap = overlaps.data_ptr(), n_det.data_ptr(), n_gt.data_ptr(), thresholds.data_ptr(), ap.data_ptr()
    d.pred_class, d.pred_score, d.gt_class = pred_class.data_ptr(), pred_score.data_ptr(), gt_class.data_ptr()
    d.pred_match, d.gt_match, d.order = pred_match.data_ptr(), gt_match.data_ptr(), order.data_ptr()
    check(lib.dc_detection_ap_f64(C.byref(d), _stream()), "dc_detection_ap_f64")
    return ap, pred_match, gt_match, order


def _caption_rows(fn, name, t, rows=None, dim=2):
    """A caption-metric operand: int32 on the GPU, `dim` dimensions, unit stride along the last.  Returns the row stride."""
    if _chk(t, torch.int32, name).dim() != dim or (rows is not None and t.shape[0] != rows):
        raise _lib.DcapError("%s: %s must be an int32 %s, got shape %s" % (fn, name, "[%s]" % ", ".join(
            ["%d" % rows if rows is not None else "rows"] + ["width"] * (dim - 1)), tuple(t.shape)))
    if dim == 1:
        return 1
    if t.shape[1] < 1 or (t.shape[0] > 1 and t.stride(0) < 1):
        raise _lib.DcapError("%s: %s needs a width and a row stride of at least 1" % (fn, name))
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def caption_metrics(cand, cand_len, refs, ref_len, ref_start, lcs=False):
    """BLEU-1..4 and ROUGE-L of N caption records in one launch (dc_caption_metrics_f64): cand int32 [N,Tc] + cand_len [N], refs int32
    [M,Tr] + ref_len [M], ref_start int32 [N+1] (CSR: the references of record i are rows ref_start[i]..ref_start[i+1]-1).  Returns
    (stats int32 [N,12], bleu float64 [4,N], rouge float64 [N]).  lcs=False: ROUGE on what the reference fork's my_lcs returns;
    lcs=True: on the true longest common subsequence.  A sentence holds at most CAPTION_MAX_TOKENS tokens (the kernel reads a longer
    length as that many: caption_metrics.score refuses it by name before it gets here).  N = 0 gives empty results without a launch."""
    lib = _lib.load()
    fn = "caption_metrics"
    N, M = cand.shape[0], refs.shape[0]
    d = _lib.CaptionMetricsDesc()
    d.N, d.M, d.Tc, d.Tr, d.lcs = N, M, cand.shape[1], refs.shape[1], int(bool(lcs))
    d.ld_cand, d.ld_refs = _caption_rows(fn, "cand", cand), _caption_rows(fn, "refs", refs)
    for name, t, rows in (("cand_len", cand_len, N), ("ref_len", ref_len, M), ("ref_start", ref_start, N + 1)):
        _caption_rows(fn, name, t, rows, dim=1)
    stats = torch.empty((N, 12), dtype=torch.int32, device=cand.device)
    bleu = torch.empty((4, N), dtype=torch.float64, device=cand.device)
    rouge = torch.empty((N,), dtype=torch.float64, device=cand.device)
    if N == 0:
        return stats, bleu, rouge
    d.cand, d.cand_len, d.refs, d.ref_len, d.ref_start = cand.data_ptr(), cand_len.data_ptr(), refs.data_ptr(), ref_len.data_ptr(), ref_start.data_ptr()
    d.stats, d.bleu, d.rouge = stats.data_ptr(), bleu.data_ptr(), rouge.data_ptr()
    check(lib.dc_caption_metrics_f64(C.byref(d), _stream()), "dc_caption_metrics_f64")
    return stats, bleu, rouge


def caption_cider(grams, sent_len, ref_start, df, df_off, group_n):
    """CIDEr of N records in one launch (dc_caption_cider_f64) from dense n-gram ids: grams int32 [4,S,T] (sentences 0..N-1 the
    candidates, then the references; -1 where no n-gram starts), sent_len int32 [S], ref_start int32 [N+1], df int32 (the orders'
    document-frequency tables one after the other, order k's at df_off[k-1]), group_n int32 [N] (the size of the record's group).
    caption_metrics.cider_gram_tables builds these.  Returns cider float64 [N]."""
    lib = _lib.load()
    fn = "caption_cider"
    N = group_n.shape[0]
    if _chk(grams, torch.int32, "grams").dim() != 3 or grams.shape[0] != 4 or not grams.is_contiguous() or grams.shape[2] < 1:
        raise _lib.DcapError("%s: grams must be a contiguous int32 [4,S,T] tensor, got shape %s" % (fn, tuple(grams.shape)))
    S, T = grams.shape[1], grams.shape[2]
    for name, t, rows in (("sent_len", sent_len, S), ("ref_start", ref_start, N + 1), ("df", df, None), ("group_n", group_n, N)):
        _caption_rows(fn, name, t, rows, dim=1)
    df_off = [int(o) for o in df_off]
    if len(df_off) != 4 or df_off[0] != 0 or sorted(df_off) != df_off or df_off[3] > df.shape[0]:
        raise _lib.DcapError("%s: df_off must be four offsets into df that start at 0 and do not decrease, got %s" % (fn, df_off))
    cider = torch.empty((N,), dtype=torch.float64, device=grams.device)
    if N == 0:
        return cider
    if S <= N:
        raise _lib.DcapError("%s: grams holds %d sentences for %d records: every record needs a reference" % (fn, S, N))
    d = _lib.CaptionCiderDesc()
    d.N, d.S, d.T, d.df_len = N, S, T, df.shape[0]
    for k in range(4):
        d.df_off[k] = df_off[k]
    d.grams, d.sent_len, d.ref_start, d.df, d.group_n, d.cider = (grams.data_ptr(), sent_len.data_ptr(), ref_start.data_ptr(), df.data_ptr(),
                                                                  group_n.data_ptr(), cider.data_ptr())
    check(lib.dc_caption_cider_f64(C.byref(d), _stream()), "dc_caption_cider_f64")
    return cider


def vocab_ce_supported(X, W):
    """Shapes the fused vocabulary softmax / cross-entropy takes (otherwise: gemm + softmax_ce)."""
    K, V = W.shape
    if X.dtype == BF16:
        return W.dtype == BF16 and K % 8 == 0 and V % 8 == 0 and X.stride(0) % 8 == 0 and W.stride(0) % 8 == 0
    return K % 32 == 0 and V % 4 == 0 and V >= 4 and X.stride(0) % 4 == 0 and W.stride(0) % 4 == 0


def vocab_ce(X, W, bias, targets, loss_rows=None, dlogits=None, dbias=None, grad_scale=1.0, row_weights=None, keras_sparse=False,
             materialize_bf16=None):
    """Fused Dense(V) + softmax + Keras cross-entropy (dc_vocab_ce): X [M,K] and W [K,V] both float32 or both bf16; the
    [M,V] logits are never materialised in fp32.  dlogits: float32 or bf16 [M, >=V] receives d(loss)/d(logits); dbias [V] its
    column sums.  materialize_bf16 (default: DCAP_VOCAB_MATERIALIZE, on): bf16 operands with a bf16 dlogits buffer -- the logits are
    rounded to bf16 and parked in that buffer by the first GEMM pass, the gradient is an in-place elementwise pass (dcap.h)."""
    lib = _lib.load()
    bf = X.dtype == BF16
    _chk(X, BF16 if bf else torch.float32, "X"), _chk(W, BF16 if bf else torch.float32, "W")
    M, K = X.shape
    if W.shape[0] != K:
        raise _lib.DcapError("vocab_ce: inner dimensions differ (%d vs %d)" % (K, W.shape[0]))
    d = VocabCeDesc()
    d.M, d.V, d.K, d.bf16 = M, W.shape[1], K, int(bf)
    d.X, d.ldx, d.W, d.ldw = X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0)
    d.bias = None if bias is None else _chk(bias, name="bias").data_ptr()
    d.targets = _chk(targets, torch.int32, "targets").data_ptr()
    d.row_weights = None if row_weights is None else _chk(row_weights, name="row_weights").data_ptr()
    d.grad_scale, d.keras_sparse = float(grad_scale), int(keras_sparse)
    d.loss_rows = None if loss_rows is None else _chk(loss_rows, name="loss_rows").data_ptr()
    if dlogits is not None:
        if dlogits.dtype not in (torch.float32, BF16) or not dlogits.is_cuda or dlogits.stride(1) != 1 or dlogits.shape[0] != M:
            raise _lib.DcapError("vocab_ce: dlogits must be a float32 or bf16 device matrix with M rows")
        d.dlogits, d.lddl, d.dl_bf16 = dlogits.data_ptr(), dlogits.stride(0), int(dlogits.dtype == BF16)
    d.dbias = None if dbias is None else _chk(dbias, name="dbias").data_ptr()
    if materialize_bf16 is None:
        materialize_bf16 = os.environ.get("DCAP_VOCAB_MATERIALIZE", "1") != "0"
    d.materialize_bf16 = int(bool(materialize_bf16) and bf and dlogits is not None and dlogits.dtype == BF16)
    _launch_ws(lib.dc_vocab_ce_workspace_bytes(C.byref(d)), X.device, lib.dc_vocab_ce, C.byref(d))


def _row_out(t, M, dtype, name):
    """A strided length-M device vector (e.g. column j of a row-major [B,T] matrix) -> (pointer, element stride)."""
    if t is None:
        return None, 1
    if not t.is_cuda or t.dtype != dtype or t.dim() != 1 or t.shape[0] != M or (M > 1 and t.stride(0) < 1):
        raise _lib.DcapError("vocab_top1: %s must be a %s device vector of %d elements" % (name, dtype, M))
    return C.c_void_p(t.data_ptr()), max(1, t.stride(0))


def _vocab_operands(X, W, bias):
    """X [M,K], W [K,V], bias [V] as the fused vocabulary kernels read them: W rows readable in whole 16-byte chunks (4 float32 / 8 bf16
    columns) up to V rounded up to that, X rows and bias 16-byte aligned (a padded / aligned copy otherwise)."""
    M, K = X.shape
    V = W.shape[1]
    q = 8 if W.dtype == BF16 else 4
    Vp = (V + q - 1) // q * q
    esz = W.element_size()
    w_ok = (W.stride(0) % q == 0 and W.stride(0) >= Vp and W.data_ptr() % 16 == 0 and
            (W.storage_offset() + (K - 1) * W.stride(0) + Vp) * esz <= W.untyped_storage().nbytes())
    if not w_ok:                                       # (the kernel reads whole 16-byte chunks of W's rows)
        Wp = torch.zeros((K, Vp), dtype=W.dtype, device=W.device)
        Wp[:, :V].copy_(W)
        W = Wp
    if X.stride(0) % q or X.data_ptr() % 16:
        X = torch.empty((M, K), dtype=X.dtype, device=X.device).copy_(X)
    if bias is not None and (bias.data_ptr() % 16 or not bias.is_contiguous()):
        bias = torch.empty((V,), dtype=torch.float32, device=bias.device).copy_(bias)
    return X, W, bias


def _vocab_args(fn, X, W, bias, tile=None):
    """The argument checks of vocab_top1 and vocab_topk (fn: the caller, for the messages) -> (lib, M, K, V, bf16 operands?)."""
    bf = X.dtype == BF16 or W.dtype == BF16            # both or neither: a mix fails W's or X's dtype check
    dt = BF16 if bf else torch.float32
    _chk(X, dt, "X"), _chk(W, dt, "W")
    if bias is not None:
        _chk(bias, name="bias")
    lib = _lib.load()
    M, K = X.shape
    V = W.shape[1]
    if W.shape[0] != K:
        raise _lib.DcapError("%s: inner dimensions differ (%d vs %d)" % (fn, K, W.shape[0]))
    if K % (8 if bf else 32):
        raise _lib.DcapError("%s: K must be a multiple of %d, got %d" % (fn, 8 if bf else 32, K))
    if bias is not None and tuple(bias.shape) != (V,):
        raise _lib.DcapError("%s: bias must be [V]" % fn)
    if tile and not bf:
        raise _lib.DcapError("%s: tile= chooses between the bf16 kernels; float32 operands have one tile shape" % fn)
    return lib, M, K, V, bf


def vocab_topk_bf16_tile(M, V, K):
    """The tile shape (128 or 256) vocab_top1 / vocab_topk run bf16 operands of this problem size on when tile is 0 / None."""
    return int(_lib.load().dc_vocab_topk_bf16_tile(int(M), int(V), int(K)))


def vocab_top1(X, W, bias=None, tokens=None, ids=None, probs=None, mask=None, tile=None):
    """Fused Dense(V) + greedy top-1: per row of X [M,K] the argmax of X W + bias (lowest index on ties) into tokens int32 [M]
    (contiguous), optionally also into ids / probs (int32 / float32 length-M vectors with any
    stride -- e.g. column j of [B,T] outputs; probs = the softmax probability of the chosen word) and mask uint8 [M] (id != 0).  The
    [M,V] logits are never materialised.  Every V >= 1: a W whose rows are not 16-byte chunks is copied once into a padded buffer.
    X and W both float32 (dc_vocab_top1_f32: fp32 MFMA products, K % 32 == 0) or both bf16 (dc_vocab_top1_bf16: the bf16 matrix pipe,
    fp32 accumulation, K % 8 == 0; tile = None / 0 (automatic), 128 or 256 picks its tile shape); bias float32 either way."""
    lib, M, K, V, bf = _vocab_args("vocab_top1", X, W, bias, tile)
    if tokens is None:
        tokens = torch.empty((M,), dtype=torch.int32, device=X.device)
    if not _chk(tokens, torch.int32, "tokens").is_contiguous() or tokens.numel() != M:
        raise _lib.DcapError("vocab_top1: tokens must be a contiguous int32 [M] tensor")
    if mask is not None and (not _chk(mask, torch.uint8, "mask").is_contiguous() or mask.numel() != M):
        raise _lib.DcapError("vocab_top1: mask must be a contiguous uint8 [M] tensor")
    ids_p, ld_ids = _row_out(ids, M, torch.int32, "ids")
    probs_p, ld_probs = _row_out(probs, M, torch.float32, "probs")
    if M == 0:
        return tokens
    X, W, bias = _vocab_operands(X, W, bias)
    d = VocabTop1Bf16Desc() if bf else VocabTop1Desc()
    d.M, d.V, d.K = M, V, K
    d.X, d.ldx, d.W, d.ldw = X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0)
    d.bias = _ptr(bias)
    d.tokens = tokens.data_ptr()
    d.ids, d.ld_ids, d.probs, d.ld_probs = ids_p, ld_ids, probs_p, ld_probs
    d.mask = _ptr(mask)
    if bf:
        d.tile = int(tile or 0)
        _launch_ws(lib.dc_vocab_top1_bf16_workspace_bytes(M, V, K, d.tile), X.device, lib.dc_vocab_top1_bf16, C.byref(d))
    else:
        _launch_ws(lib.dc_vocab_top1_workspace_bytes(M, V), X.device, lib.dc_vocab_top1_f32, C.byref(d))
    return tokens


TOPK_MAX = 8


def vocab_topk(X, W, bias, k, ids=None, probs=None, tile=None):
    """Fused Dense(V) + row top-k (beam search): per row of X [M,K] the k best words of
    X W + bias in the order logit descending, then index ascending, into ids int32 [M,k], and their softmax probabilities into probs
    float32 [M,k] (both contiguous; allocated when None).  1 <= k <= 8 and V >= k; any V (W padded as for vocab_top1).  The [M,V]
    logits are never materialised.  k = 1 gives vocab_top1's ids and probabilities.  Operands as vocab_top1: float32 (dc_vocab_topk_f32,
    K % 32 == 0) or bf16 (dc_vocab_topk_bf16, K % 8 == 0, tile=).  Returns (ids, probs)."""
    lib, M, K, V, bf = _vocab_args("vocab_topk", X, W, bias, tile)
    k = int(k)
    if not 1 <= k <= TOPK_MAX or V < k:
        raise _lib.DcapError("vocab_topk: need 1 <= k <= %d and V >= k, got k = %d, V = %d" % (TOPK_MAX, k, V))
    if ids is None:
        ids = torch.empty((M, k), dtype=torch.int32, device=X.device)
    if probs is None:
        probs = torch.empty((M, k), dtype=torch.float32, device=X.device)
    for name, t, dt in (("ids", ids, torch.int32), ("probs", probs, torch.float32)):
        if not _chk(t, dt, name).is_contiguous() or tuple(t.shape) != (M, k):
            raise _lib.DcapError("vocab_topk: %s must be a contiguous %s [M,k] tensor" % (name, dt))
    if M == 0:
        return ids, probs
    X, W, bias = _vocab_operands(X, W, bias)
    d = VocabTopkBf16Desc() if bf else VocabTopkDesc()
    d.M, d.V, d.K, d.k = M, V, K, k
    d.X, d.ldx, d.W, d.ldw = X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0)
    d.bias = _ptr(bias)
    d.ids, d.probs = ids.data_ptr(), probs.data_ptr()
    if bf:
        d.tile = int(tile or 0)
        _launch_ws(lib.dc_vocab_topk_bf16_workspace_bytes(M, V, K, k, d.tile), X.device, lib.dc_vocab_topk_bf16, C.byref(d))
    else:
        _launch_ws(lib.dc_vocab_topk_workspace_bytes(M, V, k), X.device, lib.dc_vocab_topk_f32, C.byref(d))
    return ids, probs


def vocab_sample(X, W, bias=None, *, temperature=1.0, top_k=None, seed, offset=0, tokens=None, ids=None, probs=None, mask=None, tile=None):
    """Fused Dense(V) + one draw per row from softmax((X W + bias) / temperature), by the Gumbel-max identity: the word
    argmax_v (z_v / temperature + g(i, v)), the lower index on equal values, with g standard Gumbel noise that is a pure function of
    (seed, offset + i, v) (Philox-2x32-10; include/dcap.h, dc_vocab_sample_f32) -- the same seed and offset draw the same words at every
    M, tile and precision path, row i of a call is row 0 of a call at offset + i, and there is no generator state.  seed and offset are
    integers in [0, 2^32); temperature a finite float > 0.  top_k (None, or 1..TOPK_MAX with V >= top_k) restricts the draw to the
    row's top_k best words (vocab_topk's); top_k = 1 is vocab_top1, bit for bit.  Outputs as vocab_top1: tokens int32 [M], optional
    strided ids / probs, optional mask; probs is the chosen word's softmax probability at temperature 1 over the whole vocabulary
    (what vocab_top1 and vocab_topk report), not its probability under the sampling distribution.  The [M,V] logits are never
    materialised.  Operands as vocab_top1 (float32, or bf16 with tile=; over the whole vocabulary bf16 runs on the 128 tile only).
    Returns tokens."""
    V = W.shape[1]                                      # the scalar arguments first: refused before any tensor is looked at
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float, np.floating, np.integer)) or \
            not (np.isfinite(temperature) and temperature > 0):
        raise _lib.DcapError("vocab_sample: temperature must be a finite float > 0, got %r" % (temperature,))
    with np.errstate(over="ignore"):
        inv_t = float(np.float32(1.0 / float(temperature)))
    if not (np.isfinite(inv_t) and inv_t > 0):
        raise _lib.DcapError("vocab_sample: 1 / temperature must be a finite float32 > 0, got temperature %r" % (temperature,))
    if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or not 1 <= top_k <= TOPK_MAX or top_k > V):
        raise _lib.DcapError("vocab_sample: top_k must be None or an integer in 1..%d, at most V = %d, got %r" % (TOPK_MAX, V, top_k))
    for name, v in (("seed", seed), ("offset", offset)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < 2 ** 32:
            raise _lib.DcapError("vocab_sample: %s must be an integer in [0, 2^32), got %r" % (name, v))
    lib, M, K, V, bf = _vocab_args("vocab_sample", X, W, bias, tile)
    if bf and tile == 256 and top_k is None:
        raise _lib.DcapError("vocab_sample: sampling over the whole vocabulary (top_k=None) runs on the 128 x 128 tile only: pass tile=128 or "
                             "None (the 256 x 256 bf16 tile has no sampling epilogue)")
    if tokens is None:
        tokens = torch.empty((M,), dtype=torch.int32, device=X.device)
    if not _chk(tokens, torch.int32, "tokens").is_contiguous() or tokens.numel() != M:
        raise _lib.DcapError("vocab_sample: tokens must be a contiguous int32 [M] tensor")
    if mask is not None and (not _chk(mask, torch.uint8, "mask").is_contiguous() or mask.numel() != M):
        raise _lib.DcapError("vocab_sample: mask must be a contiguous uint8 [M] tensor")
    ids_p, ld_ids = _row_out(ids, M, torch.int32, "ids")
    probs_p, ld_probs = _row_out(probs, M, torch.float32, "probs")
    if M == 0:
        return tokens
    X, W, bias = _vocab_operands(X, W, bias)
    d = VocabSampleBf16Desc() if bf else VocabSampleDesc()
    d.M, d.V, d.K = M, V, K
    d.X, d.ldx, d.W, d.ldw = X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0)
    d.bias = _ptr(bias)
    d.tokens = tokens.data_ptr()
    d.ids, d.ld_ids, d.probs, d.ld_probs = ids_p, ld_ids, probs_p, ld_probs
    d.mask = _ptr(mask)
    d.inv_t, d.seed, d.offset, d.top_k = inv_t, int(seed), int(offset), int(top_k or 0)
    if bf:
        d.tile = int(tile or 0)
        _launch_ws(lib.dc_vocab_sample_bf16_workspace_bytes(M, V, K, d.top_k, d.tile), X.device, lib.dc_vocab_sample_bf16, C.byref(d))
    else:
        _launch_ws(lib.dc_vocab_sample_workspace_bytes(M, V, d.top_k), X.device, lib.dc_vocab_sample_f32, C.byref(d))
    return tokens


def _beam_args(fn, d, cand_ids, cand_probs, scores_in, scores_out, parents, tokens_hist, j, nb, log_score, tokens, mask, more=()):
    """beam_select's and beam_step's (fn: which, for the messages) common checks -- more: further (name, tensor, dtype, shape) entries like
    tokens / mask -- and the fields their descriptors share, into d.  Returns (lib, R, k)."""
    lib = _lib.load()
    R, k = scores_out.shape
    _chk(scores_out, name="scores_out")
    for name, t, dt, shape in (("cand_ids", cand_ids, torch.int32, (k * R, k)), ("cand_probs", cand_probs, torch.float32, (k * R, k)),
                               ("scores_in", scores_in, torch.float32, (R, k)), ("tokens", tokens, torch.int32, (k * R,)),
                               ("mask", mask, torch.uint8, (k * R,))) + tuple(more):
        if t is not None and (not _chk(t, dt, name).is_contiguous() or tuple(t.shape) != shape):
            raise _lib.DcapError("%s: %s must be a contiguous %s %s tensor" % (fn, name, dt, shape))
    steps = parents.shape[0]
    for name, t in (("parents", parents), ("tokens_hist", tokens_hist)):
        if not _chk(t, torch.int32, name).is_contiguous() or tuple(t.shape) != (steps, R, k):
            raise _lib.DcapError("%s: %s must be a contiguous int32 [steps,R,k] tensor" % (fn, name))
    if not scores_out.is_contiguous() or not 1 <= k <= TOPK_MAX or not 1 <= nb <= k or not 0 <= j < steps:
        raise _lib.DcapError("%s: need contiguous scores_out, 1 <= nb <= k <= %d, 0 <= j < steps" % (fn, TOPK_MAX))
    d.R, d.k, d.nb, d.steps, d.j, d.log_score = R, k, int(nb), steps, int(j), int(bool(log_score))
    d.cand_ids, d.cand_probs, d.scores_in, d.scores_out = cand_ids.data_ptr(), cand_probs.data_ptr(), _ptr(scores_in), scores_out.data_ptr()
    d.parents, d.tokens_hist, d.tokens, d.mask = parents.data_ptr(), tokens_hist.data_ptr(), _ptr(tokens), _ptr(mask)
    return lib, R, k


def beam_select(cand_ids, cand_probs, scores_in, scores_out, parents, tokens_hist, j, nb, log_score=False, tokens=None, mask=None,
                h_in=None, c_in=None, h_out=None, c_out=None):
    """One beam-search step (dc_beam_select_f32) for R RoIs x k beams, beam-major rows (beam b of RoI r = row b * R + r):
    cand_ids / cand_probs [k*R,k] (vocab_topk's output), scores_in [R,k] (None: zeros, the first step) -> the k best of the first nb
    beams' candidates (score + p, or + log p with log_score), best first: scores_out [R,k], parents / tokens_hist [steps,R,k] at step j,
    tokens int32 [k*R] and mask uint8 [k*R] (token != 0) when given, and h_in / c_in [k*R,U] gathered by parent into h_out / c_out."""
    d = BeamSelectDesc()
    lib, R, k = _beam_args("beam_select", d, cand_ids, cand_probs, scores_in, scores_out, parents, tokens_hist, j, nb, log_score, tokens, mask)
    rows = (h_in, c_in, h_out, c_out)
    U = 0
    if any(t is not None for t in rows):
        if any(t is None for t in rows):
            raise _lib.DcapError("beam_select: h_in, c_in, h_out, c_out are all given or all None")
        U = h_in.shape[-1]
        for name, t in zip(("h_in", "c_in", "h_out", "c_out"), rows):
            if not _chk(t, name=name).is_contiguous() or tuple(t.shape) != (k * R, U):
                raise _lib.DcapError("beam_select: %s must be a contiguous float32 [k*R,U] tensor" % name)
    if R == 0:
        return scores_out
    d.U, d.h_in, d.c_in, d.h_out, d.c_out = U, _ptr(h_in), _ptr(c_in), _ptr(h_out), _ptr(c_out)
    check(lib.dc_beam_select_f32(C.byref(d), _stream()), "dc_beam_select_f32")
    return scores_out


def beam_step(cand_ids, cand_probs, scores_in, scores_out, parents, tokens_hist, j, nb, log_score=False, tokens=None, mask=None,
              rows=(), end_id=None, finished_in=None, finished_out=None):
    """One beam-search step (dc_beam_step_f32): beam_select's step -- the same rows, order (score descending, parent beam ascending, word
    id ascending) and outputs -- with row sets and an end token.  rows: up to 4 (src, dst) pairs of float32 [k*R,U] tensors (U % 4 == 0,
    widths may differ, 16-byte aligned, no dst overlapping a src or another dst): row q*R + r of dst receives row parent*R + r of src.
    end_id (None: no end token): a beam whose finished_in byte (uint8 [k*R]; None: nobody is finished) is set proposes one candidate,
    token 0 at its unchanged score, and its cand_ids / cand_probs rows are not read; finished_out (uint8 [k*R], required with end_id,
    not finished_in) marks the new beams whose parent was finished or whose token is end_id.  A finished beam's token 0 writes mask 0."""
    rows = tuple(rows)
    if len(rows) > _lib.BEAM_MAX_SETS:
        raise _lib.DcapError("beam_step: at most %d row sets, got %d" % (_lib.BEAM_MAX_SETS, len(rows)))
    if end_id is not None and (isinstance(end_id, bool) or int(end_id) != end_id or end_id < 0):
        raise _lib.DcapError("beam_step: end_id must be a word id or None, got %r" % (end_id,))
    if end_id is not None and finished_out is None:
        raise _lib.DcapError("beam_step: end_id needs finished_out")
    if finished_out is not None and finished_in is not None and finished_out.data_ptr() == finished_in.data_ptr():
        raise _lib.DcapError("beam_step: finished_out must not alias finished_in")
    R, k = scores_out.shape
    spans = []
    for i, pair in enumerate(rows):
        if len(pair) != 2:
            raise _lib.DcapError("beam_step: row set %d must be a (src, dst) pair" % i)
        src, dst = pair
        for name, t in (("src", src), ("dst", dst)):
            if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or tuple(t.shape) != (k * R, src.shape[-1]):
                raise _lib.DcapError("beam_step: row set %d: %s must be a contiguous float32 [k*R,U] tensor" % (i, name))
            if t.shape[1] % 4 or t.data_ptr() % 16:
                raise _lib.DcapError("beam_step: row set %d: %s needs U %% 4 == 0 and a 16-byte aligned base" % (i, name))
        spans.append(((src.data_ptr(), src.data_ptr() + src.numel() * 4), (dst.data_ptr(), dst.data_ptr() + dst.numel() * 4)))
    for i, (_, d0) in enumerate(spans):
        for o, (s1, d1) in enumerate(spans):
            if any(a[0] < b[1] and b[0] < a[1] for a, b in ((d0, s1),) + (((d0, d1),) if o != i else ())):
                raise _lib.DcapError("beam_step: dst of row set %d must not alias a src or another dst (set %d)" % (i, o))
    d = BeamStepDesc()
    lib, R, k = _beam_args("beam_step", d, cand_ids, cand_probs, scores_in, scores_out, parents, tokens_hist, j, nb, log_score, tokens, mask,
                           more=(("finished_in", finished_in, torch.uint8, (k * R,)), ("finished_out", finished_out, torch.uint8, (k * R,))))
    for i, (src, dst) in enumerate(rows):
        _chk(src, name="rows[%d] src" % i), _chk(dst, name="rows[%d] dst" % i)
    if R == 0:
        return scores_out
    d.end_id, d.finished_in, d.finished_out = -1 if end_id is None else int(end_id), _ptr(finished_in), _ptr(finished_out)
    d.n_sets = len(rows)
    for i, (src, dst) in enumerate(rows):
        d.U[i], d.src[i], d.dst[i] = src.shape[1], src.data_ptr(), dst.data_ptr()
    check(lib.dc_beam_step_f32(C.byref(d), _stream()), "dc_beam_step_f32")
    return scores_out


def beam_backtrace(parents, tokens_hist, out=None):
    """parents / tokens_hist int32 [steps,R,k] (beam_select's history) -> the beams' token sequences int32 [R,k,steps] (dc_beam_backtrace)."""
    lib = _lib.load()
    for name, t in (("parents", parents), ("tokens_hist", tokens_hist)):
        if not _chk(t, torch.int32, name).is_contiguous() or t.dim() != 3:
            raise _lib.DcapError("beam_backtrace: %s must be a contiguous int32 [steps,R,k] tensor" % name)
    steps, R, k = parents.shape
    if tuple(tokens_hist.shape) != (steps, R, k):
        raise _lib.DcapError("beam_backtrace: parents and tokens_hist differ in shape")
    if out is None:
        out = torch.empty((R, k, steps), dtype=torch.int32, device=parents.device)
    if not _chk(out, torch.int32, "out").is_contiguous() or tuple(out.shape) != (R, k, steps):
        raise _lib.DcapError("beam_backtrace: out must be a contiguous int32 [R,k,steps] tensor")
    if R == 0 or steps == 0:
        return out
    check(lib.dc_beam_backtrace(parents.data_ptr(), tokens_hist.data_ptr(), steps, R, k, out.data_ptr(), _stream()), "dc_beam_backtrace")
    return out


def argmax_rows(x, out=None):
    lib = _lib.load()
    _chk(x, name="x")
    if out is None:
        out = torch.empty((x.shape[0],), dtype=torch.int32, device=x.device)
    check(lib.dc_argmax_rows_f32(_ptr(x), x.shape[0], x.shape[1], x.stride(0), _ptr(out), _stream()), "dc_argmax_rows_f32")
    return out


def gather_rows(src, idx, out, width=None):
    """out[n, :width] = src[idx[n], :width] (zeros where idx[n] < 0); out may be a column slice."""
    lib = _lib.load()
    _chk(src, name="src"), _chk(out, name="out"), _chk(idx, torch.int32, "idx")
    width = out.shape[1] if width is None else width
    check(lib.dc_gather_rows_f32(_ptr(src), src.stride(0), _ptr(idx), _ptr(out), out.stride(0), idx.numel(), width, _stream()),
          "dc_gather_rows_f32")
    return out


def _bn_desc(acc, bias, gamma, beta, mean, var, eps):
    d = BnReluDesc()
    d.M, d.N, d.ld = acc.shape[0], acc.shape[1], acc.stride(0)
    d.acc = _chk(acc, name="acc").data_ptr()
    d.bias, d.gamma, d.beta, d.mean, d.var = (_chk(t, name="bn param").data_ptr() for t in (bias, gamma, beta, mean, var))
    d.eps = float(eps)
    return d


def bn_relu_fwd(acc, bias, gamma, beta, mean, var, out, eps=1e-3):
    """out = relu(gamma*(acc + bias - mean)/sqrt(var+eps) + beta); acc/out [M,N] sharing a row stride."""
    lib = _lib.load()
    d = _bn_desc(acc, bias, gamma, beta, mean, var, eps)
    if _chk(out, name="out").stride(0) != acc.stride(0):
        raise _lib.DcapError("bn_relu_fwd: out must share acc's row stride")
    d.y = out.data_ptr()
    check(lib.dc_bn_relu_fwd_f32(C.byref(d), _stream()), "dc_bn_relu_fwd_f32")
    return out


def bn_relu_bwd(acc, bias, gamma, beta, mean, var, dy, dacc, dgamma, dbeta, dbias, eps=1e-3):
    lib = _lib.load()
    d = _bn_desc(acc, bias, gamma, beta, mean, var, eps)
    for t in (dy, dacc):
        if _chk(t, name="dy/dacc").stride(0) != acc.stride(0):
            raise _lib.DcapError("bn_relu_bwd: dy and dacc must share acc's row stride")
    d.dy, d.dacc = dy.data_ptr(), dacc.data_ptr()
    d.dgamma, d.dbeta, d.dbias = (_chk(t, name="bn grad").data_ptr() for t in (dgamma, dbeta, dbias))
    check(lib.dc_bn_relu_bwd_f32(C.byref(d), _stream()), "dc_bn_relu_bwd_f32")
    return dacc


def conv_weight_dgrad_pack(w_packed, kh, kw, cin, out=None):
    """[Cout][kh*kw*Cin] -> [Cin][kh*kw*Cout] with the taps rotated: the weights that make conv2d() the data gradient."""
    lib = _lib.load()
    cout = w_packed.shape[0]
    if out is None:
        out = torch.empty((cin, kh * kw * cout), dtype=torch.float32, device=w_packed.device)
    check(lib.dc_conv_weight_dgrad_pack_f32(_ptr(_chk(w_packed, name="w")), _ptr(out), cout, kh, kw, cin, _stream()),
          "dc_conv_weight_dgrad_pack_f32")
    return out


def rpn_loss_grad(heads, dheads, sel_level, sel_index, sel_match, target_deltas, n_pos, losses, image=0, anchors_per_loc=3, counts_dev=None,
                  batched=False):
    """RPN class + bbox losses of image `image` and their gradients scattered into the (pre-zeroed) dheads.  counts_dev: int32 device
    tensor {n_sel, n_pos} overriding the host counts (sel_* / target_deltas then have fixed capacities: graph-capturable).
    batched=True: the selection indexes the WHOLE [B, h, w, C] head tensors (image b's anchor i of a level = b * h * w * A + i, images
    in order, target rows packed in the same order): both means then run over the batch's union of selected anchors, as the
    reference's batched loss graphs do (dense_img_cap/dense_model.py:877-933)."""
    lib = _lib.load()
    d = RpnLossDesc()
    d.levels, d.anchors_per_loc, d.head_stride = len(heads), anchors_per_loc, heads[0].shape[-1]
    for i, (h, g) in enumerate(zip(heads, dheads)):
        per = h.shape[1] * h.shape[2] * h.shape[3]
        d.heads[i] = h.data_ptr() + 4 * per * image
        d.dheads[i] = g.data_ptr() + 4 * per * image
        d.Hs[i], d.Ws[i] = (h.shape[0] * h.shape[1] if batched else h.shape[1]), h.shape[2]      # (a batch is a taller map to the kernel's bound check)
    d.n_sel, d.n_pos = sel_level.numel(), int(n_pos)
    if d.n_sel:                                         # no selected anchor (all neutral): the kernel only zeroes the losses
        d.sel_level, d.sel_index, d.sel_match = (_chk(t, torch.int32, "sel").data_ptr() for t in (sel_level, sel_index, sel_match))
    d.target_deltas = _chk(target_deltas, name="target_deltas").data_ptr()
    d.losses = _chk(losses, name="losses").data_ptr()
    if counts_dev is not None:
        d.counts_dev = _chk(counts_dev, torch.int32, "counts_dev").data_ptr()
        d.n_pos = min(int(n_pos), target_deltas.shape[0])
    check(lib.dc_rpn_loss_grad_f32(C.byref(d), _stream()), "dc_rpn_loss_grad_f32")


def detection_targets(proposals, gt_boxes, gt_captions, n_rois, positive_ratio, seed=None, offset=0, offset_dev=None, out=None):
    """DetectionTargetLayer for one image on the device (dc_detection_targets_f32).  proposals [N,4] / gt_boxes [G,4] float32
    normalised, gt_captions [G,T] int32.  seed None: proposal order (no shuffle).  Returns (rois [n_rois,4], captions [n_rois,T] int32,
    counts int32 [2] = {n_pos, n_neg}) -- device tensors, nothing is read back."""
    lib = _lib.load()
    _chk(proposals, name="proposals"), _chk(gt_boxes, name="gt_boxes"), _chk(gt_captions, torch.int32, "gt_captions")
    N, G, T = proposals.shape[0], gt_boxes.shape[0], gt_captions.shape[1]
    if gt_captions.shape[0] != G or not (proposals.is_contiguous() and gt_boxes.is_contiguous() and gt_captions.is_contiguous()):
        raise _lib.DcapError("detection_targets: gt_captions must have one row per GT box; operands contiguous")
    if out is None:
        out = (torch.empty((n_rois, 4), dtype=torch.float32, device=proposals.device),
               torch.empty((n_rois, T), dtype=torch.int32, device=proposals.device),
               torch.empty((2,), dtype=torch.int32, device=proposals.device))
    rois, caps, counts = out
    d = DetectionTargetsDesc()
    d.n_proposals, d.n_gt, d.n_rois, d.T = N, G, int(n_rois), T
    d.proposals, d.gt_boxes, d.gt_captions = proposals.data_ptr(), gt_boxes.data_ptr(), gt_captions.data_ptr()
    d.max_positive = int(n_rois * positive_ratio)
    import numpy as _np
    d.inv_ratio = float(_np.float32(1.0 / positive_ratio))
    d.shuffle, d.seed, d.offset = int(seed is not None), (int(seed or 0) & 0xFFFFFFFF), int(offset) & 0xFFFFFFFF
    d.offset_dev = None if offset_dev is None else _chk(offset_dev, torch.int32, "offset_dev").data_ptr()
    d.rois, d.captions, d.counts = _chk(rois, name="rois").data_ptr(), _chk(caps, torch.int32, "captions").data_ptr(), _chk(counts, torch.int32, "counts").data_ptr()
    check(lib.dc_detection_targets_f32(C.byref(d), _stream()), "dc_detection_targets_f32")
    return rois, caps, counts


def rpn_targets(anchors, gt_boxes, gt_counts, level_sizes, anchors_per_image_budget, std_dev, seed, offset=0, offset_dev=None, out=None):
    """build_rpn_targets for B images on the device (dc_rpn_targets_f64), in the packed form rpn_loss_grad(batched=True) reads.
    anchors [A,4] float64, gt_boxes [B,G,4] float64 (G <= 512: the capacity), gt_counts int32 [B] (the images' box counts, read on the
    device), level_sizes: anchors per image of each pyramid level, std_dev: RPN_BBOX_STD_DEV.  Image b's subsampling keys are
    Philox(anchor, offset + offset_dev, seed + b * 0x85EBCA6B).  out / returns (counts int32 [2] = {n_sel, n_pos}, lvl, idx, mt int32
    [B * budget], deltas float32 [B * budget, 4]) -- device tensors, nothing is read back."""
    lib = _lib.load()
    _chk(anchors, torch.float64, "anchors"), _chk(gt_boxes, torch.float64, "gt_boxes"), _chk(gt_counts, torch.int32, "gt_counts")
    if anchors.dim() != 2 or anchors.shape[1] != 4 or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4 or gt_counts.numel() != gt_boxes.shape[0]:
        raise _lib.DcapError("rpn_targets: anchors [A,4], gt_boxes [B,G,4], gt_counts [B]")
    if not (anchors.is_contiguous() and gt_boxes.is_contiguous() and gt_counts.is_contiguous()):
        raise _lib.DcapError("rpn_targets: operands must be contiguous")
    B, n = gt_boxes.shape[0], int(anchors_per_image_budget)
    sizes = [int(v) for v in level_sizes]
    if not 1 <= len(sizes) <= 5:
        raise _lib.DcapError("rpn_targets: 1..5 pyramid levels, got %d" % len(sizes))
    cap = B * max(n, 0)
    if out is None:
        dev = anchors.device
        out = (torch.empty(2, dtype=torch.int32, device=dev),) + tuple(torch.empty(max(cap, 1), dtype=torch.int32, device=dev) for _ in range(3)) + (
            torch.empty((max(cap, 1), 4), dtype=torch.float32, device=dev),)
    counts, lvl, idx, mt, deltas = out
    for t, name in ((counts, "counts"), (lvl, "lvl"), (idx, "idx"), (mt, "mt")):
        _chk(t, torch.int32, name)
    _chk(deltas, name="deltas")
    if counts.numel() < 2 or min(lvl.numel(), idx.numel(), mt.numel()) < cap or deltas.numel() < 4 * cap or not deltas.is_contiguous():
        raise _lib.DcapError("rpn_targets: outputs need 2 count words and B * budget = %d rows" % cap)
    d = RpnTargetsDesc()
    d.B, d.A, d.n_levels = B, anchors.shape[0], len(sizes)
    for i, v in enumerate(sizes):
        d.level_sizes[i] = v
    d.gt_capacity, d.budget = gt_boxes.shape[1], n
    d.anchors, d.gt_boxes, d.gt_counts = anchors.data_ptr(), gt_boxes.data_ptr(), gt_counts.data_ptr()
    for i, v in enumerate(std_dev):
        d.std_dev[i] = float(v)
    d.seed, d.offset = int(seed) & 0xFFFFFFFF, int(offset) & 0xFFFFFFFF
    d.offset_dev = None if offset_dev is None else _chk(offset_dev, torch.int32, "offset_dev").data_ptr()
    d.counts, d.sel_level, d.sel_index, d.sel_match, d.deltas = counts.data_ptr(), lvl.data_ptr(), idx.data_ptr(), mt.data_ptr(), deltas.data_ptr()
    _launch_ws(lib.dc_rpn_targets_workspace(C.byref(d)), anchors.device, lib.dc_rpn_targets_f64, C.byref(d))
    return counts, lvl, idx, mt, deltas


def caption_tables(captions, out=None, live_count=None):
    """captions int32 [B,T] (device) -> (ids_tm int32 [T*B], mask uint8 [T*B], targets_tm int32 [T*B], row_weights f32 [T*B])."""
    lib = _lib.load()
    _chk(captions, torch.int32, "captions")
    B, T = captions.shape
    dev = captions.device
    if out is None:
        out = (torch.empty(T * B, dtype=torch.int32, device=dev), torch.empty(T * B, dtype=torch.uint8, device=dev),
               torch.empty(T * B, dtype=torch.int32, device=dev), torch.empty(T * B, dtype=torch.float32, device=dev))
    ids, mask, tg, rw = out
    check(lib.dc_caption_tables_i32(_ptr(captions), B, T, _ptr(ids), _ptr(mask), _ptr(tg), _ptr(rw),
                                    None if live_count is None else _ptr(live_count), _stream()), "dc_caption_tables_i32")
    return ids, mask, tg, rw


def scatter2_add(coarse, fine):
    lib = _lib.load()
    N, Hc, Wc, Cc = coarse.shape
    check(lib.dc_scatter2_add_f32(_ptr(_chk(coarse, name="coarse")), _ptr(_chk(fine, name="fine")), N, Hc, Wc, Cc, _stream()), "dc_scatter2_add_f32")
    return fine


def l2_reg(w, coef, grad=None, loss=None, mask=None):
    """grad = grad * mask + 2 coef w (mask None: all ones); loss[0] = sum coef w^2 in a fixed order."""
    lib = _lib.load()
    _launch_ws(lib.dc_l2_reg_workspace_bytes(w.numel()) if loss is not None else 0, w.device, lib.dc_l2_reg_f32,
               _ptr(_chk(w, name="w")), _ptr(_chk(coef, name="coef")), None if mask is None else _ptr(_chk(mask, name="mask")),
               None if grad is None else _ptr(grad), w.numel(), None if loss is None else _ptr(loss))
    return loss


def set_persistent_cus(n):
    """CUs the persistent Winograd grids may occupy (0 = default); see dc_set_persistent_cus in include/dcap.h."""
    lib = _lib.load()
    check(lib.dc_set_persistent_cus(int(n)), "dc_set_persistent_cus")
    return int(lib.dc_get_persistent_cus())


def zero_fill(t):
    """t[...] = 0 by the library's zero-fill kernel (contiguous tensor of 4-byte-multiple size): no torch fill launch on the product path."""
    lib = _lib.load()
    if not t.is_contiguous() or not t.is_cuda:
        raise _lib.DcapError("zero_fill: a contiguous GPU tensor")
    check(lib.dc_zero_fill(_ptr(t), t.numel() * t.element_size(), _stream()), "dc_zero_fill")
    return t


def axpy(a, x, y):
    lib = _lib.load()
    check(lib.dc_axpy_f32(float(a), _ptr(_chk(x, name="x")), _ptr(_chk(y, name="y")), x.numel(), _stream()), "dc_axpy_f32")
    return y


def relu_bwd(dy, y, out, out_bf16=None):
    """out = dy where y > 0 else 0 (all [M,N] with one row stride).  out_bf16 (contiguous operands only): the bf16 copy of the result,
    written in the same pass (dc_relu_bwd_dual_f32)."""
    lib = _lib.load()
    _chk(dy, name="dy"), _chk(y, name="y"), _chk(out, name="out")
    if out_bf16 is not None:
        if not (dy.is_contiguous() and y.is_contiguous() and out.is_contiguous() and out_bf16.is_contiguous()) or out_bf16.numel() != out.numel():
            raise _lib.DcapError("relu_bwd: the bf16 copy needs contiguous operands of one size")
        check(lib.dc_relu_bwd_dual_f32(_ptr(dy), _ptr(y), _ptr(out), _ptr(_chk(out_bf16, BF16, "out_bf16")), out.numel(), _stream()), "dc_relu_bwd_dual_f32")
        return out
    if not (dy.stride(0) == y.stride(0) == out.stride(0)):
        raise _lib.DcapError("relu_bwd: tensors must share a row stride")
    check(lib.dc_relu_bwd_f32(_ptr(dy), _ptr(y), _ptr(out), y.shape[0], y.shape[1], y.stride(0), _stream()), "dc_relu_bwd_f32")
    return out


def fold_time(x, T, B, out):
    """out[b] = sum_t x[t*B + b] (time-major rows)."""
    lib = _lib.load()
    _chk(x, name="x"), _chk(out, name="out")
    check(lib.dc_fold_time_f32(_ptr(x), T, B, x.shape[1], x.stride(0), _ptr(out), out.stride(0), _stream()), "dc_fold_time_f32")
    return out


def embedding_grad(dx, ids, out):
    """out[v] = the sum, in ascending m, of the rows dx[m] with ids[m] == v (dc_embedding_grad_f32): the gradient of a trainable embedding
    table out [V,W] from d(embedded tokens) dx [n,W] and the int32 ids [n].  Every row of out is written (zeros for absent words)."""
    lib = _lib.load()
    _chk(dx, name="dx"), _chk(out, name="out"), _chk(ids, torch.int32, "ids")
    if dx.dim() != 2 or out.dim() != 2 or dx.shape[1] != out.shape[1] or ids.numel() != dx.shape[0] or not ids.is_contiguous():
        raise _lib.DcapError("embedding_grad: dx [n,W], contiguous ids [n], out [V,W]; got %s, %s, %s" % (tuple(dx.shape), tuple(ids.shape), tuple(out.shape)))
    n, W = dx.shape
    check(lib.dc_embedding_grad_f32(_ptr(dx), dx.stride(0) if n > 1 else W, _ptr(ids), n, _ptr(out), out.stride(0) if out.shape[0] > 1 else W,
                                    out.shape[0], W, _stream()), "dc_embedding_grad_f32")
    return out


def row_mean(x, out=None):
    """np.mean(x, axis=0) of a float32 x [K,C] -> out [C], or of every block of x [B,K,C] -> out [B,C] in the same launch, bit for bit
    (dc_row_mean_f32: the additions sequential over k, one correctly rounded division).  Rows and blocks may have any stride and the
    base any alignment; out (allocated when None) needs unit stride along C.  K = 0 or C = 0 is the library's DC_EINVAL."""
    lib = _lib.load()
    if _chk(x, name="x").dim() not in (2, 3):
        raise _lib.DcapError("row_mean: x must be a float32 [K,C] or [B,K,C] tensor, got %s" % (tuple(x.shape),))
    B, (K, Cn) = (x.shape[0] if x.dim() == 3 else 1), x.shape[-2:]
    shape = (B, Cn) if x.dim() == 3 else (Cn,)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    if tuple(_chk(out, name="out").shape) != shape or out.device != x.device:
        raise _lib.DcapError("row_mean: out must be a float32 %s tensor on x's device" % (shape,))
    ld = x.stride(-2) if K > 1 else max(Cn, 1)
    bs = x.stride(0) if x.dim() == 3 and B > 1 else 0
    ld_out = out.stride(0) if x.dim() == 3 and B > 1 else max(Cn, 1)
    check(lib.dc_row_mean_f32(_ptr(x), B, K, Cn, ld, bs, _ptr(out), ld_out, _stream()), "dc_row_mean_f32")
    return out


def colsum(x, out=None, accumulate=False):
    lib = _lib.load()
    _chk(x, name="x")
    if out is None:
        out = torch.empty((x.shape[1],), dtype=torch.float32, device=x.device)
    M, N, ld = x.shape[0], x.shape[1], x.stride(0)
    _launch_ws(lib.dc_colsum_workspace_bytes(M, N, ld), x.device, lib.dc_colsum_f32, _ptr(x), M, N, ld, _ptr(out), int(accumulate))
    return out


def sumsq(x, out=None, accumulate=False):
    lib = _lib.load()
    if out is None:
        out = torch.empty((1,), dtype=torch.float32, device=x.device)
    _launch_ws(lib.dc_sumsq_workspace_bytes(x.numel()), x.device, lib.dc_sumsq_f32, _ptr(_chk(x, name="x")), x.numel(), _ptr(out), int(accumulate))
    return out


def mean(x, out=None):
    lib = _lib.load()
    if out is None:
        out = torch.empty((1,), dtype=torch.float32, device=x.device)
    check(lib.dc_mean_f32(_ptr(_chk(x, name="x")), x.numel(), _ptr(out), _stream()), "dc_mean_f32")
    return out


def dropout_mask(out, rate, seed, offset, offset_dev=None):
    """K.dropout(ones, rate): out filled with 1/(1-rate) (kept) or 0, element i a pure function of (i, seed, offset [+ *offset_dev])."""
    lib = _lib.load()
    check(lib.dc_dropout_mask_f32(_ptr(_chk(out, name="out")), out.numel(), float(rate), int(seed) & 0xFFFFFFFF, int(offset) & 0xFFFFFFFF,
                                  None if offset_dev is None else _ptr(_chk(offset_dev, torch.int32, "offset_dev")), _stream()),
          "dc_dropout_mask_f32")
    return out


def bn_fold(gamma, beta, bias, mean, var, scale, shift, eps=1e-3):
    """Fused-epilogue operands of a convolution followed by a frozen-statistics BatchNorm (dc_bn_fold_f32)."""
    lib = _lib.load()
    for t in (gamma, beta, bias, mean, var, scale, shift):
        _chk(t, name="bn_fold operand")
    check(lib.dc_bn_fold_f32(_ptr(gamma), _ptr(beta), _ptr(bias), _ptr(mean), _ptr(var), float(eps), _ptr(scale), _ptr(shift), gamma.numel(), _stream()),
          "dc_bn_fold_f32")


def bn_bwd(dz, a, b, gamma, beta, scale, dacc, dzn):
    """dacc = dz * scale, dzn = dz * (a - b - beta) / gamma over [..., C] tensors (dc_bn_bwd_f32); b may be None."""
    lib = _lib.load()
    for t in (dz, a, gamma, beta, scale, dacc, dzn):
        if not _chk(t, name="bn_bwd operand").is_contiguous():
            raise _lib.DcapError("bn_bwd: operands must be contiguous")
    Cc = dz.shape[-1]
    check(lib.dc_bn_bwd_f32(_ptr(dz), _ptr(a), _ptr(b), _ptr(gamma), _ptr(beta), _ptr(scale), _ptr(dacc), _ptr(dzn), dz.numel() // Cc, Cc, _stream()),
          "dc_bn_bwd_f32")
    return dacc, dzn


def mul(a, b, out):
    lib = _lib.load()
    check(lib.dc_mul_f32(_ptr(_chk(a, name="a")), _ptr(_chk(b, name="b")), _ptr(_chk(out, name="out")), out.numel(), _stream()), "dc_mul_f32")
    return out


def maxpool3x3s2_same_bwd(x, y, dy, out=None):
    lib = _lib.load()
    _chk(x, name="x"), _chk(y, name="y"), _chk(dy, name="dy")
    N, H, W, Cc = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib.dc_maxpool3x3s2_same_bwd_f32(_ptr(x), _ptr(y), _ptr(dy), _ptr(out), N, H, W, Cc, _stream()), "dc_maxpool3x3s2_same_bwd_f32")
    return out


class RegSegmentTable(object):
    """dc_reg_segments on the device: the run-length form of the per-element regulariser coefficient / trainable-mask vectors of a flat
    parameter bucket (coef, mask: host float32 arrays of the bucket's length; mask None = everything trains).  The kernels keep the
    table in LDS: at most MAX_SEGMENTS runs (csrc/loss.hip: kMaxRegSegs); callers with more take the unfused passes."""
    MAX_SEGMENTS = 1024

    def __init__(self, coef, mask, device):
        coef = np.ascontiguousarray(coef, np.float32)
        mask = np.ones_like(coef) if mask is None else np.ascontiguousarray(mask, np.float32)
        n = coef.shape[0]
        cut = np.flatnonzero((coef[1:] != coef[:-1]) | (mask[1:] != mask[:-1])) + 1
        start = np.concatenate([[0], cut, [n]]).astype(np.int32)
        self.n, self.nseg = n, len(start) - 1
        self.start = torch.tensor(start, device=device)
        self.coef = torch.tensor(coef[start[:-1]], device=device)
        self.mask = torch.tensor(mask[start[:-1]], device=device)
        self.c = _lib.RegSegments(self.start.data_ptr(), self.coef.data_ptr(), self.mask.data_ptr(), self.nseg)


def reg_sumsq(w, g, segs, loss=None, gnorm_sq=None):
    """One read-only pass: loss[0] = sum coef w^2, gnorm_sq[0] = sum (g mask + 2 coef w)^2 (dc_reg_sumsq_f32), fixed summation order."""
    lib = _lib.load()
    if segs.n != w.numel() or g.numel() != w.numel():
        raise _lib.DcapError("reg_sumsq: the segment table covers %d elements, the bucket has %d" % (segs.n, w.numel()))
    _launch_ws(lib.dc_reg_sumsq_workspace_bytes(w.numel()), w.device, lib.dc_reg_sumsq_f32, _ptr(_chk(w, name="w")), _ptr(_chk(g, name="g")),
               C.byref(segs.c), w.numel(), None if loss is None else _ptr(loss), None if gnorm_sq is None else _ptr(gnorm_sq))
    return loss, gnorm_sq


def amsgrad_step(p, g, m, v, vhat, lr_t, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0, gnorm_sq=None, clipnorm=0.0, p_bf16=None,
                 lr_t_dev=None, reg=None):
    lib = _lib.load()
    d = AmsgradDesc()
    d.n = p.numel()
    d.p, d.g, d.m, d.v, d.vhat = (_chk(t, name="amsgrad buffer").data_ptr() for t in (p, g, m, v, vhat))
    d.lr_t, d.beta1, d.beta2, d.eps = float(lr_t), float(beta1), float(beta2), float(eps)
    d.grad_scale = float(grad_scale)
    d.gnorm_sq = None if gnorm_sq is None else gnorm_sq.data_ptr()
    d.clipnorm = float(clipnorm or 0.0)
    if p_bf16 is not None:
        d.p_bf16, d.n_bf16 = _chk(p_bf16, BF16, "p_bf16").data_ptr(), p_bf16.numel()
    if lr_t_dev is not None:
        d.lr_t_dev = _chk(lr_t_dev, name="lr_t_dev").data_ptr()
    if reg is not None:                                    # regulariser + trainable mask applied inside the update (RegSegmentTable)
        if reg.n != p.numel():
            raise _lib.DcapError("amsgrad_step: the segment table covers %d elements, the bucket has %d" % (reg.n, p.numel()))
        d.reg = C.pointer(reg.c)
    check(lib.dc_amsgrad_step_f32(C.byref(d), _stream()), "dc_amsgrad_step_f32")


OPTIMIZER_KINDS = {"adam": _lib.OPT_ADAM, "sgd": _lib.OPT_SGD}


def optimizer_step(kind, p, g, state, step, beta1=0.9, beta2=0.999, eps=1e-7, nesterov=False, grad_scale=1.0, gnorm_sq=None, clipnorm=0.0,
                   clipvalue=0.0, p_bf16=None, step_dev=None, reg=None):
    """One fused update of the bucket p from g (dc_optimizer_step_f32).  kind "adam": state = (m, v), step = Keras' lr_t; kind "sgd":
    state = (velocity,), or () with beta1 (the momentum) == 0 -- then nothing but p is written --, step = lr.  gnorm_sq / clipnorm,
    p_bf16, step_dev (a device word that overrides step) and reg (RegSegmentTable) as amsgrad_step takes them; clipvalue clips the
    scaled gradient after the norm clip."""
    lib = _lib.load()
    if kind not in OPTIMIZER_KINDS:
        raise _lib.DcapError("optimizer_step: kind must be one of %s, got %r" % (sorted(OPTIMIZER_KINDS), kind))
    state = tuple(state or ())
    if len(state) > 2:
        raise _lib.DcapError("optimizer_step: at most two state buckets, got %d" % len(state))
    d = _lib.OptimizerDesc()
    d.kind, d.nesterov = OPTIMIZER_KINDS[kind], int(bool(nesterov))
    d.n = p.numel()
    for t in (g,) + state:
        if t.numel() != p.numel():
            raise _lib.DcapError("optimizer_step: a bucket of %d elements beside p's %d" % (t.numel(), p.numel()))
    d.p, d.g = _chk(p, name="optimizer buffer").data_ptr(), _chk(g, name="optimizer buffer").data_ptr()
    ptrs = [_chk(t, name="optimizer state").data_ptr() for t in state] + [None, None]
    d.state0, d.state1 = ptrs[0], ptrs[1]
    d.step, d.beta1, d.beta2, d.eps = float(step), float(beta1), float(beta2), float(eps)
    d.grad_scale = float(grad_scale)
    d.gnorm_sq = None if gnorm_sq is None else gnorm_sq.data_ptr()
    d.clipnorm, d.clipvalue = float(clipnorm or 0.0), float(clipvalue or 0.0)
    if p_bf16 is not None:
        d.p_bf16, d.n_bf16 = _chk(p_bf16, BF16, "p_bf16").data_ptr(), p_bf16.numel()
    if step_dev is not None:
        d.step_dev = _chk(step_dev, name="step_dev").data_ptr()
    if reg is not None:
        if reg.n != p.numel():
            raise _lib.DcapError("optimizer_step: the segment table covers %d elements, the bucket has %d" % (reg.n, p.numel()))
        d.reg = C.pointer(reg.c)
    check(lib.dc_optimizer_step_f32(C.byref(d), _stream()), "dc_optimizer_step_f32")
