"""Operand placement cases: where a pointer, a leading dimension or a width is not "16-byte friendly", the C ABI (include/dcap.h)
either refuses the call with DC_EALIGN before anything is launched or serves it on a scalar / ragged / smaller-tile path.  This module
holds what tests/test_gpu_operand_placement.py (the fallback paths compute the right thing, every refusal refuses) and
tests/test_placement_inventory.py (every DC_EALIGN site of the source has a refusal case) share.  Plain module, no fixtures; torch
and the package are imported inside the functions, so importing it needs neither a GPU nor the built library.

Operands live on binary grids (as _decode_cases._exact_operands: at most 5 significant bits each), so that every product, partial sum
and epilogue value is exact in fp32 -- and in bf16 and the split-bf16 modes -- whatever the summation order: a kernel's output is
compared with the float64 result by equality, no tolerance."""
import re

import numpy as np

DC_EALIGN = -2
GUARD = 64                                   # sentinel elements on either side of a carved view (a multiple of 8: keeps the base rule)
SENTINEL = {"float32": 1.5e30, "bfloat16": -3.0e30, "int32": 0x5A5A5A5A, "int16": 0x5A5A, "uint8": 0xA5, "float64": 1.5e300}


# ---------------------------------------------------------------------------------------------------------------------------------
# exact operands (host, float64)

def grid(rng, shape, step, bound):
    """Multiples of `step` within +-bound, as float64."""
    n = int(round(bound / step))
    return rng.integers(-n, n + 1, shape).astype(np.float64) * step


def assert_exact_f32(a, what):
    """The float64 array survives a round trip through float32 unchanged: the precondition of every equality comparison."""
    a = np.asarray(a, np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a), "%s is not exact in float32" % what
    return a


def epilogue(acc, scale=None, shift=None, residual=None, relu=False, base=None):
    """relu((acc * scale + shift) + residual) + base in float64, every stage checked to be exact in float32.  Each value is a multiple
    of 2^-12 (products 2^-11, scale down to 1/2) and |value| < 2^12 is asserted: 24 significant bits suffice at every stage, in any
    summation order (partial sums of the products are multiples of 2^-11 bounded by the same figure)."""
    v = assert_exact_f32(acc, "the accumulator")
    if scale is not None:
        v = v * scale
    if shift is not None:
        v = v + shift
    v = assert_exact_f32(v, "acc * scale + shift")
    if residual is not None:
        v = assert_exact_f32(v + residual, "... + residual")
    if relu:
        v = np.maximum(v, 0.0)
    if base is not None:
        v = assert_exact_f32(v + base, "... + C0")
    return v


def _bound_ok(K):
    # |acc| <= K / 16, scale <= 2, |shift| <= 1/2, |residual| and |C0| <= 4
    assert 2.0 * K / 16.0 + 0.5 + 4.0 + 4.0 < 2.0 ** 12, "K = %d leaves the exact range" % K


def gemm_case(seed, M, N, K, scale=True, shift=True, residual=None, relu=True, accumulate=True):
    """A [M,K] in steps of 1/8 within +-1, B [K,N] in steps of 1/256 within +-1/16, shift in steps of 1/2048 within +-1/2, scale from
    {0.5, 1, 2}, residual ("full": [M,N]; an integer r: [r,N], row m % r) and the accumulate base C0 in steps of 1/8 within +-4.
    -> dict of float64 arrays (None where absent) with want = relu((A B * scale + shift) + residual) + C0."""
    _bound_ok(K)
    rng = np.random.default_rng(seed)
    c = {"M": M, "N": N, "K": K, "relu": relu}
    c["A"] = grid(rng, (M, K), 1 / 8, 1.0)
    c["B"] = grid(rng, (K, N), 1 / 256, 1 / 16)
    c["scale"] = rng.choice(np.array([0.5, 1.0, 2.0]), N) if scale else None
    c["shift"] = grid(rng, (N,), 1 / 2048, 0.5) if shift else None
    c["res_rows"] = 0
    if residual == "full":
        c["residual"] = grid(rng, (M, N), 1 / 8, 4.0)
        res = c["residual"]
    elif residual:
        assert M % residual == 0
        c["residual"], c["res_rows"] = grid(rng, (int(residual), N), 1 / 8, 4.0), int(residual)
        res = np.tile(c["residual"], (M // residual, 1))
    else:
        c["residual"], res = None, None
    c["C0"] = grid(rng, (M, N), 1 / 8, 4.0) if accumulate else None
    c["want"] = epilogue(c["A"] @ c["B"], c["scale"], c["shift"], res, relu, c["C0"])
    return c


def conv_case(seed, N, H, W, Cin, Cout, kh, stride, res_mode=0, relu=True, scale=True, shift=True):
    """x [N,H,W,Cin] and the HWIO kernel on gemm_case's grids; kh x kh kernel, TF 'SAME' padding for 3 x 3 / stride 1, none for 1 x 1.
    res_mode 1: residual [N,Ho,Wo,Cout]; 2: the 2x coarser map, upsampled by repetition.  -> dict with the packed kernel w [Cout,
    kh*kh*Cin] (cin fastest), Ho, Wo, pad and want = relu((conv * scale + shift) + residual)."""
    from oracle import np_oracle as O
    _bound_ok(kh * kh * Cin)
    rng = np.random.default_rng(seed)
    x = grid(rng, (N, H, W, Cin), 1 / 8, 1.0)
    k = grid(rng, (kh, kh, Cin, Cout), 1 / 256, 1 / 16)
    pad = (kh - 1) // 2
    acc = O.conv2d_nhwc(x, k, stride=stride, padding=(pad, pad, pad, pad))
    Ho, Wo = acc.shape[1], acc.shape[2]
    c = {"x": x, "w": np.transpose(k, (3, 0, 1, 2)).reshape(Cout, kh * kh * Cin), "kh": kh, "stride": stride, "pad": pad, "Ho": Ho, "Wo": Wo,
         "Cout": Cout, "res_mode": res_mode, "relu": relu}
    c["scale"] = rng.choice(np.array([0.5, 1.0, 2.0]), Cout) if scale else None
    c["shift"] = grid(rng, (Cout,), 1 / 2048, 0.5) if shift else None
    if res_mode == 1:
        c["residual"] = grid(rng, (N, Ho, Wo, Cout), 1 / 8, 4.0)
        res = c["residual"]
    elif res_mode == 2:
        assert Ho % 2 == 0 and Wo % 2 == 0
        c["residual"] = grid(rng, (N, Ho // 2, Wo // 2, Cout), 1 / 8, 4.0)
        res = c["residual"].repeat(2, axis=1).repeat(2, axis=2)
    else:
        c["residual"], res = None, None
    c["want"] = epilogue(acc, c["scale"], c["shift"], res, relu)
    return c


def bf16_of(want):
    """The bf16 output copy: round-to-nearest-even of the exact fp32 value (as float64)."""
    from oracle import np_oracle as O
    return O.to_bf16(want)


# ---------------------------------------------------------------------------------------------------------------------------------
# device tensors at chosen places

def _torch():
    import torch
    return torch


def dev(a, dtype=None):
    torch = _torch()
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float32, device="cuda")


def host(t):
    torch = _torch()
    return (t.float() if t.dtype == torch.bfloat16 else t).detach().cpu().numpy().astype(np.float64)


def _dtype_name(dtype):
    return str(dtype).replace("torch.", "")


def _sentinel_buffer(n, dtype):
    torch = _torch()
    buf = torch.empty(n, dtype=dtype, device="cuda")
    buf.fill_(SENTINEL[_dtype_name(dtype)])
    return buf


def carve(t, offset_bytes=0, ld=None):
    """A view with t's values and shape whose data_ptr() lies `offset_bytes` past a 16-byte boundary and, for a 2-D t with ld, whose
    row stride is ld elements -- carved out of a larger sentinel-filled buffer (GUARD elements before and after; the padding columns
    of a strided view hold the sentinel too).  untouched_outside(view) checks that nothing but the view's own elements changed."""
    torch = _torch()
    esz = t.element_size()
    assert offset_bytes % esz == 0 and 0 <= offset_bytes < 16
    off = offset_bytes // esz
    if ld is None:
        span = t.numel()
        size, stride = tuple(t.shape), tuple(t.contiguous().stride()) if t.dim() else ()
    else:
        assert t.dim() == 2 and ld >= t.shape[1]
        span = (t.shape[0] - 1) * ld + t.shape[1]
        size, stride = tuple(t.shape), (ld, 1)
    buf = _sentinel_buffer(GUARD + off + span + GUARD + 16, t.dtype)
    assert buf.data_ptr() % 16 == 0 and (GUARD * esz) % 16 == 0
    view = buf.as_strided(size, stride, GUARD + off)
    view.copy_(t)
    assert view.data_ptr() % 16 == offset_bytes and tuple(view.shape) == tuple(t.shape)
    view._placement_base = buf
    return view


def misplaced(t, floats=1, elems=None):
    """carve() with the base 4 bytes per float past a 16-byte boundary (`elems`: that many ELEMENTS past it instead -- a bf16 tensor on
    a 2-byte boundary is misplaced(t, elems=1))."""
    return carve(t, 4 * floats if elems is None else elems * t.element_size())


def restride(t, ld, floats=0):
    """carve() of a 2-D t with row stride ld (and the base `floats` * 4 bytes past a 16-byte boundary)."""
    return carve(t, 4 * floats, ld)


def sentinel_like(shape, dtype=None):
    torch = _torch()
    dtype = dtype or torch.float32
    return _sentinel_buffer(int(np.prod(shape)), dtype).view(*shape)


def _bits(t):
    torch = _torch()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def untouched_outside(view):
    """True when every element of the carved buffer outside `view` still holds the sentinel."""
    buf = view._placement_base
    snap = buf.clone()
    snap.as_strided(tuple(view.shape), tuple(view.stride()), view.storage_offset() - buf.storage_offset()).fill_(SENTINEL[_dtype_name(buf.dtype)])
    return bool(_torch().equal(_bits(snap), _bits(_sentinel_buffer(buf.numel(), buf.dtype))))


# ---------------------------------------------------------------------------------------------------------------------------------
# the refusals: one entry per DC_EALIGN message literal of csrc/*.hip and *.h, each with the calls that provoke it

def literal_regex(literal):
    """The message literal as a pattern for dc_last_error(): printf conversions are wildcards, %% is a per-cent sign."""
    out, pos = [], 0
    for m in re.finditer(r"%(?:%|[-+ #0]*\d*(?:\.\d+)?(?:hh|h|ll|l|z|j|t)?[diouxXeEfgGcsp])", literal):
        out.append(re.escape(literal[pos:m.start()]))
        out.append("%" if m.group(0) == "%%" else ".*")
        pos = m.end()
    out.append(re.escape(literal[pos:]))
    return re.compile("".join(out), re.S)


class Harness(object):
    """What a refusal case builds its one offending call from: valid small operands, outputs whose bytes are recorded before the call
    (watch) and compared after it (unchanged), and the two ways to call -- an ops wrapper, or the C entry point through ctypes, both
    raising DcapError with the code and dc_last_error()'s text."""

    def __init__(self, ops, lib):
        import ctypes
        import torch
        from image_captioning_amd import _lib
        self.ops, self.lib, self.L, self.C, self.torch = ops, lib, _lib, ctypes, torch
        self.watched = []
        self.who = None               # set by a case: the prefix its refusal's message must carry
        self._workspace = None

    # inputs: zeros of the right shape (a refused call reads nothing)
    def zeros(self, *shape, dtype=None):
        return self.torch.zeros(shape, dtype=dtype or self.torch.float32, device="cuda")

    def bf16(self, *shape):
        return self.zeros(*shape, dtype=self.torch.bfloat16)

    def i32(self, *shape):
        return self.zeros(*shape, dtype=self.torch.int32)

    def off(self, t, nbytes=4):
        """t's copy `nbytes` past a 16-byte boundary."""
        return carve(t, nbytes)

    def strided(self, rows, cols, ld, dtype=None):
        return carve(self.zeros(rows, cols, dtype=dtype), 0, ld)

    # outputs: sentinel-filled, watched
    def out(self, *shape, dtype=None, nbytes=0, ld=None):
        t = carve(sentinel_like(shape, dtype), nbytes, ld)
        self.watched.append((t._placement_base, _bits(t._placement_base).clone()))
        return t

    def watch(self, t):
        """An in / out operand (or one the entry point would otherwise fill): must keep its bytes."""
        self.watched.append((t, _bits(t.contiguous()).clone()))
        return t

    def unchanged(self):
        self.torch.cuda.synchronize()
        return all(self.torch.equal(_bits(t.contiguous()), before) for t, before in self.watched)

    def stream(self):
        return self.C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def raw(self, name, *args):
        """lib.<name>(*args); tensors pass as their device pointers."""
        conv = [self.C.c_void_p(a.data_ptr()) if isinstance(a, self.torch.Tensor) else a for a in args]
        self.L.check(getattr(self.lib, name)(*conv), name)

    def workspace(self, nbytes):
        ws, wsb = self.ops.WORKSPACE.get(max(int(nbytes), 1), "cuda")
        return ws, wsb

    def misplace_workspace(self, who=None):
        """From here on the ops wrappers get their scratch buffers 4 bytes past a 16-byte boundary (sentinel-filled, watched) instead of
        ops.WORKSPACE's; restore() puts ops.WORKSPACE back.  who: the prefix dc_last_error() must carry (which launcher refused)."""
        harness = self

        class _Misplaced(object):
            def get(self, nbytes, device):
                if nbytes == 0:
                    return None, 0
                return harness.out(int(nbytes), dtype=harness.torch.uint8, nbytes=4), int(nbytes)

        if self._workspace is None:
            self._workspace = self.ops.WORKSPACE
        self.ops.WORKSPACE = _Misplaced()
        self.who = who

    def restore(self):
        if self._workspace is not None:
            self.ops.WORKSPACE, self._workspace = self._workspace, None


REFUSALS = []          # (message literal exactly as in the source, case id, callable(h: Harness) making the one offending call)


def refusal(literal, case_id):
    def deco(fn):
        REFUSALS.append((literal, case_id, fn))
        return fn
    return deco


# --- dc_gemm_f32 -------------------------------------------------------------------------------------------------------------------
_GEMM_F32 = "dc_gemm_f32: A/B must be 16-byte aligned with lda, ldb multiples of 4"


@refusal(_GEMM_F32, "gemm_f32-A+4")
def _(h):
    h.ops.gemm(h.off(h.zeros(8, 32)), h.zeros(32, 8), out=h.out(8, 8))


@refusal(_GEMM_F32, "gemm_f32-B+4")
def _(h):
    h.ops.gemm(h.zeros(8, 32), h.off(h.zeros(32, 8)), out=h.out(8, 8))


@refusal(_GEMM_F32, "gemm_f32-lda34")
def _(h):
    h.ops.gemm(h.strided(8, 32, 34), h.zeros(32, 8), out=h.out(8, 8))


@refusal(_GEMM_F32, "gemm_f32-ldb10")
def _(h):
    h.ops.gemm(h.zeros(8, 32), h.strided(32, 8, 10), out=h.out(8, 8))


# every split-K launcher refuses a workspace off the 16-byte boundary when its slab stores are 16 bytes wide (N % 4 == 0); the message
# names the launcher
_SLABS = "%s: the workspace must be 16-byte aligned when N is a multiple of 4"


@refusal(_SLABS, "splitk-workspace+4-gemm_f32")
def _(h):
    d = h.L.GemmDesc()
    A, B, out = h.zeros(8, 128), h.zeros(128, 8), h.out(8, 8)
    d.M, d.N, d.K, d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.split_k = 8, 8, 128, A.data_ptr(), 128, B.data_ptr(), 8, out.data_ptr(), 8, 2
    need = h.lib.dc_gemm_workspace_bytes(h.C.byref(d))
    assert need == 2 * 8 * 8 * 4
    ws = h.out(need, dtype=h.torch.uint8, nbytes=4)
    h.who = "igemm split-K"
    h.raw("dc_gemm_f32", h.C.byref(d), ws, need, h.stream())


@refusal(_SLABS, "splitk-workspace+4-gemm_bf16-tile128")
def _(h):
    h.misplace_workspace("bgemm split-K")
    info = {}
    try:
        h.ops.gemm_bf16(h.bf16(16, 128), h.bf16(128, 16), out=h.out(16, 16), split_k=2, info=info)
    finally:
        assert info == {"tile": 128, "split_k": 2}, info


@refusal(_SLABS, "splitk-workspace+4-gemm_bf16-tile256")
def _(h):
    h.misplace_workspace("bgemm256 split-K")
    info = {}
    try:
        h.ops.gemm_bf16(h.bf16(512, 2112), h.bf16(512, 2112), b_trans=True, out=h.out(512, 512), split_k=33, info=info)
    finally:
        assert info == {"tile": 256, "split_k": 33}, info


@refusal(_SLABS, "splitk-workspace+4-conv2d-bf16x3")
def _(h):
    h.misplace_workspace("igemm_bs split-K")
    h.ops.conv2d(h.zeros(1, 8, 8, 64), h.zeros(64, 64), 1, 1, 1, 0, 0, 8, 8, out=h.out(1, 8, 8, 64), split_k=2, math=1)


@refusal(_SLABS, "splitk-workspace+4-conv2d-f32")
def _(h):
    h.misplace_workspace("igemm split-K")
    h.ops.conv2d(h.zeros(1, 8, 8, 64), h.zeros(32, 64), 1, 1, 1, 0, 0, 8, 8, out=h.out(1, 8, 8, 32), split_k=2)


@refusal(_SLABS, "splitk-workspace+4-conv2d_bf16")
def _(h):
    h.misplace_workspace("dc_conv2d_bf16 split-K")
    info = {}
    try:
        h.ops.conv2d_bf16(h.bf16(1, 8, 8, 128), h.bf16(64, 128), 1, 1, 1, 0, 0, 8, 8, out=h.out(1, 8, 8, 64), split_k=2, tile=128, info=info)
    finally:
        assert info == {"tile": 128, "split_k": 2}, info


@refusal(_SLABS, "splitk-workspace+4-conv2d_wgrad_bf16")
def _(h):
    h.misplace_workspace("dc_conv2d_wgrad_bf16 split-K")
    h.ops.conv2d_wgrad_bf16(h.bf16(1, 8, 16, 128), h.bf16(1, 8, 16, 8), 1, 1, 1, 0, 0, out=h.out(8, 128), split_k=2)


@refusal(_SLABS, "splitk-workspace+4-conv2d_wgrad_f32")
def _(h):
    h.misplace_workspace("igemm split-K")
    h.ops.conv2d_wgrad(h.zeros(1, 8, 16, 64), h.zeros(1, 8, 16, 4), 1, 1, 1, 0, 0, out=h.out(4, 64), split_k=2)


# --- dc_gemm_bf16 ------------------------------------------------------------------------------------------------------------------
_GEMM_BF16 = "dc_gemm_bf16: K, lda, ldb must be multiples of 8 (16-byte chunks) and A, B 16-byte aligned"
_GEMM_BF16_ROW = "dc_gemm_bf16: a K-major operand needs its row length (M for A^T, N for B) to be a multiple of 8"


@refusal(_GEMM_BF16, "gemm_bf16-A+4")
def _(h):
    h.ops.gemm_bf16(h.off(h.bf16(16, 64)), h.bf16(64, 16), out=h.out(16, 16))


@refusal(_GEMM_BF16, "gemm_bf16-B+8")
def _(h):
    h.ops.gemm_bf16(h.bf16(16, 64), h.off(h.bf16(64, 16), 8), out=h.out(16, 16))


@refusal(_GEMM_BF16, "gemm_bf16-K60")
def _(h):
    h.ops.gemm_bf16(h.strided(16, 60, 64, h.torch.bfloat16), h.strided(60, 16, 16, h.torch.bfloat16), out=h.out(16, 16))


@refusal(_GEMM_BF16, "gemm_bf16-lda68")
def _(h):
    h.ops.gemm_bf16(h.strided(16, 64, 68, h.torch.bfloat16), h.bf16(64, 16), out=h.out(16, 16))


@refusal(_GEMM_BF16_ROW, "gemm_bf16-N12")
def _(h):
    h.ops.gemm_bf16(h.bf16(16, 64), h.strided(64, 12, 16, h.torch.bfloat16), out=h.out(16, 12))


@refusal(_GEMM_BF16_ROW, "gemm_bf16-At-M12")
def _(h):
    h.ops.gemm_bf16(h.strided(64, 12, 16, h.torch.bfloat16), h.bf16(64, 16), a_trans=True, out=h.out(12, 16))


# --- convolutions ------------------------------------------------------------------------------------------------------------------
_CONV = "dc_conv2d: x and w must be 16-byte aligned"


@refusal(_CONV, "conv2d-x+4")
def _(h):
    h.ops.conv2d(h.off(h.zeros(1, 4, 4, 32)), h.zeros(32, 32), 1, 1, 1, 0, 0, 4, 4, out=h.out(1, 4, 4, 32))


@refusal(_CONV, "conv2d-w+4")
def _(h):
    h.ops.conv2d(h.zeros(1, 4, 4, 32), h.off(h.zeros(32, 32)), 1, 1, 1, 0, 0, 4, 4, out=h.out(1, 4, 4, 32))


@refusal(_CONV, "conv2d-bf16x3-x+4")
def _(h):
    h.ops.conv2d(h.off(h.zeros(1, 4, 4, 32)), h.zeros(32, 32), 1, 1, 1, 0, 0, 4, 4, out=h.out(1, 4, 4, 32), math=1)


_CONV_BF16 = "dc_conv2d_bf16: x, w, y, y_bf16 must be 16-byte aligned"


@refusal(_CONV_BF16, "conv2d_bf16-x+4")
def _(h):
    h.ops.conv2d_bf16(h.off(h.bf16(1, 4, 4, 64)), h.bf16(64, 64), 1, 1, 1, 0, 0, 4, 4, out=h.out(1, 4, 4, 64))


@refusal(_CONV_BF16, "conv2d_bf16-y+4")
def _(h):
    h.ops.conv2d_bf16(h.bf16(1, 4, 4, 64), h.bf16(64, 64), 1, 1, 1, 0, 0, 4, 4, out=h.out(1, 4, 4, 64, nbytes=4))


@refusal(_CONV_BF16, "conv2d_bf16-y_bf16+2")
def _(h):
    h.ops.conv2d_bf16(h.bf16(1, 4, 4, 64), h.bf16(64, 64), 1, 1, 1, 0, 0, 4, 4, out=h.out(1, 4, 4, 64),
                      out_bf16=h.out(1, 4, 4, 64, dtype=h.torch.bfloat16, nbytes=2))


@refusal("dc_conv2d_wgrad: pointers must be 16-byte aligned", "conv2d_wgrad-dy+4")
def _(h):
    h.ops.conv2d_wgrad(h.zeros(1, 4, 4, 64), h.off(h.zeros(1, 4, 4, 4)), 1, 1, 1, 0, 0, out=h.out(4, 64))


@refusal("dc_conv2d_wgrad: pointers must be 16-byte aligned", "conv2d_wgrad-dw+4")
def _(h):
    h.ops.conv2d_wgrad(h.zeros(1, 4, 4, 64), h.zeros(1, 4, 4, 4), 1, 1, 1, 0, 0, out=h.out(4, 64, nbytes=4))


@refusal("dc_conv2d_wgrad_bf16: pointers must be 16-byte aligned", "conv2d_wgrad_bf16-x+4")
def _(h):
    h.ops.conv2d_wgrad_bf16(h.off(h.bf16(1, 4, 4, 128)), h.bf16(1, 4, 4, 8), 1, 1, 1, 0, 0, out=h.out(8, 128))


@refusal("dc_conv2d_wgrad_bf16: pointers must be 16-byte aligned", "conv2d_wgrad_bf16-dw+4")
def _(h):
    h.ops.conv2d_wgrad_bf16(h.bf16(1, 4, 4, 128), h.bf16(1, 4, 4, 8), 1, 1, 1, 0, 0, out=h.out(8, 128, nbytes=4))


@refusal("dc_pw_chain_pack: out must be 16-byte aligned", "pw_chain_pack-out+4")
def _(h):
    h.ops.pw_chain_pack(h.zeros(32, 8), out=h.out(32, 8, nbytes=4))


@refusal("dc_pw_chain_pack_b3: out must be 16-byte aligned", "pw_chain_pack_b3-out+4")
def _(h):
    h.ops.pw_chain_pack_b3(h.zeros(32, 16), out=h.out(32, 48, dtype=h.torch.int16, nbytes=4))


def _pw_chain(h, **moved):
    """The 64 -> 256 -> 64 seam on four pixels; moved: operand name -> byte offset."""
    t = {"x": h.zeros(4, 64), "w1": h.zeros(256, 64), "shift1": h.zeros(256), "w2": h.zeros(64, 256), "shift2": h.zeros(64),
         "scale1": h.zeros(256), "residual": h.zeros(4, 256)}
    for name, nbytes in moved.items():
        if name in t:
            t[name] = h.off(t[name], nbytes)
    y, z = h.out(4, 256, nbytes=moved.get("y", 0)), h.out(4, 64, nbytes=moved.get("z", 0))
    h.ops.pw_chain(t["x"], t["w1"], t["shift1"], t["w2"], t["shift2"], scale1=t["scale1"], residual=t["residual"], y=y, z=z)


for _name in ("x", "w1", "shift1", "w2", "shift2", "scale1", "residual", "y", "z"):
    refusal("dc_pw_chain: every pointer must be 16-byte aligned", "pw_chain-%s+4" % _name)(lambda h, _n=_name: _pw_chain(h, **{_n: 4}))


@refusal("dc_conv2d_winograd_pack: u must be 16-byte aligned", "winograd_pack-u+4")
def _(h):
    h.ops.winograd_pack(h.zeros(32, 9 * 32), 32, 32, out=h.out(16 * 32 * 32, nbytes=4))


@refusal("dc_conv2d_winograd_pack_b3: u must be 16-byte aligned", "winograd_pack_b3-u+4")
def _(h):
    h.ops.winograd_pack_b3(h.zeros(32, 9 * 32), 32, 32, out=h.out(48 * 32 * 32, dtype=h.torch.int16, nbytes=4))


# --- the bandwidth kernels of conv.hip / proposal.hip ---------------------------------------------------------------------------------
@refusal("dc_scatter2_add: pointers must be 16-byte aligned", "scatter2_add-coarse+4")
def _(h):
    h.ops.scatter2_add(h.off(h.zeros(1, 2, 2, 4)), h.out(1, 4, 4, 4))


@refusal("dc_scatter2_add: pointers must be 16-byte aligned", "scatter2_add-fine+4")
def _(h):
    h.ops.scatter2_add(h.zeros(1, 2, 2, 4), h.out(1, 4, 4, 4, nbytes=4))


_DOWN = "dc_downsample2x_sum: pointers must be 16-byte aligned (out_bf16: 8)"


@refusal(_DOWN, "downsample2x_sum-fine+4")
def _(h):
    h.ops.downsample2x_sum(h.off(h.zeros(1, 4, 4, 4)), out=h.out(1, 2, 2, 4))


@refusal(_DOWN, "downsample2x_sum-out_bf16+2")
def _(h):
    h.ops.downsample2x_sum(h.zeros(1, 4, 4, 4), out=h.out(1, 2, 2, 4), out_bf16=h.out(1, 2, 2, 4, dtype=h.torch.bfloat16, nbytes=2))


@refusal(_DOWN, "downsample2x_sum-out_bf16+4")
def _(h):
    h.ops.downsample2x_sum(h.zeros(1, 4, 4, 4), out=h.out(1, 2, 2, 4), out_bf16=h.out(1, 2, 2, 4, dtype=h.torch.bfloat16, nbytes=4))


@refusal("dc_maxpool3x3s2: pointers must be 16-byte aligned", "maxpool3x3s2-x+4")
def _(h):
    h.ops.maxpool3x3s2_same(h.off(h.zeros(1, 4, 4, 4)), out=h.out(1, 2, 2, 4))


@refusal("dc_maxpool3x3s2: pointers must be 16-byte aligned", "maxpool3x3s2-y+4")
def _(h):
    h.ops.maxpool3x3s2_same(h.zeros(1, 4, 4, 4), out=h.out(1, 2, 2, 4, nbytes=4))


@refusal("dc_maxpool2x2s2: pointers must be 16-byte aligned", "maxpool2x2s2-x+4")
def _(h):
    h.ops.maxpool2x2s2(h.off(h.zeros(1, 4, 4, 4)), out=h.out(1, 2, 2, 4))


@refusal("dc_maxpool2x2s2: pointers must be 16-byte aligned", "maxpool2x2s2-y+4")
def _(h):
    h.ops.maxpool2x2s2(h.zeros(1, 4, 4, 4), out=h.out(1, 2, 2, 4, nbytes=4))


@refusal("dc_mold_image: out must be 16-byte aligned", "mold_image-out+4")
def _(h):
    h.ops.mold_image_rgbx(h.zeros(1, 4, 4, 3, dtype=h.torch.uint8), (1.0, 2.0, 3.0), out=h.out(1, 4, 4, 4, nbytes=4))


@refusal("dc_mold_image_padded: out must be 16-byte aligned", "mold_image_padded-out+4")
def _(h):
    h.ops.mold_image_padded(h.zeros(1, 4, 4, 3, dtype=h.torch.uint8), (1.0, 2.0, 3.0), h.out(1, 4, 4, 8, nbytes=4))


@refusal("dc_subsample2: pointers must be 16-byte aligned", "subsample2-x+4")
def _(h):
    h.ops.subsample2(h.off(h.zeros(1, 4, 4, 4)), out=h.out(1, 2, 2, 4))


@refusal("dc_subsample2: pointers must be 16-byte aligned", "subsample2-y+4")
def _(h):
    h.ops.subsample2(h.zeros(1, 4, 4, 4), out=h.out(1, 2, 2, 4, nbytes=4))


# --- casts ---------------------------------------------------------------------------------------------------------------------------
_CAST = "dc_cast_f32_bf16: x 16-byte, out 8-byte aligned"
_UNCAST = "dc_cast_bf16_f32: out 16-byte, x 8-byte aligned"


@refusal(_CAST, "cast_f32_bf16-x+4")
def _(h):
    h.ops.to_bf16(h.off(h.zeros(64)), out=h.out(64, dtype=h.torch.bfloat16))


@refusal(_CAST, "cast_f32_bf16-out+4")
def _(h):
    h.ops.to_bf16(h.zeros(64), out=h.out(64, dtype=h.torch.bfloat16, nbytes=4))


@refusal(_CAST, "cast_f32_bf16-out+2")
def _(h):
    h.ops.to_bf16(h.zeros(64), out=h.out(64, dtype=h.torch.bfloat16, nbytes=2))


@refusal(_UNCAST, "cast_bf16_f32-x+4")
def _(h):
    h.ops.from_bf16(h.off(h.bf16(64), 4), h.out(64))


@refusal(_UNCAST, "cast_bf16_f32-out+4")
def _(h):
    h.ops.from_bf16(h.bf16(64), h.out(64, nbytes=4))


# --- RoIAlign ------------------------------------------------------------------------------------------------------------------------
def _roi_maps(h, moved=None, out=False):
    hw = ((8, 8), (4, 4), (2, 2), (1, 1))
    maps = []
    for i, (a, b) in enumerate(hw):
        nbytes = 4 if moved == i else 0
        maps.append(h.out(1, a, b, 4, nbytes=nbytes) if out else h.off(h.zeros(1, a, b, 4), nbytes))
    return maps


@refusal("dc_roi_align_pyramid: feature map %d not 16-byte aligned", "roi_align-map2+4")
def _(h):
    h.ops.roi_align_pyramid(_roi_maps(h, moved=2), h.zeros(1, 2, 4), 64.0, pool=2, out=h.out(1, 2, 2, 2, 4))


@refusal("dc_roi_align_pyramid: boxes/out not 16-byte aligned", "roi_align-boxes+4")
def _(h):
    h.ops.roi_align_pyramid(_roi_maps(h), h.off(h.zeros(1, 2, 4)), 64.0, pool=2, out=h.out(1, 2, 2, 2, 4))


@refusal("dc_roi_align_pyramid: boxes/out not 16-byte aligned", "roi_align-out+4")
def _(h):
    h.ops.roi_align_pyramid(_roi_maps(h), h.zeros(1, 2, 4), 64.0, pool=2, out=h.out(1, 2, 2, 2, 4, nbytes=4))


@refusal("dc_roi_align_pyramid_bwd: gradient map %d not 16-byte aligned", "roi_align_bwd-map0+4")
def _(h):
    h.ops.roi_align_pyramid_bwd(_roi_maps(h, moved=0, out=True), h.zeros(1, 2, 4), 64.0, h.zeros(1, 2, 2, 2, 4), pool=2)


@refusal("dc_roi_align_pyramid_bwd: boxes / dout not 16-byte aligned", "roi_align_bwd-dout+4")
def _(h):
    h.ops.roi_align_pyramid_bwd(_roi_maps(h, out=True), h.zeros(1, 2, 4), 64.0, h.off(h.zeros(1, 2, 2, 2, 4)), pool=2)


@refusal("dc_roi_tile_groups: boxes not 16-byte aligned", "roi_tile_groups-boxes+4")
def _(h):
    groups = h.ops.RoiTileGroups(1, ((16, 16), (8, 8), (4, 4), (2, 2)), "cuda")
    for t in groups.lists + [groups.counts, groups.marks]:
        h.watch(t)
    h.ops.roi_tile_groups(h.off(h.zeros(1, 2, 4)), groups, 64.0 * 64.0, pool=2)


# --- proposals, refinement, detection targets ---------------------------------------------------------------------------------------
def _proposals(h, anchors_bytes=0, out_bytes=0):
    heads = [h.zeros(1, 2, 2, 18)]
    anchors = h.off(h.zeros(12, 4), anchors_bytes)
    h.ops.rpn_proposals(heads, anchors, (32, 32), 4, 0.7, pre_nms_limit=8, out=h.out(1, 4, 4, nbytes=out_bytes))


refusal("dc_proposals: anchors/proposals must be 16-byte aligned", "proposals-anchors+4")(lambda h: _proposals(h, anchors_bytes=4))
refusal("dc_proposals: anchors/proposals must be 16-byte aligned", "proposals-out+4")(lambda h: _proposals(h, out_bytes=4))


def _refine(h, boxes_bytes=0, scores_bytes=0, consts_bytes=0):
    d = h.L.RefineDesc()
    rois, cap = h.zeros(1, 4, 4), h.zeros(4)
    # (the float64 operands as float32 words of the same bytes: an 8-byte site moved by 4 is no float64 view torch can make)
    consts = h.off(h.zeros(1, 2 * h.L.REFINE_CONSTS), consts_bytes)
    boxes, keep, count = h.out(1, 2, 4, dtype=h.torch.int32, nbytes=boxes_bytes), h.out(1, 2, dtype=h.torch.int32), h.out(1, dtype=h.torch.int32)
    scores = h.out(1, 2 * 4, nbytes=scores_bytes)
    d.B, d.N, d.rois, d.caption_scores, d.caption_stride, d.image_consts = 1, 4, rois.data_ptr(), cap.data_ptr(), 1, consts.data_ptr()
    d.threshold, d.max_instances = 0.5, 2
    d.boxes_out, d.keep_out, d.count_out, d.scores_out = boxes.data_ptr(), keep.data_ptr(), count.data_ptr(), scores.data_ptr()
    ws, wsb = h.workspace(1 << 16)
    h.raw("dc_refine_generations_f64", h.C.byref(d), ws, wsb, h.stream())


_REFINE = "dc_refine_generations: boxes_out must be 16-byte, scores_out / image_consts 8-byte aligned"
refusal(_REFINE, "refine-boxes_out+4")(lambda h: _refine(h, boxes_bytes=4))
refusal(_REFINE, "refine-scores_out+4")(lambda h: _refine(h, scores_bytes=4))
refusal(_REFINE, "refine-image_consts+4")(lambda h: _refine(h, consts_bytes=4))


def _detection_targets(h, prop_bytes=0, gt_bytes=0, rois_bytes=0):
    out = (h.out(4, 4, nbytes=rois_bytes), h.out(4, 3, dtype=h.torch.int32), h.out(2, dtype=h.torch.int32))
    h.ops.detection_targets(h.off(h.zeros(4, 4), prop_bytes), h.off(h.zeros(2, 4), gt_bytes), h.i32(2, 3), 4, 0.5, out=out)


_DT = "dc_detection_targets: boxes must be 16-byte aligned"
refusal(_DT, "detection_targets-proposals+4")(lambda h: _detection_targets(h, prop_bytes=4))
refusal(_DT, "detection_targets-gt_boxes+4")(lambda h: _detection_targets(h, gt_bytes=4))
refusal(_DT, "detection_targets-rois+4")(lambda h: _detection_targets(h, rois_bytes=4))


# --- losses, gradients, optimiser ------------------------------------------------------------------------------------------------------
_SOFTMAX = "dc_softmax_ce: rows must be 16-byte aligned when ld %% 4 == 0"


@refusal(_SOFTMAX, "softmax_ce-logits+4")
def _(h):
    h.ops.softmax_ce(h.off(h.zeros(4, 8)), h.i32(4), probs=h.out(4, 8), loss_rows=h.out(4))


@refusal(_SOFTMAX, "softmax_ce-probs+4")
def _(h):
    h.ops.softmax_ce(h.zeros(4, 8), h.i32(4), probs=h.out(4, 8, nbytes=4), loss_rows=h.out(4))


@refusal(_SOFTMAX, "softmax_ce-dlogits+8")
def _(h):
    h.ops.softmax_ce(h.zeros(4, 8), h.i32(4), dlogits=h.out(4, 8, nbytes=8), loss_rows=h.out(4))


_GATHER = "dc_gather_rows: width/ld must be multiples of 4 and pointers 16-byte aligned"


@refusal(_GATHER, "gather_rows-src+4")
def _(h):
    h.ops.gather_rows(h.off(h.zeros(8, 8)), h.i32(4), h.out(4, 8))


@refusal(_GATHER, "gather_rows-out+4")
def _(h):
    h.ops.gather_rows(h.zeros(8, 8), h.i32(4), h.out(4, 8, nbytes=4))


@refusal(_GATHER, "gather_rows-width6")
def _(h):
    h.ops.gather_rows(h.zeros(8, 8), h.i32(4), h.out(4, 6, ld=8))


@refusal(_GATHER, "gather_rows-ld_out10")
def _(h):
    h.ops.gather_rows(h.zeros(8, 8), h.i32(4), h.out(4, 8, ld=10))


_RELU_DUAL = "dc_relu_bwd_dual: dy, y, out must be 16-byte aligned, out_bf16 8-byte aligned"


@refusal(_RELU_DUAL, "relu_bwd_dual-dy+4")
def _(h):
    h.ops.relu_bwd(h.off(h.zeros(4, 8)), h.zeros(4, 8), h.out(4, 8), out_bf16=h.out(4, 8, dtype=h.torch.bfloat16))


@refusal(_RELU_DUAL, "relu_bwd_dual-out_bf16+2")
def _(h):
    h.ops.relu_bwd(h.zeros(4, 8), h.zeros(4, 8), h.out(4, 8), out_bf16=h.out(4, 8, dtype=h.torch.bfloat16, nbytes=2))


@refusal(_RELU_DUAL, "relu_bwd_dual-out_bf16+4")
def _(h):
    h.ops.relu_bwd(h.zeros(4, 8), h.zeros(4, 8), h.out(4, 8), out_bf16=h.out(4, 8, dtype=h.torch.bfloat16, nbytes=4))


@refusal("dc_sumsq: x must be 16-byte aligned", "sumsq-x+4")
def _(h):
    h.ops.sumsq(h.off(h.zeros(64)), out=h.out(1))


@refusal("dc_reg_sumsq: w and g must be 16-byte aligned", "reg_sumsq-g+4")
def _(h):
    segs = h.ops.RegSegmentTable(np.zeros(64, np.float32), None, "cuda")
    h.ops.reg_sumsq(h.zeros(64), h.off(h.zeros(64)), segs, loss=h.out(1), gnorm_sq=h.out(1))


def _bn_bwd(h, moved):
    t = {"dz": h.zeros(4, 8), "a": h.zeros(4, 8), "b": h.zeros(4, 8), "gamma": h.zeros(8), "beta": h.zeros(8), "scale": h.zeros(8)}
    if moved in t:
        t[moved] = h.off(t[moved])
    dacc, dzn = h.out(4, 8, nbytes=4 if moved == "dacc" else 0), h.out(4, 8, nbytes=4 if moved == "dzn" else 0)
    h.ops.bn_bwd(t["dz"], t["a"], t["b"], t["gamma"], t["beta"], t["scale"], dacc, dzn)


for _name in ("dz", "a", "b", "gamma", "beta", "scale", "dacc", "dzn"):
    refusal("dc_bn_bwd: pointers must be 16-byte aligned", "bn_bwd-%s+4" % _name)(lambda h, _n=_name: _bn_bwd(h, _n))


def _amsgrad(h, moved):
    t = {n: (h.out(64, nbytes=4 if moved == n else 0)) for n in ("p", "m", "v", "vhat")}
    g = h.off(h.zeros(64), 4 if moved == "g" else 0)
    h.ops.amsgrad_step(t["p"], g, t["m"], t["v"], t["vhat"], 0.1)


for _name in ("p", "g", "m", "v", "vhat"):
    refusal("dc_amsgrad_step: buffers must be 16-byte aligned", "amsgrad-%s+4" % _name)(lambda h, _n=_name: _amsgrad(h, _n))


# --- fused vocabulary kernels ----------------------------------------------------------------------------------------------------------
def _vocab_ce(h, bf=False, K=32, V=8, ldx=None, ldw=None, x_bytes=0, w_bytes=0, bias_bytes=0, dl=None, dl_bytes=0, lddl=None):
    dt = h.torch.bfloat16 if bf else h.torch.float32
    X = carve(h.zeros(4, K, dtype=dt), x_bytes, ldx)
    W = carve(h.zeros(K, V, dtype=dt), w_bytes, ldw)
    bias = h.off(h.zeros(V), bias_bytes)
    dlogits = None if dl is None else h.out(4, V, dtype=dl, nbytes=dl_bytes, ld=lddl)
    h.ops.vocab_ce(X, W, bias, h.i32(4), loss_rows=h.out(4), dlogits=dlogits)


_CE = "dc_vocab_ce: X, W, bias must be 16-byte aligned"
refusal(_CE, "vocab_ce-X+4")(lambda h: _vocab_ce(h, x_bytes=4))
refusal(_CE, "vocab_ce-W+4")(lambda h: _vocab_ce(h, w_bytes=4))
refusal(_CE, "vocab_ce-bias+4")(lambda h: _vocab_ce(h, bias_bytes=4))
refusal(_CE, "vocab_ce-bf16-X+4")(lambda h: _vocab_ce(h, bf=True, x_bytes=4))
_CE_BF = "dc_vocab_ce (bf16): K, V, ldx, ldw must be multiples of 8"
refusal(_CE_BF, "vocab_ce-bf16-V12")(lambda h: _vocab_ce(h, bf=True, V=12, ldw=16))
refusal(_CE_BF, "vocab_ce-bf16-ldx36")(lambda h: _vocab_ce(h, bf=True, ldx=36))
_CE_F32 = "dc_vocab_ce (f32): K must be a multiple of 32 and V, ldx, ldw multiples of 4"
refusal(_CE_F32, "vocab_ce-f32-K40")(lambda h: _vocab_ce(h, K=40))
refusal(_CE_F32, "vocab_ce-f32-V6")(lambda h: _vocab_ce(h, V=6, ldw=8))
refusal(_CE_F32, "vocab_ce-f32-ldw10")(lambda h: _vocab_ce(h, ldw=10))
_CE_DL = "dc_vocab_ce: dlogits rows must be 16-byte (fp32) / 8-byte (bf16) aligned, lddl a multiple of 4"


@refusal(_CE_DL, "vocab_ce-dlogits-f32+4")
def _(h):
    _vocab_ce(h, dl=h.torch.float32, dl_bytes=4)


@refusal(_CE_DL, "vocab_ce-dlogits-f32+8")
def _(h):
    _vocab_ce(h, dl=h.torch.float32, dl_bytes=8)


@refusal(_CE_DL, "vocab_ce-dlogits-f32-lddl10")
def _(h):
    _vocab_ce(h, dl=h.torch.float32, lddl=10)


@refusal(_CE_DL, "vocab_ce-dlogits-bf16+2")
def _(h):
    _vocab_ce(h, bf=True, dl=h.torch.bfloat16, dl_bytes=2)


@refusal(_CE_DL, "vocab_ce-dlogits-bf16+4")
def _(h):
    _vocab_ce(h, bf=True, dl=h.torch.bfloat16, dl_bytes=4)


@refusal(_CE_DL, "vocab_ce-dlogits-bf16-lddl10")
def _(h):
    _vocab_ce(h, bf=True, dl=h.torch.bfloat16, lddl=10)


def _vocab_topk(h, bf=False, ldx=None, ldw=None, x_bytes=0, w_bytes=0, bias_bytes=0):
    """dc_vocab_topk_f32 / _bf16 through the descriptor (the ops wrapper copies a misplaced operand to a fresh buffer first)."""
    dt = h.torch.bfloat16 if bf else h.torch.float32
    M, K, V, k = 4, 32, 8, 1
    X = carve(h.zeros(M, K, dtype=dt), x_bytes, ldx)
    W = carve(h.zeros(K, V, dtype=dt), w_bytes, ldw)
    bias = h.off(h.zeros(V), bias_bytes)
    ids, probs = h.out(M, k, dtype=h.torch.int32), h.out(M, k)
    d = h.L.VocabTopkBf16Desc() if bf else h.L.VocabTopkDesc()
    d.M, d.V, d.K, d.k = M, V, K, k
    d.X, d.ldx, d.W, d.ldw, d.bias, d.ids, d.probs = X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), bias.data_ptr(), ids.data_ptr(), probs.data_ptr()
    if bf:
        ws, wsb = h.workspace(h.lib.dc_vocab_topk_bf16_workspace_bytes(M, V, K, k, 0))
        h.raw("dc_vocab_topk_bf16", h.C.byref(d), ws, wsb, h.stream())
    else:
        ws, wsb = h.workspace(h.lib.dc_vocab_topk_workspace_bytes(M, V, k))
        h.raw("dc_vocab_topk_f32", h.C.byref(d), ws, wsb, h.stream())


_TK = "%s: X, W, bias must be 16-byte aligned"
refusal(_TK, "vocab_topk-X+4")(lambda h: _vocab_topk(h, x_bytes=4))
refusal(_TK, "vocab_topk-W+4")(lambda h: _vocab_topk(h, w_bytes=4))
refusal(_TK, "vocab_topk-bias+4")(lambda h: _vocab_topk(h, bias_bytes=4))
refusal(_TK, "vocab_topk-bf16-X+4")(lambda h: _vocab_topk(h, bf=True, x_bytes=4))
refusal(_TK, "vocab_topk-bf16-W+8")(lambda h: _vocab_topk(h, bf=True, w_bytes=8))
refusal(_TK, "vocab_topk-bf16-bias+4")(lambda h: _vocab_topk(h, bf=True, bias_bytes=4))
refusal("%s: K must be a multiple of 32 and ldx, ldw multiples of 4", "vocab_topk-ldx34")(lambda h: _vocab_topk(h, ldx=34))
refusal("%s: K must be a multiple of 32 and ldx, ldw multiples of 4", "vocab_topk-ldw10")(lambda h: _vocab_topk(h, ldw=10))
refusal("%s: K, ldx, ldw must be multiples of 8", "vocab_topk-bf16-ldx36")(lambda h: _vocab_topk(h, bf=True, ldx=36))
refusal("%s: K, ldx, ldw must be multiples of 8", "vocab_topk-bf16-ldw12")(lambda h: _vocab_topk(h, bf=True, ldw=12))


def _beam_select(h, moved):
    R, k, U, steps = 2, 2, 4, 2
    rows = {n: h.zeros(k * R, U) for n in ("h_in", "c_in")}
    rows.update({n: h.out(k * R, U, nbytes=4 if moved == n else 0) for n in ("h_out", "c_out")})
    if moved in ("h_in", "c_in"):
        rows[moved] = h.off(rows[moved])
    h.ops.beam_select(h.i32(k * R, k), h.zeros(k * R, k), None, h.out(R, k), h.out(steps, R, k, dtype=h.torch.int32),
                      h.out(steps, R, k, dtype=h.torch.int32), 0, 1, **rows)


for _name in ("h_in", "c_in", "h_out", "c_out"):
    refusal("%s: row set %d must be 16-byte aligned", "beam_select-%s+4" % _name)(lambda h, _n=_name: _beam_select(h, _n))


# --- LSTM ------------------------------------------------------------------------------------------------------------------------------
def _lstm_fwd(h, moved):
    B, T, U = 2, 2, 4
    if moved == "workspace":
        h.misplace_workspace()
    z = h.watch(h.zeros(T * B, 4 * U))
    U_rec = h.off(h.zeros(U, 4 * U), 4 if moved == "U_rec" else 0)
    masks = h.off(h.zeros(4, B, U), 4 if moved == "rec_masks" else 0)
    h.ops.lstm_seq_fwd(z, U_rec, None, B, T, h_seq=h.out(T * B, U, nbytes=4 if moved == "h_seq" else 0), c_seq=h.out(T * B, U), rec_masks=masks)


for _name in ("U_rec", "h_seq", "rec_masks", "workspace"):
    refusal("dc_lstm_seq_fwd: U_rec, h_seq, rec_masks and the workspace must be 16-byte aligned", "lstm_seq_fwd-%s+4" % _name)(
        lambda h, _n=_name: _lstm_fwd(h, _n))


def _lstm_bwd(h, moved):
    B, T, U = 2, 2, 4
    if moved == "workspace":
        h.misplace_workspace()
    t = {"U_rec": h.zeros(U, 4 * U), "h_seq": h.zeros(T * B, U)}
    if moved in t:
        t[moved] = h.off(t[moved])
    h.ops.lstm_seq_bwd(h.zeros(T * B, 4 * U), t["U_rec"], None, t["h_seq"], h.zeros(T * B, U), B, T, dh_seq=h.zeros(T * B, U),
                       dz=h.out(T * B, 4 * U, nbytes=4 if moved == "dz" else 0), dU=h.out(U, 4 * U))


for _name in ("U_rec", "h_seq", "dz", "workspace"):
    refusal("dc_lstm_seq_bwd: U_rec, h_seq, dz and the workspace must be 16-byte aligned", "lstm_seq_bwd-%s+4" % _name)(
        lambda h, _n=_name: _lstm_bwd(h, _n))


@refusal("dc_lstm_step: h_prev must be 16-byte aligned", "lstm_step-h_prev+4")
def _(h):
    B, U = 2, 32
    h.ops.lstm_step(h.watch(h.zeros(B, 4 * U)), h.zeros(U, 4 * U), h_prev=h.off(h.zeros(B, U)), c_prev=h.zeros(B, U), h=h.out(B, U),
                    c=h.out(B, U), U_packed=h.zeros(U, 4 * U))


# message literal -> why no case provokes it (keep this empty: a new DC_EALIGN site comes with its refusal case)
UNPROVOKED = {}


def refusal_literals():
    return {lit for lit, _, _ in REFUSALS}
