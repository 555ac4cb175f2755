"""The workspace contract of include/dcap.h, case by case: every entry point that takes (void* workspace, size_t workspace_bytes) runs
on a buffer of EXACTLY dc_*_workspace_bytes() bytes, poisoned, with guard bytes on either side, and refuses one that is a byte short.
This module holds what tests/test_gpu_workspace_contract.py (the runs on the device) and tests/test_workspace_inventory.py (every such
entry point of the header has a case, every case's size query is positive; CPU only) share.  Plain module, no fixtures; torch and the
package are imported inside the functions, so importing it needs neither a GPU nor the built library.

A case is one function `body(c)` over a Ctx: it uploads its deterministic inputs, allocates every output with c.out() and makes each
library call inside `with c.call("dc_..."):`.  Case.run(ops) runs the body to its end and returns the outputs; Case.raw_call(ops, lib,
index, mode) runs the calls before `index` as they are and call `index` with outputs that are sentinel-filled and watched
(_placement_cases.Harness) and a workspace that is one byte short of what the wrapper asked for ("short": an exact, guarded buffer,
workspace_bytes = need - 1) or missing ("null": workspace = NULL, workspace_bytes = need).  The wrapper of image_captioning_amd/ops.py
is the ctypes call; the provider installed as ops.WORKSPACE decides which (workspace, workspace_bytes) pair the entry point sees.

References come from oracle.np_oracle and the builders of the sibling tests; tolerances are the sibling tests' own.  Operands on the
binary grids of _placement_cases are compared with the float64 result by equality."""
import contextlib
import ctypes as C
import functools

import numpy as np

import _placement_cases as PC

DC_EWORKSPACE = -3
FRONT = 64 << 10                              # bytes of guard before the scratch part
PATTERN = 0xA5                                # what the guards hold
DUMMY = 0x7F0000100000                        # a non-null, 4 KiB aligned address for the host-only size queries (never dereferenced)


def back_guard_bytes(nbytes):
    """max(1 MiB, 4 * nbytes) rounded up to 256: an under-reported size of up to 5x stays inside memory the test owns, and the room is
    at least what the same request has inside ops.WORKSPACE (never below 1 MiB, 25 % slack)."""
    return (max(1 << 20, 4 * int(nbytes)) + 255) // 256 * 256


class Guarded(object):
    """One allocation `front guard | nbytes | back guard`, the scratch part on a 256-byte boundary."""

    def __init__(self, nbytes, fill, device):
        import torch
        self.nbytes, back = int(nbytes), back_guard_bytes(nbytes)
        self.whole = torch.empty(256 + FRONT + self.nbytes + back, dtype=torch.uint8, device=device)
        off = (-self.whole.data_ptr()) % 256
        self.front = self.whole[off:off + FRONT]
        self.view = self.whole[off + FRONT:off + FRONT + self.nbytes]
        self.back = self.whole[off + FRONT + self.nbytes:off + FRONT + self.nbytes + back]
        self.whole.fill_(PATTERN)
        self.view.fill_(fill)
        assert self.view.data_ptr() % 256 == 0 and self.view.numel() == self.nbytes

    def damage(self):
        """None when both guards hold the pattern, else where they do not: (guard, first byte, last byte, count) per damaged guard --
        offsets count from the guard's own start (the back guard starts at the first byte past the scratch part)."""
        found = []
        for name, g in (("front", self.front), ("back", self.back)):
            bad = (g != PATTERN).nonzero().flatten()
            if bad.numel():
                found.append((name, int(bad[0]), int(bad[-1]), int(bad.numel())))
        return found or None


class ExactWorkspace(object):
    """A drop-in for ops.WORKSPACE: every get() hands out a fresh buffer of exactly the bytes asked for, filled with `fill`, between
    guards.  handed: every allocation; asked: every size, zeros included."""

    def __init__(self, fill):
        self.fill, self.handed, self.asked = fill, [], []

    def get(self, nbytes, device):
        nbytes = int(nbytes)
        self.asked.append(nbytes)
        if nbytes == 0:
            return None, 0
        g = Guarded(nbytes, self.fill, device)
        self.handed.append(g)
        return g.view, nbytes

    def damage(self):
        import torch
        torch.cuda.synchronize()
        found = [(g.nbytes, d) for g in self.handed for d in [g.damage()] if d]
        return found or None

    def guards_intact(self):
        return self.damage() is None


class ShortWorkspace(ExactWorkspace):
    """The refusal tests' provider.  mode "short": the exact guarded buffer with workspace_bytes one less than asked; "null": no buffer,
    workspace_bytes as asked."""

    def __init__(self, mode):
        ExactWorkspace.__init__(self, PATTERN)
        assert mode in ("short", "null")
        self.mode = mode

    def get(self, nbytes, device):
        if int(nbytes) == 0 or self.mode == "null":
            self.asked.append(int(nbytes))
            return None, int(nbytes)
        view, n = ExactWorkspace.get(self, nbytes, device)
        return view, n - 1


@contextlib.contextmanager
def swapped(ops, provider):
    """ops.WORKSPACE is `provider` while the block lasts; the module's own provider is back afterwards, whatever the block did."""
    before = ops.WORKSPACE
    ops.WORKSPACE = provider
    try:
        yield provider
    finally:
        ops.WORKSPACE = before


class _Stop(Exception):
    """Ends a body after the call under test."""


class Ctx(object):
    """What a case's body works with: ops, the outputs made so far (t) and the call markers."""

    def __init__(self, ops, lib=None, target=None, mode=None):
        self.ops, self.lib, self.target, self.mode = ops, lib, target, mode
        self.t, self.index, self.live = {}, -1, False
        self.h = PC.Harness(ops, lib) if target is not None else None
        self.symbol = self.error = self.provider = None

    def out(self, name, *shape, dtype=None, init=None):
        """An output tensor: sentinel-filled (an in / out operand: `init`'s values).  Inside the call under test it is carved out of a
        larger sentinel buffer and watched."""
        import torch
        dtype = dtype or torch.float32
        if init is not None:
            t = PC.dev(init, dtype)
            if self.live:
                self.h.watch(t)
        elif self.live:
            t = self.h.out(*shape, dtype=dtype)
        else:
            t = PC.sentinel_like(shape, dtype)
        self.t[name] = t
        return t

    @contextlib.contextmanager
    def call(self, symbol):
        self.index += 1
        if self.target is None or self.index < self.target:
            yield
            return
        from image_captioning_amd import _lib
        self.symbol, self.provider, self.live = symbol, ShortWorkspace(self.mode), True
        try:
            with swapped(self.ops, self.provider):
                yield
        except _lib.DcapError as e:
            self.error = e
        finally:
            self.live = False
        raise _Stop()


class Case(object):
    """id, the dc_* entry points its body calls IN CALL ORDER (symbols), need(lib) -> the size query's answer for the case, body(c),
    check(outputs).  serves_short: indices of calls whose entry point serves a short workspace instead of refusing it."""

    def __init__(self, id, symbols, need, body, check, serves_short=()):
        self.id, self.symbols, self.need, self.body, self.check, self.serves_short = id, tuple(symbols), need, body, check, tuple(serves_short)

    def run(self, ops):
        c = Ctx(ops)
        self.body(c)
        assert c.index + 1 == len(self.symbols), "%s: the body made %d calls, symbols names %d" % (self.id, c.index + 1, len(self.symbols))
        return c.t

    def raw_call(self, ops, lib, index, mode):
        """-> the Ctx after call `index` ran on a short / missing workspace: error (DcapError or None), provider, h (the Harness that
        watched the outputs), t (the outputs)."""
        c = Ctx(ops, lib, index, mode)
        try:
            self.body(c)
        except _Stop:
            pass
        assert c.symbol == self.symbols[index], (c.symbol, self.symbols[index])
        return c


CASES = []


def case(id, symbols, need, check, serves_short=()):
    def deco(body):
        assert id not in [c.id for c in CASES]
        CASES.append(Case(id, symbols, need, body, check, serves_short))
        return body
    return deco


def by_id(id):
    return [c for c in CASES if c.id == id][0]


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers

def _L():
    from image_captioning_amd import _lib
    return _lib


def _torch():
    import torch
    return torch


def _O():
    from oracle import np_oracle as O
    return O


def _desc(cls, pointers=(), **fields):
    """A descriptor with the given fields; every name in `pointers` gets a distinct dummy address."""
    d = cls()
    for k, v in fields.items():
        setattr(d, k, v)
    for i, name in enumerate(pointers):
        setattr(d, name, DUMMY + (i << 32))
    return d


def host(t):
    return PC.host(t)


def equal(got, want, what=""):
    got = host(got) if not isinstance(got, np.ndarray) else got
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d of %d entries differ, first at %s: got %r want %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


def close(got, want, tol, what=""):
    """test_gpu_kernels.close / test_gpu_bf16.close: the largest error over max(1, largest |want|)."""
    got = host(got) if not isinstance(got, np.ndarray) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
    print("%s: max err %.3e (scaled), tolerance %.1e" % (what, err, tol))
    assert err < tol, "%s: max err %.3e (scaled) exceeds %.1e" % (what, err, tol)


def bf16(a):
    """float64 / float32 host array -> bf16 device tensor (the values are exact in bf16 on the grids used here)."""
    torch = _torch()
    t = PC.dev(a).to(torch.bfloat16)
    assert np.array_equal(host(t), np.asarray(a, np.float64)), "operand is not exact in bf16"
    return t


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_gemm_f32: exact operands (_placement_cases.gemm_case), shift + accumulate epilogue (additive: the K % 32 tail pair may run)

@functools.lru_cache(maxsize=None)
def _gemm_data(M, N, K):
    return PC.gemm_case(1000 + M + N + K, M, N, K, scale=False, shift=True, relu=False, accumulate=True)


def _gemm_f32(M, N, K, split_k, b_trans=False):
    def need(lib):
        d = _desc(_L().GemmDesc, ("A", "B", "C", "shift"), M=M, N=N, K=K, lda=K, ldb=K if b_trans else N, b_trans=int(b_trans), ldc=N,
                  accumulate=1, split_k=split_k)
        return lib.dc_gemm_workspace_bytes(C.byref(d))

    def body(c):
        g = _gemm_data(M, N, K)
        A, B, sh = PC.dev(g["A"]), PC.dev(g["B"].T if b_trans else g["B"]), PC.dev(g["shift"])
        with c.call("dc_gemm_f32"):
            c.ops.gemm(A, B, out=c.out("C", M, N, init=g["C0"]), b_trans=b_trans, shift=sh, accumulate=True, split_k=split_k)

    def check(t):
        equal(t["C"], _gemm_data(M, N, K)["want"], "C")

    name = "gemm_f32-%dx%dx%d-%s" % (M, N, K, "auto" if not split_k else "split%d" % split_k)
    case(name, ["dc_gemm_f32"], need, check)(body)


_gemm_f32(64, 64, 256, 0)            # choose_tile: fewer than 256 blocks, 8 K-tiles -> split 2
_gemm_f32(8, 8, 128, 2)
_gemm_f32(64, 64, 300, 0)            # the gemm_split_tail pair: K = 288 split, then the range-checked tail on the same workspace
_gemm_f32(64, 62, 256, 2, b_trans=True)     # N % 4 != 0: the scalar slab path of splitk_reduce_kernel (B as [N][K]: ldb % 4 == 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_gemm_bf16

@functools.lru_cache(maxsize=None)
def _bgemm_data(M, N, K):
    return PC.gemm_case(2000 + M + N + K, M, N, K, scale=False, shift=True, relu=False, accumulate=False)


def _bgemm_desc(M, N, K, split_k):
    return _desc(_L().GemmBf16Desc, ("A", "B", "C", "shift"), M=M, N=N, K=K, lda=K, ldb=N, ldc=N, split_k=split_k)


def bgemm_plan(lib, M, N, K, split_k):
    """(tile, slices) dc_gemm_bf16 runs the case's problem with (dc_gemm_bf16_tile: host only)."""
    sk = C.c_int(0)
    tile = lib.dc_gemm_bf16_tile(C.byref(_bgemm_desc(M, N, K, split_k)), C.byref(sk))
    return int(tile), int(sk.value)


def _gemm_bf16(M, N, K, split_k, tile):
    def need(lib):
        return lib.dc_gemm_bf16_workspace_bytes(C.byref(_bgemm_desc(M, N, K, split_k)))

    def body(c):
        g = _bgemm_data(M, N, K)
        A, B, sh = bf16(g["A"]), bf16(g["B"]), PC.dev(g["shift"])
        info = {}
        with c.call("dc_gemm_bf16"):
            try:
                c.ops.gemm_bf16(A, B, out=c.out("C", M, N), shift=sh, split_k=split_k, info=info)
            finally:
                assert info["tile"] == tile and info["split_k"] > 1, info

    def check(t):
        equal(t["C"], _bgemm_data(M, N, K)["want"], "C")

    case("gemm_bf16-%dx%dx%d-split%d-tile%d" % (M, N, K, split_k, tile), ["dc_gemm_bf16"], need, check)(body)


_gemm_bf16(64, 128, 512, 3, 128)
_gemm_bf16(1024, 1024, 8192, 16, 256)    # test_gemm_bf16_256_tile_layouts' split shape (at K = 2048, split 4 the plan leaves the 256 tile)
BGEMM_256 = (1024, 1024, 8192, 16)


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_conv2d_nhwc_f32 (math 0: igemm; math 1: the igemm_bf16s.h launcher) and dc_conv2d_wgrad_f32

def _conv_desc(cls, N, H, W, Cin, Cout, k, stride, pad, Ho, Wo, pointers, **kw):
    return _desc(cls, pointers, N=N, H=H, W=W, Cin=Cin, Cout=Cout, kh=k, kw=k, stride=stride, pad_t=pad, pad_l=pad, Ho=Ho, Wo=Wo, **kw)


@functools.lru_cache(maxsize=None)
def _conv_data(N, H, W, Cin, Cout, k, stride):
    return PC.conv_case(3000 + H + Cin + Cout + k, N, H, W, Cin, Cout, k, stride, res_mode=0, relu=True)


def _conv_f32(shape, math):
    N, H, W, Cin, Cout, k, stride = shape

    def need(lib):
        g = _conv_data(*shape)
        d = _conv_desc(_L().ConvDesc, N, H, W, Cin, Cout, k, stride, g["pad"], g["Ho"], g["Wo"], ("x", "w", "y", "scale", "shift"), relu=1, math=math)
        return lib.dc_conv2d_workspace_bytes(C.byref(d))

    def body(c):
        g = _conv_data(*shape)
        x, w, sc, sh = PC.dev(g["x"]), PC.dev(g["w"]), PC.dev(g["scale"]), PC.dev(g["shift"])
        with c.call("dc_conv2d_nhwc_f32"):
            c.ops.conv2d(x, w, k, k, stride, g["pad"], g["pad"], g["Ho"], g["Wo"], sc, sh, relu=True, math=math,
                         out=c.out("y", N, g["Ho"], g["Wo"], Cout))

    def check(t):
        equal(t["y"], _conv_data(*shape)["want"], "y")

    case("conv2d_f32-%s-math%d" % ("x".join(map(str, shape)), math), ["dc_conv2d_nhwc_f32"], need, check)(body)


_conv_f32((1, 8, 8, 512, 512, 3, 1), 0)      # CONV_CASES' "small M, long K: split-K path"
_conv_f32((1, 8, 8, 512, 512, 3, 1), 1)


@functools.lru_cache(maxsize=None)
def _wgrad_data(N, H, W, Cin, Cout, k, stride):
    """x in steps of 1/8 within +-1, dy in steps of 1/256 within +-1/16 (exact in bf16 too), the accumulate base in steps of 1/8 within
    +-4: every product is a multiple of 2^-11 and every partial sum stays below N H W / 16 <= 2^7, so dw is exact in any order."""
    O = _O()
    rng = np.random.default_rng(4000 + H + Cin + Cout + k)
    pad = (k - 1) // 2
    x = PC.grid(rng, (N, H, W, Cin), 1 / 8, 1.0)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = PC.grid(rng, (N, Ho, Wo, Cout), 1 / 256, 1 / 16)
    assert N * Ho * Wo / 16.0 + 4.0 < 2.0 ** 12
    _, dw, _ = O.conv2d_nhwc_backward(x, np.zeros((k, k, Cin, Cout)), dy, stride, 'same' if k == 3 else 'valid')
    want = PC.assert_exact_f32(np.transpose(dw, (3, 0, 1, 2)).reshape(Cout, k * k * Cin), "dw")
    base = PC.grid(rng, want.shape, 1 / 8, 4.0)
    return {"x": x, "dy": dy, "pad": pad, "Ho": Ho, "Wo": Wo, "want": want, "base": base, "want_acc": PC.assert_exact_f32(want + base, "dw + base")}


def _wgrad_f32(shape, accumulate):
    N, H, W, Cin, Cout, k, stride = shape

    def need(lib):
        pad = (k - 1) // 2
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        d = _conv_desc(_L().ConvDesc, N, H, W, Cin, Cout, k, stride, pad, Ho, Wo, ("x", "w", "y"), accumulate=int(accumulate))
        return lib.dc_conv2d_wgrad_workspace_bytes(C.byref(d))

    def body(c):
        g = _wgrad_data(*shape)
        x, dy = PC.dev(g["x"]), PC.dev(g["dy"])
        with c.call("dc_conv2d_wgrad_f32"):
            out = c.out("dw", Cout, k * k * Cin, init=g["base"] if accumulate else None)
            c.ops.conv2d_wgrad(x, dy, k, k, stride, g["pad"], g["pad"], out=out, accumulate=accumulate)

    def check(t):
        g = _wgrad_data(*shape)
        equal(t["dw"], g["want_acc"] if accumulate else g["want"], "dw")

    case("wgrad_f32-%s%s" % ("x".join(map(str, shape)), "-accumulate" if accumulate else ""), ["dc_conv2d_wgrad_f32"], need, check)(body)


_wgrad_f32((2, 16, 16, 64, 64, 3, 1), False)     # 512 pixels of K, 9 blocks: split 4
_wgrad_f32((2, 16, 16, 64, 64, 3, 1), True)


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_conv2d_bf16 and dc_conv2d_wgrad_bf16

BCONV = (1, 64, 64, 256, 256, 3, 1)          # BCONV_SMALL's first entry; the cost model runs it unsplit, so slabs on request: split_k = 2
BWGRAD = (1, 16, 16, 128, 64, 3, 1)          # the first of test_conv2d_wgrad_bf16_matches_oracle's cases


def _conv_bf16(shape, split_k):
    N, H, W, Cin, Cout, k, stride = shape

    def need(lib):
        pad = (k - 1) // 2
        d = _conv_desc(_L().ConvBf16Desc, N, H, W, Cin, Cout, k, stride, pad, H, W, ("x", "w", "y", "y_bf16", "scale", "shift"), relu=1, split_k=split_k)
        return lib.dc_conv2d_bf16_workspace_bytes(C.byref(d))

    def body(c):
        torch = _torch()
        g = _conv_data(*shape)
        x, w, sc, sh = bf16(g["x"]), bf16(g["w"]), PC.dev(g["scale"]), PC.dev(g["shift"])
        with c.call("dc_conv2d_bf16"):
            c.ops.conv2d_bf16(x, w, k, k, stride, g["pad"], g["pad"], g["Ho"], g["Wo"], scale=sc, shift=sh, relu=True, split_k=split_k,
                              out=c.out("y", N, g["Ho"], g["Wo"], Cout), out_bf16=c.out("y_bf16", N, g["Ho"], g["Wo"], Cout, dtype=torch.bfloat16))

    def check(t):
        want = _conv_data(*shape)["want"]
        equal(t["y"], want, "y")
        equal(t["y_bf16"], PC.bf16_of(want), "y_bf16")

    case("conv2d_bf16-%s-split%d" % ("x".join(map(str, shape)), split_k), ["dc_conv2d_bf16"], need, check)(body)


_conv_bf16(BCONV, 2)


def _wgrad_bf16(shape, split_k, accumulate):
    N, H, W, Cin, Cout, k, stride = shape

    def need(lib):
        pad = (k - 1) // 2
        d = _conv_desc(_L().ConvWgradBf16Desc, N, H, W, Cin, Cout, k, stride, pad, H, W, ("x", "dy", "dw"), split_k=split_k, accumulate=int(accumulate))
        return lib.dc_conv2d_wgrad_bf16_workspace_bytes(C.byref(d))

    def body(c):
        g = _wgrad_data(*shape)
        x, dy = bf16(g["x"]), bf16(g["dy"])
        with c.call("dc_conv2d_wgrad_bf16"):
            out = c.out("dw", Cout, k * k * Cin, init=g["base"] if accumulate else None)
            c.ops.conv2d_wgrad_bf16(x, dy, k, k, stride, g["pad"], g["pad"], out=out, split_k=split_k, accumulate=accumulate)

    def check(t):
        g = _wgrad_data(*shape)
        equal(t["dw"], g["want_acc"] if accumulate else g["want"], "dw")

    case("wgrad_bf16-%s-split%d%s" % ("x".join(map(str, shape)), split_k, "-accumulate" if accumulate else ""), ["dc_conv2d_wgrad_bf16"], need, check)(body)


_wgrad_bf16(BWGRAD, 2, False)
_wgrad_bf16(BWGRAD, 2, True)


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_lstm_seq_fwd_f32 / dc_lstm_seq_bwd_f32: test_lstm_seq_forward_backward and test_lstm_recurrent_dropout_matches_oracle

@functools.lru_cache(maxsize=None)
def _lstm_data(B, T, I, U, masks, seq_mask):
    O = _O()
    rng = np.random.default_rng(B + T + U)
    x = rng.standard_normal((B, T, I))
    W = rng.standard_normal((I, 4 * U)) / np.sqrt(I)
    Ur = rng.standard_normal((U, 4 * U)) / np.sqrt(U)
    b = 0.1 * rng.standard_normal(4 * U)
    mask = None
    if seq_mask:
        mask = rng.random((B, T)) > 0.3
        mask[0] = False                                   # a fully masked row
        mask[1] = True
    rm = O.recurrent_dropout_masks(rng, B, U, 0.2) if masks else None
    H, cache = O.lstm_forward(x, mask, W, Ur, b, rec_masks=rm)
    dH = rng.standard_normal((B, T, U))
    dlast = rng.standard_normal((B, U))
    dx, dW, dU, db = O.lstm_backward(dH, cache, dh_last=dlast)
    xt = np.transpose(x, (1, 0, 2)).reshape(T * B, I)
    dU0 = rng.standard_normal((U, 4 * U))
    return {"xt": xt, "z": (xt @ W + b).astype(np.float32), "Ur": Ur, "mask": mask, "rm": rm, "H": H, "dH": np.transpose(dH, (1, 0, 2)).reshape(T * B, U),
            "dlast": dlast, "dW": dW, "dU": dU, "db": db, "dU0": dU0}


def _lstm_seq(B, T, I, U, masks, accumulate=False):
    seq_mask = B >= 3 and T > 1
    key = (B, T, I, U, masks, seq_mask)

    def need(lib):
        return lib.dc_lstm_seq_workspace_bytes(B, T, U)

    def body(c):
        torch = _torch()
        g = _lstm_data(*key)
        z, Ud = PC.dev(g["z"]), PC.dev(g["Ur"])
        mk = None if g["mask"] is None else PC.dev(g["mask"].T.reshape(-1), torch.uint8)
        rmd = None if g["rm"] is None else PC.dev(g["rm"])
        dh_seq, dh_last = PC.dev(g["dH"]), PC.dev(g["dlast"])
        with c.call("dc_lstm_seq_fwd_f32"):
            if c.live:
                c.h.watch(z)                               # in / out: the pre-activations
            h_seq, c_seq = c.ops.lstm_seq_fwd(z, Ud, mk, B, T, h_seq=c.out("h_seq", T * B, U), c_seq=c.out("c_seq", T * B, U), rec_masks=rmd)
        c.t["z"] = z
        with c.call("dc_lstm_seq_bwd_f32"):
            c.ops.lstm_seq_bwd(z, Ud, mk, h_seq, c_seq, B, T, dh_seq=dh_seq, dh_last=dh_last, dz=c.out("dz", T * B, 4 * U),
                               dU=c.out("dU", U, 4 * U), rec_masks=rmd)
        if accumulate:
            with c.call("dc_lstm_seq_bwd_f32"):
                c.ops.lstm_seq_bwd(z, Ud, mk, h_seq, c_seq, B, T, dh_seq=dh_seq, dh_last=dh_last, dz=c.out("dz_acc", T * B, 4 * U),
                                   dU=c.out("dU_acc", U, 4 * U, init=g["dU0"]), accumulate_dU=True, rec_masks=rmd)

    def check(t):
        g = _lstm_data(*key)
        close(host(t["h_seq"]).reshape(T, B, U).transpose(1, 0, 2), g["H"], 2e-5, "h_seq")
        dz = host(t["dz"])
        close(t["dU"], g["dU"], 5e-5, "dU")
        close(g["xt"].T @ dz, g["dW"], 5e-5, "dW = x^T dz")
        close(dz.sum(0), g["db"], 5e-5, "db = colsum dz")
        if accumulate:
            close(t["dU_acc"], g["dU"] + g["dU0"], 5e-5, "dU0 + dU")
            equal(t["dz_acc"], dz, "dz of the accumulating call")

    name = "lstm_seq-%dx%dx%dx%d-%s%s" % (B, T, I, U, "masks" if masks else "plain", "-accumulate_dU" if accumulate else "")
    case(name, ["dc_lstm_seq_fwd_f32", "dc_lstm_seq_bwd_f32"] + (["dc_lstm_seq_bwd_f32"] if accumulate else []), need, check)(body)


_lstm_seq(3, 4, 8, 4, False)                       # unfused both ways
_lstm_seq(6, 5, 16, 32, False, accumulate=True)    # fused forward with the U_rec pack at the end, fused backward; accumulate_dU 0 and 1
_lstm_seq(6, 5, 16, 32, True)                      # fused masked forward (drop_fused), fused backward
_lstm_seq(16, 5, 16, 32, True)                     # the masked copies outgrow the U_rec pack: `drop` is the largest scenario, within 1 KiB of what runs
_lstm_seq(8, 3, 16, 260, True)                     # U % 16 != 0: unfused; K = 260 ragged: slabs at the front, hm / tmp4 / hm_seq at the end
_lstm_seq(130, 3, 16, 260, False)                  # the dU_rec GEMM has K = (T - 1) B = 260 and splits too
_lstm_seq(130, 3, 16, 260, True)
_lstm_seq(5, 1, 16, 32, False)                     # T = 1


# dc_lstm_step_f32: one step from a given state, against O.lstm_forward(T = 1, h0, c0) (W = identity: x is the projection itself)

@functools.lru_cache(maxsize=None)
def _step_data(B, U):
    O = _O()
    rng = np.random.default_rng(77 + B + U)
    z = rng.standard_normal((B, 4 * U)).astype(np.float32)
    Ur = rng.standard_normal((U, 4 * U)) / np.sqrt(U)
    h0, c0 = 0.5 * rng.standard_normal((B, U)), 0.5 * rng.standard_normal((B, U))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    H, cache = O.lstm_forward(z.astype(np.float64)[:, None, :], None, np.eye(4 * U), f32(Ur), np.zeros(4 * U), h0=f32(h0), c0=f32(c0))
    return {"z": z, "Ur": Ur, "h0": h0, "c0": c0, "h": H[:, 0], "c": cache["c_last"]}


def _lstm_step(B, U):
    def need(lib):
        return lib.dc_lstm_step_workspace_bytes(B, U)

    def body(c):
        g = _step_data(B, U)
        z, Ud, h0, c0 = PC.dev(g["z"]), PC.dev(g["Ur"]), PC.dev(g["h0"]), PC.dev(g["c0"])
        with c.call("dc_lstm_step_f32"):
            if c.live:
                c.h.watch(z)
            c.ops.lstm_step(z, Ud, h_prev=h0, c_prev=c0, h=c.out("h", B, U), c=c.out("c", B, U), U_packed=None)
        c.t["z"] = z

    def check(t):
        g = _step_data(B, U)
        close(t["h"], g["h"], 2e-5, "h")
        close(t["c"], g["c"], 2e-5, "c")

    case("lstm_step-%dx%d" % (B, U), ["dc_lstm_step_f32"], need, check)(body)


_lstm_step(8, 32)          # U_packed = NULL: the pack goes at the end of the workspace
_lstm_step(8, 260)         # the unfused step: the GEMM with its slabs


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_vocab_ce: the construction of test_vocab_ce_masked_keras_sparse (a clipped-low and a clipped-high target, a zero-weight row)

@functools.lru_cache(maxsize=None)
def _ce_data(M, V, K, bf):
    O = _O()
    rng = np.random.default_rng(V + K)
    X = rng.standard_normal((M, K))
    W = rng.standard_normal((K, V)) * (2.0 / np.sqrt(K))
    b = rng.standard_normal(V)
    t = rng.integers(0, V, M)
    b[t[0]] -= 80.0
    X[1] = 0
    w = rng.random(M)
    w[2] = 0.0
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    z = (O.to_bf16(X) @ O.to_bf16(W) if bf else f32(X) @ f32(W)) + b
    want_loss, want_d = O.sparse_cce_keras_with_grad(t, O.softmax(z), w)
    return {"X": X, "W": W, "b": b, "t": t, "w": w, "loss": want_loss, "d": want_d}


def _vocab_ce(M, V, K, bf):
    def need(lib):
        d = _desc(_L().VocabCeDesc, ("X", "W", "bias", "targets", "row_weights", "loss_rows", "dlogits", "dbias"), M=M, V=V, K=K, bf16=int(bf),
                  ldx=K, ldw=V, lddl=V, dl_bf16=0, grad_scale=1.0, keras_sparse=1, materialize_bf16=0)
        return lib.dc_vocab_ce_workspace_bytes(C.byref(d))

    def body(c):
        torch = _torch()
        g = _ce_data(M, V, K, bf)
        Xd, Wd = PC.dev(g["X"]), PC.dev(g["W"])
        if bf:
            Xd, Wd = Xd.to(torch.bfloat16), Wd.to(torch.bfloat16)
        bd, td, wd = PC.dev(g["b"]), PC.dev(g["t"], torch.int32), PC.dev(g["w"])
        with c.call("dc_vocab_ce"):
            c.ops.vocab_ce(Xd, Wd, bd, td, loss_rows=c.out("loss", M), dlogits=c.out("dlogits", M, V), dbias=c.out("dbias", V), grad_scale=1.0,
                           row_weights=wd, keras_sparse=True)

    def check(t):
        g = _ce_data(M, V, K, bf)
        close(t["loss"], g["loss"], 3e-5, "loss")
        close(t["dlogits"], g["d"], 3e-5, "dlogits")
        close(t["dbias"], g["d"].sum(0), 1e-4, "dbias")
        assert float(t["dlogits"][2].abs().max()) == 0.0

    case("vocab_ce-%dx%dx%d-%s" % (M, V, K, "bf16" if bf else "f32"), ["dc_vocab_ce"], need, check)(body)


_vocab_ce(9, 24, 64, False)
_vocab_ce(33, 1000, 1024, False)
_vocab_ce(33, 1000, 1024, True)


# ---------------------------------------------------------------------------------------------------------------------------------
# the vocabulary reductions on _decode_cases._exact_operands: the logits are exact, so ids equal the float64 answer

VM, VV = 37, 1001
SEED, OFFSET = 20240611, 3


@functools.lru_cache(maxsize=None)
def _vocab_data(K):
    """(X, W, b, float64 logits z) on _decode_cases._exact_operands."""
    from _decode_cases import _exact_operands
    X, W, b = _exact_operands(np.random.default_rng(VM * 7 + VV + K), VM, K, VV)
    z = X.astype(np.float64) @ W.astype(np.float64) + b.astype(np.float64)
    return X, W, b, z


def _vocab_operands(K, bf):
    X, W, b, _ = _vocab_data(K)
    if bf:
        return bf16(X), bf16(W), PC.dev(b)
    return PC.dev(X), PC.dev(W), PC.dev(b)


def topk_reference(K, k):
    """ids [M,k] (value descending, then column ascending: test_top_k_5_draws_among_the_five_best's order) and their softmax
    probabilities (_sampling_ref.softmax_of)."""
    import _sampling_ref as S
    z = _vocab_data(K)[3]
    ids = np.argsort(-z, axis=1, kind="stable")[:, :k]
    return ids, np.stack([S.softmax_of(z, ids[:, j]) for j in range(k)], axis=1)


def sample_reference(K, top_k, tau):
    """(ids, smallest gap between the two best perturbed values, probabilities): _sampling_ref's restatement."""
    import _sampling_ref as S
    z = _vocab_data(K)[3]
    assert np.abs(z * S.inv_t(tau)).max() <= 16
    allowed = None
    if top_k:
        allowed = np.zeros(z.shape, bool)
        np.put_along_axis(allowed, np.argsort(-z, axis=1, kind="stable")[:, :top_k], True, axis=1)
    want, gap = S.choose(S.perturbed(z, tau, SEED, OFFSET), allowed)
    return want, float(gap.min()), S.softmax_of(z, want)


def _vocab_top(K, k, bf, tile, top1):
    sym = "dc_vocab_top%s_%s" % ("1" if top1 else "k", "bf16" if bf else "f32")

    def need(lib):
        if bf:
            return lib.dc_vocab_top1_bf16_workspace_bytes(VM, VV, K, tile) if top1 else lib.dc_vocab_topk_bf16_workspace_bytes(VM, VV, K, k, tile)
        return lib.dc_vocab_top1_workspace_bytes(VM, VV) if top1 else lib.dc_vocab_topk_workspace_bytes(VM, VV, k)

    def body(c):
        torch = _torch()
        X, W, b = _vocab_operands(K, bf)
        kw = dict(tile=tile) if bf else {}
        with c.call(sym):
            if top1:
                c.ops.vocab_top1(X, W, b, tokens=c.out("ids", VM, dtype=torch.int32), probs=c.out("probs", VM), mask=c.out("mask", VM, dtype=torch.uint8), **kw)
            else:
                c.ops.vocab_topk(X, W, b, k, ids=c.out("ids", VM, k, dtype=torch.int32), probs=c.out("probs", VM, k), **kw)

    def check(t):
        ids, p = topk_reference(K, k)
        got_ids, got_p = t["ids"].cpu().numpy().reshape(VM, k), t["probs"].cpu().numpy().reshape(VM, k)
        np.testing.assert_array_equal(got_ids, ids)
        np.testing.assert_allclose(got_p, p, rtol=1e-6, atol=0)
        if top1:
            np.testing.assert_array_equal(t["mask"].cpu().numpy(), (ids[:, 0] != 0).astype(np.uint8))

    case("%s-%dx%dx%d-k%d%s" % (sym[3:], VM, VV, K, k, "-tile%d" % tile if bf else ""), [sym], need, check)(body)


_vocab_top(64, 1, False, 0, True)
_vocab_top(64, 3, False, 0, False)
_vocab_top(256, 8, False, 0, False)
_vocab_top(64, 1, True, 128, True)
_vocab_top(256, 1, True, 256, True)
_vocab_top(64, 3, True, 128, False)
_vocab_top(256, 8, True, 256, False)


def _vocab_sample(K, top_k, bf, tile, tau):
    sym = "dc_vocab_sample_%s" % ("bf16" if bf else "f32")

    def need(lib):
        if bf:
            return lib.dc_vocab_sample_bf16_workspace_bytes(VM, VV, K, top_k, tile)
        return lib.dc_vocab_sample_workspace_bytes(VM, VV, top_k)

    def body(c):
        torch = _torch()
        X, W, b = _vocab_operands(K, bf)
        kw = dict(tile=tile) if bf else {}
        with c.call(sym):
            c.ops.vocab_sample(X, W, b, temperature=tau, top_k=top_k or None, seed=SEED, offset=OFFSET, tokens=c.out("ids", VM, dtype=torch.int32),
                               probs=c.out("probs", VM), mask=c.out("mask", VM, dtype=torch.uint8), **kw)

    def check(t):
        import _sampling_ref as S
        want, gap, p = sample_reference(K, top_k, tau)
        assert gap >= S.GAP, "an undecided row: pick another seed"
        np.testing.assert_array_equal(t["ids"].cpu().numpy(), want)
        np.testing.assert_allclose(t["probs"].cpu().numpy(), p, rtol=1e-6, atol=0)
        np.testing.assert_array_equal(t["mask"].cpu().numpy(), (want != 0).astype(np.uint8))

    case("%s-%dx%dx%d-top_k%d%s" % (sym[3:], VM, VV, K, top_k, "-tile%d" % tile if bf else ""), [sym], need, check)(body)


SAMPLE_CASES = [(64, 0, False, 0, 1.0), (256, 5, False, 0, 2.0), (64, 0, True, 128, 1.0), (256, 5, True, 256, 2.0)]
for _a in SAMPLE_CASES:
    _vocab_sample(*_a)


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_proposals_f32

@functools.lru_cache(maxsize=None)
def _pyramid_data(B, S):
    """test_rpn_proposals_bit_exact_given_scores' inputs."""
    O = _O()
    rng = np.random.default_rng(S)
    strides, scales, ratios = [4, 8, 16, 32, 64], (32, 64, 128, 256, 512), [0.5, 1, 2]
    shapes = [[S // s, S // s] for s in strides]
    heads = [rng.standard_normal((B, h, w, 18)).astype(np.float32) for h, w in shapes]
    for hd in heads:
        hd[..., 6:] *= 0.5
    heads[0][0, 0, 0, :6] = heads[0][0, 0, 1, :6]              # exact score ties between neighbouring anchors
    anchors = O.generate_pyramid_anchors(scales, ratios, shapes, strides, 1).astype(np.float32)
    return heads, anchors, shapes


def _proposal_desc(B, hw, apl, A_total, k, count, thr, image_hw):
    d = _desc(_L().ProposalDesc, ("anchors", "proposals", "scores_out", "order_out", "keep_out"), B=B, levels=len(hw), anchors_per_loc=apl, A_total=A_total,
              image_h=float(image_hw[0]), image_w=float(image_hw[1]), pre_nms_limit=k, proposal_count=count, nms_threshold=thr)
    for i, (h, w) in enumerate(hw):
        d.heads[i], d.Hs[i], d.Ws[i] = DUMMY + ((8 + i) << 32), h, w
    for i, v in enumerate((0.1, 0.1, 0.2, 0.2)):
        d.std_dev[i] = v
    return d


def _proposals_pyramid(B, S, count=100, pre=600):
    def need(lib):
        heads, anchors, shapes = _pyramid_data(B, S)
        return lib.dc_proposals_workspace_bytes(C.byref(_proposal_desc(B, shapes, 3, anchors.shape[0], pre, count, 0.7, (S, S))))

    def body(c):
        heads, anchors, _ = _pyramid_data(B, S)
        hd, ad = [PC.dev(h) for h in heads], PC.dev(anchors)
        with c.call("dc_proposals_f32"):
            props, (scores, order, keep) = c.ops.rpn_proposals(hd, ad, (S, S), count, 0.7, pre_nms_limit=pre, debug=True, out=c.out("proposals", B, count, 4))
        c.t.update(scores=scores, order=order, keep=keep)

    def check(t):
        O = _O()
        heads, anchors, _ = _pyramid_data(B, S)
        scores, order, keep, props = (t[k].cpu().numpy() for k in ("scores", "order", "keep", "proposals"))
        cls = np.concatenate([h[..., :6].reshape(B, -1, 2) for h in heads], axis=1)
        box = np.concatenate([h[..., 6:].reshape(B, -1, 4) for h in heads], axis=1)
        assert np.abs(scores - O.softmax(cls)[:, :, 1]).max() < 1e-6
        for b in range(B):
            want, ix, kp = O.proposal_layer(scores[b], box[b], anchors, (S, S), count, 0.7, pre_nms_limit=pre)
            np.testing.assert_array_equal(order[b], ix)
            np.testing.assert_array_equal(keep[b][:len(kp)], kp)
            assert np.all(keep[b][len(kp):] == -1)
            np.testing.assert_allclose(props[b], want, rtol=3e-7, atol=1e-7)
            assert np.all(props[b][len(kp):] == 0)

    case("proposals-pyramid-B%d-S%d" % (B, S), ["dc_proposals_f32"], need, check)(body)


_proposals_pyramid(1, 256)

PLANTED = "clustered100_4097"                # the smaller of _proposal_cases' two planted k = 4097 cases


@functools.lru_cache(maxsize=None)
def _planted():
    import _proposal_cases as P
    return P.build(PLANTED)


def _planted_need(lib):
    p = _planted()
    return lib.dc_proposals_workspace_bytes(C.byref(_proposal_desc(p.B, [(1, p.N)], 1, p.N, p.k, p.count, p.thr, p.image_hw)))


def _planted_check(t):
    import _proposal_cases as P
    p = _planted()
    got = {k: t[k].cpu().numpy() for k in ("scores", "order", "keep", "proposals")}
    assert np.abs(got["scores"] - P.host_scores(p.logits)).max() < 1e-6
    k = min(p.k, p.N)
    for b, r in enumerate(P.reference(p, got["scores"])):          # test_gpu_proposals.assert_equals_oracle
        n = len(r["keep"])
        np.testing.assert_array_equal(got["order"][b], np.argsort(-got["scores"][b].astype(np.float64), kind="stable")[:k])
        np.testing.assert_array_equal(got["order"][b], r["order"])
        np.testing.assert_array_equal(got["keep"][b][:n], r["keep"])
        assert np.all(got["keep"][b][n:] == -1)
        np.testing.assert_array_equal(got["proposals"][b][:n], r["proposals"][:n])
        assert np.all(got["proposals"][b][n:] == 0)


@case("proposals-" + PLANTED, ["dc_proposals_f32"], _planted_need, _planted_check)
def _(c):
    p = _planted()
    hd, ad = [PC.dev(p.heads())], PC.dev(p.anchors)
    with c.call("dc_proposals_f32"):
        props, (scores, order, keep) = c.ops.rpn_proposals(hd, ad, p.image_hw, p.count, p.thr, pre_nms_limit=p.k, anchors_per_loc=1, debug=True,
                                                           out=c.out("proposals", p.B, p.count, 4))
    c.t.update(scores=scores, order=order, keep=keep)


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_refine_generations_f64: test_against_the_host_path_at_the_mask_word_edges_and_a_second_scan_group at N = 1 (its smallest) and 65

def _refine_cfg(side, thr=0.3, max_instances=100):
    import types
    return types.SimpleNamespace(IMAGE_SHAPE=np.array([side, side, 3]), DETECTION_NMS_THRESHOLD=thr, DETECTION_MAX_INSTANCES=max_instances)


@functools.lru_cache(maxsize=None)
def _refine_data(N):
    """The sibling test's draws: _boxes(rng, N, max(1, N // 6)), then _word_scores(rng, N, 15)."""
    from image_captioning_amd import dense_model
    rng = np.random.default_rng(100 + N)
    nclu = max(1, N // 6)
    cc, hw = rng.uniform(0.02, 0.98, (nclu, 2)), rng.uniform(0.04, 0.3, (nclu, 2))
    which = rng.integers(0, nclu, N)
    ctr = cc[which] + 0.15 * hw[which] * rng.standard_normal((N, 2))
    size = hw[which] * np.exp(0.25 * rng.standard_normal((N, 2)))
    rois = np.concatenate([ctr - 0.5 * size, ctr + 0.5 * size], axis=1).astype(np.float32)[None]
    ws = rng.uniform(0.05, 1.0, (N, 15)).astype(np.float32)
    cfg, window, shape = _refine_cfg(320), (40, 0, 280, 320), (300, 400, 3)
    consts = np.stack([dense_model.refine_constants(window, cfg, shape)]).reshape(1, -1)
    return {"rois": rois, "ws": ws, "cfg": cfg, "window": window, "shape": shape, "consts": consts}


def _refine(N):
    M = 100

    def fill(d, N_):
        d.B, d.N, d.T, d.threshold, d.max_instances = 1, N_, 15, 0.3, M

    def need(lib):
        d = _desc(_L().RefineDesc, ("rois", "word_scores", "image_consts", "boxes_out", "keep_out", "count_out", "scores_out"))
        fill(d, N)
        return lib.dc_refine_generations_workspace_bytes(C.byref(d))

    def body(c):
        torch = _torch()
        g = _refine_data(N)
        rois, ws, consts = PC.dev(g["rois"]), PC.dev(g["ws"]), PC.dev(g["consts"], torch.float64)
        with c.call("dc_refine_generations_f64"):
            if c.live:                       # the wrapper allocates its outputs: the same call from the descriptor, into watched ones
                d = _L().RefineDesc()
                fill(d, N)
                d.rois, d.word_scores, d.image_consts = rois.data_ptr(), ws.data_ptr(), consts.data_ptr()
                d.boxes_out, d.keep_out = c.out("boxes", 1, M, 4, dtype=torch.int32).data_ptr(), c.out("keep", 1, M, dtype=torch.int32).data_ptr()
                d.count_out, d.scores_out = c.out("count", 1, dtype=torch.int32).data_ptr(), c.out("scores", 1, N, dtype=torch.float64).data_ptr()
                c.ops._launch_ws(c.lib.dc_refine_generations_workspace_bytes(C.byref(d)), rois.device, c.lib.dc_refine_generations_f64, C.byref(d))
            else:
                out = c.ops.refine_generations(rois, consts, 0.3, M, word_scores=ws)
                c.t.update(zip(("boxes", "keep", "count", "scores"), out))

    def check(t):
        from image_captioning_amd import dense_model
        g = _refine_data(N)
        boxes, keep, count, scores = (t[k].cpu().numpy() for k in ("boxes", "keep", "count", "scores"))
        want_s = np.log(g["ws"].astype(np.float64)).sum(1)
        assert np.all(np.abs(scores.reshape(-1) - want_s) <= 1e-12 * np.maximum(1.0, np.abs(want_s)))
        hb, hk = dense_model.refine_generations(g["rois"][0], None, g["window"], g["cfg"], caption_scores=scores[0])
        final, ok = dense_model.unmold_generations(hb, g["shape"], g["window"])
        want_boxes, want_keep = final[ok], hk[ok]
        n = len(want_keep)
        assert count[0] == n
        assert np.array_equal(keep[0, :n], want_keep) and np.all(keep[0, n:] == -1)
        assert np.array_equal(boxes[0, :n], want_boxes) and np.all(boxes[0, n:] == 0)

    case("refine_generations-N%d" % N, ["dc_refine_generations_f64"], need, check)(body)


_refine(1)
_refine(65)          # the second word of the mask


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_rpn_targets_f64: test_random_boxes_equal_the_host_function at G = 1, budget 16 on the 128 x 128 pyramid

RT_STD = (0.1, 0.1, 0.2, 0.2)


@functools.lru_cache(maxsize=None)
def _rt_data(G, budget):
    import _rpn_targets_ref as R
    anchors, sizes = R.pyramid(128)
    boxes = [R.random_boxes(10 + G, G, 128)]
    with np.errstate(divide="ignore"):
        want = R.host_packed(anchors, boxes, sizes, budget, 77, 5, RT_STD)
    return anchors, sizes, boxes, want


def _rpn_targets(G, budget):
    def need(lib):
        anchors, sizes, _, _ = _rt_data(G, budget)
        d = _desc(_L().RpnTargetsDesc, ("anchors", "gt_boxes", "gt_counts", "counts", "sel_level", "sel_index", "sel_match", "deltas"), B=1,
                  A=anchors.shape[0], n_levels=len(sizes), gt_capacity=G, budget=budget)
        for i, v in enumerate(sizes):
            d.level_sizes[i] = int(v)
        return lib.dc_rpn_targets_workspace(C.byref(d))

    def body(c):
        torch = _torch()
        anchors, sizes, boxes, _ = _rt_data(G, budget)
        ad = PC.dev(anchors, torch.float64)
        gt = PC.dev(np.asarray(boxes[0], np.float64).reshape(1, G, 4), torch.float64)
        counts = PC.dev([G], torch.int32)
        with c.call("dc_rpn_targets_f64"):
            out = (c.out("counts", 2, dtype=torch.int32), c.out("lvl", budget, dtype=torch.int32), c.out("idx", budget, dtype=torch.int32),
                   c.out("mt", budget, dtype=torch.int32), c.out("deltas", budget, 4))
            c.ops.rpn_targets(ad, gt, counts, sizes, budget, RT_STD, 77, offset=5, out=out)

    def check(t):
        want = _rt_data(G, budget)[3]
        got = {k: t[k].cpu().numpy() for k in ("counts", "lvl", "idx", "mt", "deltas")}
        n_sel, n_pos = int(want["counts"][0]), int(want["counts"][1])          # test_gpu_rpn_targets.check
        assert got["counts"].tolist() == [n_sel, n_pos]
        for k in ("lvl", "idx", "mt"):
            assert np.array_equal(got[k][:n_sel], want[k]), k
            assert not got[k][n_sel:].any(), k + " tail"
        a, b = np.asarray(got["deltas"][:n_pos], np.float32), np.asarray(want["deltas"], np.float32)
        ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
        ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
        assert ia.size == 0 or np.abs(ia - ib).max() <= 1
        assert not got["deltas"][n_pos:].any()

    case("rpn_targets-G%d-budget%d" % (G, budget), ["dc_rpn_targets_f64"], need, check)(body)


_rpn_targets(1, 16)


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_resize_pad_u8 / dc_resize_pad_flip_u8: the 10 x 12 image placed as (20, 24, 6, 4) on the 32 x 32 canvas

RESIZE_PLACE, RESIZE_CANVAS = (20, 24, 6, 4), (32, 32)


@functools.lru_cache(maxsize=None)
def _resize_image():
    img = np.random.default_rng(4).integers(0, 256, (10, 12, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


def _resize(flip):
    sym = "dc_resize_pad_flip_u8" if flip else "dc_resize_pad_u8"
    flips = [True] if flip else None

    def need(lib):
        from image_captioning_amd import ops
        packed, rec = ops.pack_resize_batch([_resize_image()], [RESIZE_PLACE], flips)
        d = _desc(_L().ResizePadDesc, ("packed", "out"), B=1, packed_bytes=packed.size, records=rec.ctypes.data, H=RESIZE_CANVAS[0], W=RESIZE_CANVAS[1])
        return lib.dc_resize_pad_u8_workspace_bytes(C.byref(d))

    def body(c):
        torch = _torch()
        packed, rec = c.ops.pack_resize_batch([_resize_image()], [RESIZE_PLACE], flips)
        pd = torch.from_numpy(packed).to("cuda")
        with c.call(sym):
            c.ops.resize_pad_packed(pd, rec, out=c.out("canvas", 1, RESIZE_CANVAS[0], RESIZE_CANVAS[1], 3, dtype=torch.uint8), flips=flips)

    def check(t):
        import _resize_ref as R
        nh, nw, top, left = RESIZE_PLACE
        want = R.padded(R.pil_resize(_resize_image(), nh, nw), RESIZE_CANVAS[0], RESIZE_CANVAS[1], top, left)
        assert np.array_equal(t["canvas"].cpu().numpy()[0], want[:, ::-1] if flip else want)

    case("resize_pad%s-10x12-to-20x24" % ("_flip" if flip else ""), [sym], need, check)(body)


_resize(False)
_resize(True)


# ---------------------------------------------------------------------------------------------------------------------------------
# dc_mask_paste_u8: _detect_cases' smallest image (40 x 50, twelve detections of a 64 x 1 mask)

PASTE = "taps_64x1"


def _paste_need(lib):
    import _detect_cases as K
    p = K.paste_case(PASTE)
    d = _desc(_L().MaskPasteDesc, ("masks", "boxes", "out"), M=p.M, h=p.masks.shape[1], w=p.masks.shape[2], H=p.H, W=p.W)
    return lib.dc_mask_paste_u8_workspace_bytes(C.byref(d))


def _paste_check(t):
    import _detect_cases as K
    assert np.array_equal(t["out"].cpu().numpy(), K.paste_case(PASTE).reference())


@case("mask_paste-" + PASTE, ["dc_mask_paste_u8"], _paste_need, _paste_check)
def _(c):
    import _detect_cases as K
    torch = _torch()
    p = K.paste_case(PASTE)
    masks, boxes = PC.dev(p.masks), PC.dev(p.boxes, torch.int32)
    with c.call("dc_mask_paste_u8"):
        c.ops.mask_paste(masks, boxes, p.H, p.W, out=c.out("out", p.M, p.H, p.W, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------------------------------------
# the reductions of loss.hip

@functools.lru_cache(maxsize=None)
def _colsum_data(M, N):
    """Multiples of 1/8 within +-1: every partial sum is a multiple of 1/8 below M <= 2^13, exact in float32 in any order -- the chunked
    sum and the one-chunk fallback of a short workspace both give the float64 column sums."""
    x = PC.grid(np.random.default_rng(M + N), (M, N), 1 / 8, 1.0)
    return x, PC.assert_exact_f32(x.sum(0), "the column sums")


def _colsum(M, N):
    def need(lib):
        return lib.dc_colsum_workspace_bytes(M, N, N)

    def body(c):
        x = PC.dev(_colsum_data(M, N)[0])
        with c.call("dc_colsum_f32"):
            c.ops.colsum(x, out=c.out("sums", N))

    def check(t):
        equal(t["sums"], _colsum_data(M, N)[1], "column sums")

    case("colsum-%dx%d" % (M, N), ["dc_colsum_f32"], need, check, serves_short=(0,))(body)


_colsum(512, 20)           # 4 chunks
_colsum(5000, 20)


@functools.lru_cache(maxsize=None)
def _vector_data(n):
    rng = np.random.default_rng(n)
    return rng.standard_normal(n), rng.random(n) * (rng.random(n) < 0.7), rng.standard_normal(n)


def _sumsq_need(lib):
    return lib.dc_sumsq_workspace_bytes(10007)


def _sumsq_check(t):
    x = _vector_data(10007)[0].astype(np.float32).astype(np.float64)
    close(t["out"], np.array([(x ** 2).sum()]), 1e-5, "sumsq")


@case("sumsq-10007", ["dc_sumsq_f32"], _sumsq_need, _sumsq_check)
def _(c):
    x = PC.dev(_vector_data(10007)[0])
    with c.call("dc_sumsq_f32"):
        c.ops.sumsq(x, out=c.out("out", 1))


def _l2_need(lib):
    return lib.dc_l2_reg_workspace_bytes(5000)


def _l2_check(t):
    wv, coef, g = _vector_data(5000)
    close(t["grad"], g + 2 * coef * wv, 1e-6, "grad")
    close(t["loss"], np.array([(coef * wv * wv).sum()]), 1e-5, "loss")


@case("l2_reg-5000-loss", ["dc_l2_reg_f32"], _l2_need, _l2_check)
def _(c):
    wv, coef, g = _vector_data(5000)
    w, cf = PC.dev(wv), PC.dev(coef)
    with c.call("dc_l2_reg_f32"):
        c.ops.l2_reg(w, cf, c.out("grad", 5000, init=g), c.out("loss", 1))


def _reg_sumsq(name):
    def need(lib):
        import _reg_segment_cases as RS
        return lib.dc_reg_sumsq_workspace_bytes(RS.build(name).n)

    def body(c):
        import _reg_segment_cases as RS
        rc = RS.build(name)
        w_h, g_h = RS.sparse_data(name)
        segs = c.ops.RegSegmentTable(rc.coef, rc.mask if rc.nseg > 1 else None, "cuda")
        w, g = PC.dev(w_h), PC.dev(g_h)
        with c.call("dc_reg_sumsq_f32"):
            c.ops.reg_sumsq(w, g, segs, loss=c.out("loss", 1), gnorm_sq=c.out("gnorm_sq", 1))

    def check(t):
        import _reg_segment_cases as RS
        rc = RS.build(name)
        w_h, g_h = RS.sparse_data(name)
        loss, norm, units = RS.reg_sums(w_h, g_h, rc.coef, rc.mask)
        assert units < 2 ** 24
        assert float(t["loss"].item()) == loss and float(t["gnorm_sq"].item()) == norm

    case("reg_sumsq-" + name, ["dc_reg_sumsq_f32"], need, check)(body)


_reg_sumsq("small")        # (the sibling's small table: 10 007 elements, one pass)
_reg_sumsq("one")          # 4 S + 1 elements: five passes of the capped grid


def symbols():
    return sorted({s for c in CASES for s in c.symbols})
