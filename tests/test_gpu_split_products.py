"""Every split-bf16 kernel held to its six piece products (-m gpu).

The 2e-5 max-norm tolerance of the other split-bf16 tests cannot tell the six-product arithmetic from one that lost a third-order product
(2^-18 of a product), reads a stale third piece at some positions or runs on two pieces.  Here the error got - want of every kernel is
projected on the float64 contribution D_ij of each piece product (tests/_split_cases.py; tests/test_split_cases.py proves the instrument
on emulated arithmetic): c_ij is 0 for a product the kernel sums once, -1 for a missing one, +1 for one counted twice -- over the whole
output and over every 32-channel block or work item, so a product missing on an eighth of a stratum's work moves its c by 0.125.

The bound 0.1 is derived, not measured: the noise of c is r / sqrt(n) with r the ratio of fp32 accumulation noise to one third-order term
(at most 1 up to K = 4608) and n >= 1024 outputs per stratum, so at most 0.03.  relu is off everywhere (it breaks the linearity); scale,
shift and residual stay on, they are affine and part of `want`.  Outputs start as NaN.  Every test prints a `split-products` line with
its largest |c| and the max-norm errors of the split-bf16 kernel and of its exact-fp32 sibling against float64 (DESIGN.md has the table)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _split_cases as S
from test_gpu_kernels import _wino_items_per_block

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 0.1
MATHS = [(1, "bf16x3"), (2, "bf16x2"), (3, "bf16"), (0, "f32")]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def dev(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def nans(shape):
    return torch.full(tuple(shape), float("nan"), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def maxnorm(got, prob):
    idx = Ellipsis if prob.whole is None else prob.whole
    return float(np.abs(got.astype(np.float64) - prob.want)[idx].max()) / max(1.0, float(np.abs(prob.want[idx]).max()))


def judge(name, kernel, prob, got, arithmetic, sibling=None):
    """The coefficient assertions of one launch.  arithmetic: 'bf16x3' / 'f32' (every kept product once), 'bf16x2' (the three third-order
    products missing, no more and no less), 'bf16' (one piece).  sibling: the exact-fp32 kernel's output, for the record."""
    got = np.asarray(got)
    assert np.isfinite(got[Ellipsis if prob.whole is None else prob.whole]).all(), "%s: the launch left outputs unwritten" % name
    if prob.whole is not None:
        assert np.isnan(got[~prob.whole]).all(), "%s: wrote outside the listed groups" % name
    c = S.coefficients(got, prob.want, prob.D, prob.strata, prob.whole)
    present = {"bf16x3": S.KEPT, "f32": S.KEPT, "bf16x2": S.SECOND, "bf16": ()}[arithmetic]
    missing = {"bf16x3": (), "f32": (), "bf16x2": S.THIRD, "bf16": S.SECOND}[arithmetic]
    err = maxnorm(got, prob)
    w = S.worst(c, present) if present else (0.0, "-", "-")
    print("split-products | %s | %s | %s | K %d | largest |c| %.4f (%s, %s) | max-norm %.2e | fp32 sibling %s" %
          (name, kernel, arithmetic, prob.K, w[0], w[1], w[2], err, "-" if sibling is None else "%.2e" % maxnorm(np.asarray(sibling), prob)))
    if missing:
        print("split-products | %s | missing products: %s" % (name, {ij: round(c["all"][ij], 4) for ij in missing}))
    assert w[0] <= BOUND, "%s (%s): c%s = %.4f in stratum '%s'" % (name, kernel, w[2], c[w[1]][w[2]], w[1])
    for sname, v in c.items():
        for ij in missing:
            assert -1.1 <= v[ij] <= -0.9, "%s (%s): c%s = %.4f in stratum '%s', the arithmetic drops this product: -1" % (name, kernel, ij, v[ij], sname)
    if arithmetic in ("bf16x3", "f32"):
        assert err < 2e-5, "%s (%s): max-norm error %.3e" % (name, kernel, err)
    return c


# ---------------------------------------------------------------------------------------------------------------- igemm_bs_kernel

def _expect_bs(info, math, tile, split_k):
    if math == 0:
        assert not info["kernel"].startswith("igemm_bs_kernel"), info
    else:
        assert info["kernel"] == "igemm_bs_kernel<%d, %d>" % tile and info["tile"] == tile and info["split_k"] == split_k, info


@pytest.mark.parametrize("math,arithmetic", MATHS, ids=[m[1] for m in MATHS])
@pytest.mark.parametrize("name", sorted(S.CONV))
def test_conv2d_piece_products(ops, name, math, arithmetic):
    o, prob = S.conv_case(name)
    args = (dev(o["x"]), dev(o["w"]), o["k"], o["k"], o["stride"], o["pad"], o["pad"], o["Ho"], o["Wo"], dev(o["scale"]), dev(o["shift"]),
            dev(o["residual"]), o["res_mode"], False)
    info = {}
    got = host(ops.conv2d(*args, out=nans(prob.out_shape), math=math, info=info))
    _expect_bs(info, math, o["tile"], o["split_k"])
    sibling = host(ops.conv2d(*args, out=nans(prob.out_shape), math=0)) if math == 1 else None
    judge("conv " + name, info["kernel"], prob, got, arithmetic, sibling)


@pytest.mark.parametrize("math,arithmetic", MATHS, ids=[m[1] for m in MATHS])
def test_stem_piece_products(ops, math, arithmetic):
    """The 7x7 / stride 2 stem on the uint8 image through mold_image_rgbx: the StemKC loader (K = 7 rows of 8 taps x RGBX)."""
    o, prob = S.stem_case()
    rgbx = ops.mold_image_rgbx(dev(o["img"], torch.uint8), S.MEAN_PIXEL)
    assert np.array_equal(host(rgbx), o["x"])              # the operand the kernel splits is the one the host split
    args = (rgbx, dev(o["w"]), 7, 7, 2, 3, 3, o["Ho"], o["Wo"], dev(o["scale"]), dev(o["shift"]), None, 0, False)
    info = {}
    got = host(ops.conv2d(*args, out=nans(prob.out_shape), math=math, info=info))
    _expect_bs(info, math, o["tile"], o["split_k"])
    sibling = host(ops.conv2d(*args, out=nans(prob.out_shape), math=0)) if math == 1 else None
    judge(S.STEM[0], info["kernel"], prob, got, arithmetic, sibling)


def _group_list(groups, capacity):
    lst = torch.zeros(capacity, dtype=torch.int32, device="cuda")
    lst[:len(groups)] = torch.tensor(list(groups), dtype=torch.int32)
    return lst, torch.tensor([len(groups)], dtype=torch.int32, device="cuda")


def test_conv2d_tiles_piece_products(ops):
    """The list-driven 128 x 128 kernel on half the tile groups of the map: coefficients on the listed groups only."""
    o, prob = S.tiles_case()
    N, H, W, Cout = prob.out_shape
    lst, count = _group_list(o["groups"], N * S.group_count(H, W))
    x, w, sc, sh, res = dev(o["x"]), dev(o["w"]), dev(o["scale"]), dev(o["shift"]), dev(o["residual"])
    dense = (x, w, 1, 1, 1, 0, 0, H, W, sc, sh, res, 2, False)
    assert ops.conv2d_kernel_name(*dense, split_k=1, math=1) == "igemm_bs_kernel<128, 128>"
    got = host(ops.conv2d_tiles(x, w, lst, count, nans(prob.out_shape), sc, sh, res, 2, False))
    sibling = np.where(prob.whole, host(ops.conv2d(*dense, math=0)), np.nan)
    judge(S.TILES[0], "igemm_bs_kernel<128, 128> (tile list)", prob, got, "bf16x3", sibling)
    judge(S.TILES[0] + " control", "dense fp32", prob, sibling, "f32")


# ---------------------------------------------------------------------------------------------------------------- Winograd

def _wino_args(ops, o):
    N, H, W, Cin, Cout = o["shape"]
    return (dev(o["x"]), dev(o["w"]), 3, 3, 1, 1, 1, H, W, dev(o["scale"]), dev(o["shift"]), None, 0, False)


@pytest.mark.parametrize("name", sorted(S.WINO))
def test_winograd_b3_piece_products(ops, name):
    o, prob = S.wino_case(name)
    N, H, W, Cin, Cout = o["shape"]
    if name == S.WINO_MULTI:                               # 32-tile items on 512 persistent blocks: some block takes two
        items, per_block = _wino_items_per_block(N, H, W, Cout, 32)
        assert Cin <= 64 and items > 512 and per_block > 1.0 and Cout % 64 != 0
        second = {"item slice %d group %d" % sg for sg in S.wino_second_items(prob.out_shape)}
        assert len(second) == items - 512 and second & {s for s, _ in prob.strata}
    args = _wino_args(ops, o)
    info = {}
    got = host(ops.conv2d(*args, out=nans(prob.out_shape), w_wino_b3=ops.winograd_pack_b3(args[1], Cin, Cout), info=info))
    assert info["kernel"] == "wino32b_kernel"
    finfo = {}
    sibling = host(ops.conv2d(*args, out=nans(prob.out_shape), w_wino=ops.winograd_pack(args[1], Cin, Cout), info=finfo))
    assert finfo["kernel"] in ("wino32_kernel", "wino64_kernel")
    judge("wino " + name, info["kernel"], prob, got, "bf16x3", sibling)
    judge("wino %s control" % name, finfo["kernel"], prob, sibling, "f32")


_CHILD = r"""
import sys
import numpy as np, torch
from image_captioning_amd import ops
src, dst = sys.argv[1], sys.argv[2]
data = np.load(src)
outs, names = {}, []
for k in range(int(data["count"])):
    x, w, sc, sh = [torch.tensor(data["%s%d" % (f, k)], device="cuda") for f in ("x", "w", "scale", "shift")]
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    args = (x, w, 3, 3, 1, 1, 1, H, W, sc, sh, None, 0, False)
    u = ops.winograd_pack_b3(w, Cin, Cout)
    names.append(ops.conv2d_kernel_name(*args, w_wino_b3=u))
    out = torch.full((N, H, W, Cout), float("nan"), device="cuda")
    outs["y%d" % k] = ops.conv2d(*args, out=out, w_wino_b3=u).cpu().numpy()
torch.cuda.synchronize()
np.savez(dst, names=np.array(names), **outs)
"""


@pytest.mark.parametrize("var,value,kernel", [("DCAP_WINO_TILES", "64", "wino64b_kernel"), ("DCAP_WINO_COUT", "32", "wino32b_kernel"),
                                              ("DCAP_WINO_COUT", "64", "wino32b_kernel")], ids=["tiles64", "cout32", "cout64"])
def test_winograd_b3_forced_kernels_piece_products(ops, tmp_path, var, value, kernel):
    """wino64b_kernel and the 32- / 64-channel items of wino32b_kernel, each forced in a child process of its own (the switches are read
    once per process); the child saves its outputs, the parent judges them."""
    names = sorted(S.WINO)
    data = {"count": len(names)}
    for k, n in enumerate(names):
        o = S.wino_case(n)[0]
        data.update({"x%d" % k: o["x"], "w%d" % k: o["w"], "scale%d" % k: o["scale"], "shift%d" % k: o["shift"]})
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **data)
    env = dict(os.environ, **{var: value})
    r = subprocess.run([sys.executable, "-c", _CHILD, src, dst], env=env, cwd=ROOT, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    res = np.load(dst)
    assert list(res["names"]) == [kernel] * len(names)
    for k, n in enumerate(names):
        judge("wino %s %s=%s" % (n, var, value), kernel, S.wino_case(n)[1], res["y%d" % k], "bf16x3")


def test_winograd_groups_piece_products(ops):
    """wino32b_list_kernel on a partial, unordered list: coefficients on the listed groups."""
    o, prob = S.wino_groups_case()
    N, H, W, Cin, Cout = o["shape"]
    args = _wino_args(ops, o)
    u = ops.winograd_pack_b3(args[1], Cin, Cout)
    lst, count = _group_list(o["groups"], N * S.group_count(H, W))
    got = host(ops.conv2d_winograd_groups(args[0], args[1], u, lst, count, nans(prob.out_shape), args[9], args[10], False))
    sibling = np.where(prob.whole, host(ops.conv2d(*args, w_wino=ops.winograd_pack(args[1], Cin, Cout))), np.nan)
    judge("wino " + S.WINO_GROUPS[0], "wino32b_list_kernel", prob, got, "bf16x3", sibling)


def test_winograd_levels_piece_products(ops):
    """wino32b_levels_kernel: two levels' lists in one launch."""
    cases = S.wino_levels_case()
    xs, ws, us, lists, outs, scs, shs = [], [], [], [], [], [], []
    counts = torch.zeros(len(cases), dtype=torch.int32, device="cuda")
    for l, (o, prob) in enumerate(cases):
        N, H, W, Cin, Cout = o["shape"]
        xs.append(dev(o["x"])), ws.append(dev(o["w"])), scs.append(dev(o["scale"])), shs.append(dev(o["shift"]))
        us.append(ops.winograd_pack_b3(ws[-1], Cin, Cout))
        lst, cnt = _group_list(o["groups"], N * S.group_count(H, W))
        lists.append(lst)
        counts[l:l + 1] = cnt
        outs.append(nans(prob.out_shape))
    ops.conv2d_winograd_levels(xs, ws, us, lists, counts, outs, scs, shs, False)
    for l, (o, prob) in enumerate(cases):
        sibling = np.where(prob.whole, host(ops.conv2d(*_wino_args(ops, o), w_wino=ops.winograd_pack(ws[l], *o["shape"][3:]))), np.nan)
        judge("wino %s %d" % (S.WINO_LEVELS[0], l), "wino32b_levels_kernel", prob, host(outs[l]), "bf16x3", sibling)


# ---------------------------------------------------------------------------------------------------------------- pw_chain_kernel

def _chain_kernel_name(shape, w1f, w2f):
    from image_captioning_amd import _lib
    d = _lib.PwChainDesc()
    d.M, d.K1, d.N1, d.N2 = shape
    if w1f.dtype == torch.int16:
        d.w1_b3, d.w2_b3 = w1f.data_ptr(), w2f.data_ptr()
    buf = C.create_string_buffer(64)
    _lib.check(_lib.load().dc_pw_chain_kernel_name(C.byref(d), buf, 64), "dc_pw_chain_kernel_name")
    return buf.value.decode()


def _run_chain(ops, name, shape, pack):
    o = S.chain_operands(name)
    M, K1, N1, N2 = shape
    w1f, w2f = pack(dev(o["w1"])), pack(dev(o["w2"]))
    y, z = ops.pw_chain(dev(o["x"]), w1f, dev(o["shift1"]), w2f, dev(o["shift2"]), scale1=dev(o["scale1"]), scale2=dev(o["scale2"]),
                        residual=dev(o["residual"]), relu1=False, relu2=False, y=nans((M, N1)), z=nans((M, N2)))
    return _chain_kernel_name(shape, w1f, w2f), host(y), host(z)


@pytest.mark.parametrize("name", sorted(S.CHAIN))
def test_pw_chain_piece_products(ops, name):
    """Both layers of pw_chain_kernel<.., true>; layer 2 on the fp32 y the kernel itself wrote -- the operand it split."""
    shape = S.CHAIN[name]
    kernel, y, z = _run_chain(ops, name, shape, ops.pw_chain_pack_b3)
    assert kernel == "pw_chain_kernel<%d, %d, true>" % (shape[2] // 256, shape[3] // 32)
    fkernel, fy, fz = _run_chain(ops, name, shape, ops.pw_chain_pack)
    assert fkernel == "pw_chain_kernel<%d, %d, false>" % (shape[2] // 256, shape[3] // 32)
    p1 = S.chain_layer1(name)
    judge("chain %s layer 1" % name, kernel, p1, y, "bf16x3", fy)
    judge("chain %s layer 1 control" % name, fkernel, p1, fy, "f32")
    judge("chain %s layer 2" % name, kernel, S.chain_layer2(name, y), z, "bf16x3")
    judge("chain %s layer 2 control" % name, fkernel, S.chain_layer2(name, fy), fz, "f32")


def test_pw_chain_stream_control(ops):
    """The 64 -> 256 -> 64 stream form takes fp32 products only: the instrument's noise floor on it."""
    name, shape = S.CHAIN_STREAM
    kernel, y, z = _run_chain(ops, name, shape, ops.pw_chain_pack)
    assert kernel == "pw_chain_stream_kernel<64, 256, 64>"
    judge("chain %s layer 1 control" % name, kernel, S.chain_layer1(name), y, "f32")
    judge("chain %s layer 2 control" % name, kernel, S.chain_layer2(name, y), z, "f32")


# ---------------------------------------------------------------------------------------------------------------- the packs, bit for bit

def _planes(t):
    return host(t).view(np.uint16)


def test_winograd_pack_b3_is_the_split_of_the_fp32_pack(ops):
    Cin, Cout = 64, 96
    w = dev(S.pack((S._rng("wino pack").standard_normal((3, 3, Cin, Cout)) / 24.0).astype(np.float32)))
    NTG, KC = Cout // 32, Cin // 16
    # fp32: f4 index ((((xi NTG + ntg) KC + kc) 2 + j) 64 + 32 h + i), component e  <->  cout = 32 ntg + i, cin = 16 kc + 8 h + 4 j + e
    u = host(ops.winograd_pack(w, Cin, Cout)).reshape(16, NTG, KC, 2, 2, 32, 4)             # xi, ntg, kc, j, h, i, e
    u = u.transpose(0, 1, 5, 2, 4, 3, 6).reshape(16, Cout, Cin)
    # b3: ushort index (((((xi NTG + ntg) KC + kc) 3 + piece) 64 + 32 h + i) 8 + jj)  <->  cout = 32 ntg + i, cin = 16 kc + 8 h + jj
    b = _planes(ops.winograd_pack_b3(w, Cin, Cout)).reshape(16, NTG, KC, 3, 2, 32, 8)       # xi, ntg, kc, piece, h, i, jj
    b = b.transpose(3, 0, 1, 5, 2, 4, 6).reshape(3, 16, Cout, Cin)
    assert np.array_equal(b, S.bf16_bits(S.split3(u)))
    hostU = S.wino_U(host(w).reshape(Cout, 3, 3, Cin).transpose(1, 2, 3, 0)).reshape(16, Cin, Cout).transpose(0, 2, 1)
    assert np.abs(u - hostU).max() <= 2.0 ** -22 * np.abs(hostU).max()                      # the same U up to the sums' last bits


def test_pw_chain_pack_b3_is_the_split_of_the_fp32_pack(ops):
    N, K = 128, 160
    wh = (S._rng("chain pack").standard_normal((N, K)) / 12.0).astype(np.float32)
    w = dev(wh)
    # fp32: f4 index ((cb K/8 + g) 64 + 32 h + i), component e  <->  w[32 cb + i][8 g + 4 h + e]
    f = host(ops.pw_chain_pack(w)).reshape(N // 32, K // 8, 2, 32, 4).transpose(0, 3, 1, 2, 4).reshape(N, K)
    assert np.array_equal(f, wh)
    # b3: ushort index ((((cb K/16 + g) 3 + piece) 64 + 32 h + i) 8 + jj)  <->  w[32 cb + i][16 g + 8 h + jj]
    b = _planes(ops.pw_chain_pack_b3(w)).reshape(N // 32, K // 16, 3, 2, 32, 8).transpose(2, 0, 4, 1, 3, 5).reshape(3, N, K)
    assert np.array_equal(b, S.bf16_bits(S.split3(f)))


def test_split_bf16x3_is_split3(ops):
    rng = np.random.default_rng(3)                         # the vector of test_gpu_kernels.py::test_split_bf16x3_pieces
    x = (rng.standard_normal(4097) * np.exp(rng.uniform(-20, 20, 4097))).astype(np.float32)
    x[:4] = [0.0, 1.0, -2.5, 2.0 ** -120]
    assert np.array_equal(_planes(ops.split_bf16x3(dev(x))), S.bf16_bits(S.split3(x)))
