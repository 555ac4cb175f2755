"""The detection kernels of csrc/detect.hip on the device (-m gpu) at the sizes where their grids and loops wrap: a second and third
256-wide x block and a second grid-stride pass of mask_paste, its longest tap windows and bytescale's edges; mask_head_tail at P = 1 and
16, Cin and Cmid off the powers of two, row counts on and just past the 128-row block, invalid class ids on a wave's first and last
lane, the next wave's first lane and the last valid row; class_select at one, two, three and four passes of its lane loop with planted ties and -inf logits.

The cases are tests/_detect_cases.py's, proven to hold their edges by tests/test_detect_cases.py on the CPU.  References and bounds are
the existing ones: mask_paste bit for bit against mask_rcnn_model.unmold_mask (PIL), mask_head_tail against _maskrcnn_ref.mask_tail
within mask_tail_tol, class_select against _maskrcnn_ref.class_select within (d_max + C + 8) u with ids and deltas exact.  Out of scope:
NaN anywhere, +inf logits, rows of nothing but -inf, masks with subnormal values or a range below 1e-30 (see _detect_cases.py)."""
import numpy as np
import pytest
import torch

import _detect_cases as K
import _maskrcnn_ref as R
from _detect_device import dev, run_tail

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


# ---- class_select ------------------------------------------------------------------------------------------------------------------
def check_select(ops, z, d, label):
    """Contiguous and with padded row strides (1e30 in the logits' padding): ids and deltas exact, scores within (d_max + C + 8) u with
    d_max the largest FINITE gap, the same bits both ways and on a second call.  Returns (ids, scores)."""
    R_, C = z.shape
    ldz, ldd = C + 3, 4 * C + 8
    zs, ds = np.full((R_, ldz), 1e30, np.float32), np.full((R_, ldd), 7.0, np.float32)
    zs[:, :C], ds[:, :4 * C] = z, d
    want_ids, want_scores, want_d, _ = R.class_select(z, d)
    d_max = K.select_finite_gap(z)
    tol = (d_max + C + 8) * U
    res = []
    for zt, dt in ((dev(z), dev(d)), (dev(zs)[:, :C], dev(ds)[:, :4 * C]), (dev(z), dev(d))):
        ids, scores, deltas = (t.cpu().numpy() for t in ops.class_select(zt, dt))
        assert ids.dtype == np.int32 and ids.shape == (R_,) and scores.shape == (R_,) and deltas.shape == (R_, 4)
        assert np.array_equal(ids, want_ids), (label, np.flatnonzero(ids != want_ids)[:8])
        assert np.array_equal(deltas.view(np.int32), want_d.view(np.int32))
        rel = np.abs(scores.astype(np.float64) - want_scores) / want_scores
        if not res:
            print("class_select %s R %d C %d: d_max %.1f, worst relative score error %.3e, bound %.3e" % (label, R_, C, d_max, rel.max(), tol))
        assert np.isfinite(scores).all() and (rel <= tol).all()
        res.append(scores)
    assert np.array_equal(res[0].view(np.int32), res[1].view(np.int32)), "the row strides changed the scores"
    assert np.array_equal(res[0].view(np.int32), res[2].view(np.int32)), "two calls differ"
    return want_ids, res[0]


@pytest.mark.parametrize("C", K.SELECT_C)
@pytest.mark.parametrize("R_", K.SELECT_R)
def test_class_select_lane_loop_and_block_edges(ops, R_, C):
    z, d = K.select_case(R_, C)
    ids, _ = check_select(ops, z, d, "sweep")
    assert ids[0] == 0 and ids[1] == C - 2
    if C > 70:
        assert ids[2] == 3 and ids[3] == 5


@pytest.mark.parametrize("C", K.SELECT_C)
def test_class_select_planted_rows(ops, C):
    """Maxima in the last pass only, ties across a lane's passes and across lanes, -inf logits (exp(-inf) = 0: the lone finite logit's
    score is exactly 1)."""
    z, d, names, want = K.select_planted(C)
    ids, scores = check_select(ops, z, d, "planted")
    assert ids.tolist() == want
    if "only_70_finite" in names:
        assert scores[names.index("only_70_finite")] == 1.0
    # the planted rows again as the rows of a second block's second wave: 5 rows of the sweep in front of them
    zf, df = K.select_case(5, C)
    ids2, scores2 = check_select(ops, np.concatenate([zf, z]), np.concatenate([df, d]), "planted after 5 rows")
    assert ids2[5:].tolist() == want and np.array_equal(scores2[5:].view(np.int32), scores.view(np.int32))


# ---- mask_head_tail ------------------------------------------------------------------------------------------------------------------
def check_tail(name, got):
    P, N, Cin, Cmid, C = K.TAIL_EDGES[name][:5]
    ids = K.tail_edge(name)[5].astype(np.int64)
    want, z, A = K.tail_reference(name)
    tol = R.mask_tail_tol(A, Cin, Cmid)
    assert got.shape == (N, 2 * P, 2 * P) and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - want)
    print("mask_head_tail %s P %d N %d Cin %d Cmid %d C %d: worst error %.3e, worst error / bound %.3f, |z| up to %.1f"
          % (name, P, N, Cin, Cmid, C, err.max(), (err / tol).max(), np.abs(z).max()))
    assert (err <= tol).all()
    bad = (ids < 0) | (ids >= C)
    assert not got[bad].view(np.int32).any()                             # exact zeros (+0.0) for every RoI whose class is out of range
    assert (got[~bad] > 0).all()                                         # |z| < 30: a float32 sigmoid never reaches 0 there
    return bad


@pytest.mark.parametrize("name", [n for n in K.TAIL_EDGES if n != "off_boundary"])
def test_mask_head_tail_edges(ops, name):
    """run_tail pre-fills `out` with NaN and asserts that two calls give the same bits."""
    bad = check_tail(name, run_tail(ops, K.tail_edge(name)))
    assert bad.sum() == {"lane_per_roi": 4, "all_invalid": 3, "invalid_first": 1, "invalid_last": 1}.get(name, 0)


def test_mask_head_tail_off_the_16_byte_boundary_at_96_channels(ops):
    """(7, 3, 96, 96, 5), signed x: x, wd and wm_t each 4 bytes past a 16-byte boundary (one at a time and all three) return the aligned
    call's bits, which are held to float64."""
    x, wd, bd, wm, bm, ids = K.tail_edge("off_boundary")
    base = [dev(x), dev(wd), dev(bd), dev(np.ascontiguousarray(wm.T)), dev(bm), dev(ids, torch.int32)]
    assert all(t.data_ptr() % 16 == 0 for t in (base[0], base[1], base[3]))
    want = ops.mask_head_tail(*base).cpu().numpy()
    check_tail("off_boundary", want)

    def off(t):
        buf = torch.zeros(t.numel() + 4, device="cuda")
        shift = 1 + (-(buf.data_ptr() // 4) % 4)                           # first element 4 bytes past a 16-byte boundary
        v = buf[shift:shift + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    for which in ((0,), (1,), (3,), (0, 1, 3)):
        args = [off(t) if i in which else t for i, t in enumerate(base)]
        got = ops.mask_head_tail(*args).cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), which


# ---- mask_paste ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.PASTE_NAMES)
def test_mask_paste_edges_equal_the_host_path(ops, name):
    """Bit for bit mask_rcnn_model.unmold_mask, with 0xFF guard bytes before and after `out` (every byte of out is written, none beyond)."""
    c = K.paste_case(name)
    want = c.reference()
    G, n = 4096, c.M * c.H * c.W
    buf = torch.full((n + 2 * G,), 0xFF, dtype=torch.uint8, device="cuda")
    out = buf[G:G + n].view(c.M, c.H, c.W)
    got = ops.mask_paste(dev(c.masks), dev(c.boxes, torch.int32), c.H, c.W, out=out)
    assert got is out
    host = buf.cpu().numpy()
    assert (host[:G] == 0xFF).all() and (host[G + n:] == 0xFF).all(), "guard bytes were written"
    got = host[G:G + n].reshape(c.M, c.H, c.W)
    for i in range(c.M):
        assert np.array_equal(got[i], want[i]), (name, c.labels[i], c.boxes[i].tolist(), int((got[i] != want[i]).sum()))
    fresh = ops.mask_paste(dev(c.masks), dev(c.boxes, torch.int32), c.H, c.W)
    assert fresh.dtype == torch.uint8 and np.array_equal(fresh.cpu().numpy(), got)
