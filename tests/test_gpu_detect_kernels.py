"""The three detection kernels on the device (-m gpu) against float64 / the host path: ops.class_select, ops.mask_head_tail,
ops.mask_paste (csrc/detect.hip).  References: tests/_maskrcnn_ref.py; mask_paste is held bit for bit to mask_rcnn_model.unmold_mask,
the host path detect(postprocess="host") runs."""
import numpy as np
import pytest
import torch

import _maskrcnn_ref as R
from _detect_cases import select_case, tail_case
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
@pytest.mark.parametrize("C", [2, 5, 81])
@pytest.mark.parametrize("R_", [1, 7, 1000])
def test_class_select(ops, R_, C):
    z, d = select_case(R_, C)
    ldz, ldd = C + 3, 4 * C + 8                                          # padded row strides, sentinel in the padding
    zs, ds = np.full((R_, ldz), 1e30, np.float32), np.full((R_, ldd), 7.0, np.float32)
    zs[:, :C], ds[:, :4 * C] = z, d
    want_ids, want_scores, want_d, d_max = R.class_select(z, d)
    tol = (d_max + C + 8) * U
    res = []
    for zt, dt in ((dev(z), dev(d)), (dev(zs)[:, :C], dev(ds)[:, :4 * C])):
        ids, scores, deltas = ops.class_select(zt, dt)
        assert ids.dtype == torch.int32 and tuple(ids.shape) == (R_,) and tuple(scores.shape) == (R_,) and tuple(deltas.shape) == (R_, 4)
        ids, scores, deltas = ids.cpu().numpy(), scores.cpu().numpy(), deltas.cpu().numpy()
        assert np.array_equal(ids, want_ids)                             # np.argmax: the lowest index of equal maxima
        assert np.array_equal(deltas.view(np.int32), want_d.view(np.int32))
        rel = np.abs(scores.astype(np.float64) - want_scores) / want_scores
        print("class_select R %d C %d: d_max %.1f, worst relative score error %.3e, bound %.3e" % (R_, C, d_max, rel.max(), tol))
        assert np.isfinite(scores).all() and (rel <= tol).all()
        res.append((ids, scores, deltas))
    assert np.array_equal(res[0][1].view(np.int32), res[1][1].view(np.int32))          # the stride changes nothing
    again = ops.class_select(dev(z), dev(d))
    assert np.array_equal(again[1].cpu().numpy().view(np.int32), res[0][1].view(np.int32))
    if C > 70 and R_ >= 4:
        assert want_ids[2] == 3 and want_ids[3] == 5                     # the planted ties resolved downwards
    assert want_ids[0] == 0


def test_class_select_3d_deltas_and_given_outputs(ops):
    z, d = select_case(7, 5)
    ids, scores, out = torch.zeros(7, dtype=torch.int32, device="cuda"), torch.zeros(7, device="cuda"), torch.zeros(7, 4, device="cuda")
    got = ops.class_select(dev(z), dev(d.reshape(7, 5, 4)), class_ids=ids, scores=scores, deltas_out=out)
    assert got[0] is ids and got[1] is scores and got[2] is out
    assert np.array_equal(ids.cpu().numpy(), R.class_select(z, d)[0])


# ---- mask_head_tail ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [5, 81])
@pytest.mark.parametrize("Cin,Cmid", [(256, 256), (64, 32)])
@pytest.mark.parametrize("N", [1, 3, 101])
def test_mask_head_tail(ops, N, Cin, Cmid, C):
    case = tail_case(N, Cin, Cmid, C)
    got = run_tail(ops, case)
    want, z, A = R.mask_tail(*case)
    tol = R.mask_tail_tol(A, Cin, Cmid)
    err = np.abs(got.astype(np.float64) - want)
    print("mask_head_tail N %d Cin %d Cmid %d C %d: worst error %.3e, worst error / bound %.3f, |z| up to %.1f"
          % (N, Cin, Cmid, C, err.max(), (err / tol).max(), np.abs(z).max()))
    assert np.isfinite(got).all() and (err <= tol).all()
    ids = case[5]
    bad = np.flatnonzero((ids < 0) | (ids >= C))
    assert len(bad) == (1 if N >= 3 else 0)
    for n in bad:
        assert not got[n].view(np.int32).any()                           # exact zeros for the RoI whose class is out of range ...
        assert (got[n - 1] > 0).all() and (got[n + 1] > 0).all()         # ... and its neighbours are untouched (checked against float64 above)
    assert 0 in ids or N == 1
    assert ids[-1] == C - 1


def test_mask_head_tail_off_the_16_byte_boundary_gives_the_same_bits(ops):
    """x, wd and wm_t each 4 bytes past a 16-byte boundary (one at a time and all three): the 4-byte-load instantiation runs and
    returns the aligned call's bits."""
    x, wd, bd, wm, bm, ids = tail_case(3, 64, 32, 5)
    ids[1] = 2
    base = [dev(x), dev(wd), dev(bd), dev(np.ascontiguousarray(wm.T)), dev(bm), dev(ids, torch.int32)]
    want = ops.mask_head_tail(*base).cpu().numpy()

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


def test_mask_head_tail_at_logits_near_200(ops):
    """Biases of +-200 on classes 0 and C - 1: the sigmoid stays finite and ordered."""
    case = tail_case(3, 64, 32, 5, big=True)
    x, wd, bd, wm, bm, ids = case
    ids[:] = [0, 2, 4]
    got = run_tail(ops, (x, wd, bd, wm, bm, ids))
    want, z, A = R.mask_tail(x, wd, bd, wm, bm, ids)
    print("|z| range of the +200 RoI [%.1f, %.1f], of the -200 RoI [%.1f, %.1f]" % (z[0].min(), z[0].max(), z[2].min(), z[2].max()))
    assert z[0].min() > 150 and z[2].max() < -150
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    assert (np.abs(got - want) <= R.mask_tail_tol(A, 64, 32)).all()
    assert (got[0] == 1.0).all() and (got[2] == 0.0).all() and got[0].min() >= got[1].max() and got[1].min() >= got[2].max()
    # monotone through the whole range: the same RoI under a sweep of the class bias
    sweep = np.array([-200.0, -120.0, -90.0, -30.0, -1.0, 0.0, 1.0, 30.0, 90.0, 120.0, 200.0], np.float32)
    xs = np.repeat(x[:1], len(sweep), axis=0)
    wm2, ids2 = np.repeat(wm[:, 2:3], len(sweep), axis=1), np.arange(len(sweep), dtype=np.int32)
    got = run_tail(ops, (xs, wd, bd, wm2, sweep, ids2))
    assert np.isfinite(got).all() and (np.diff(got, axis=0) >= 0).all() and got[0].max() == 0.0 and got[-1].min() == 1.0


# ---- mask_paste ------------------------------------------------------------------------------------------------------------------
H, W = 97, 131
BOXES = [
    (20, 30, 60, 70),        # 40 x 40
    (24, 33, 64, 93),        # overlaps the first
    (5, 7, 6, 8),            # 1 x 1
    (50, 3, 51, 43),         # 1 x 40
    (30, 40, 40, 45),        # 10 x 5: a downscale in both axes
    (2, 5, 92, 125),         # 90 x 120
    (70, 100, 97, 131),      # touches the bottom-right corner
    (10, 10, 10, 30),        # zero area
    (90, 120, 98, 131),      # leaves the image
    (0, 0, 33, 57),          # a constant mask
]
CONSTANT = 9


def paste_masks(M):
    rng = np.random.RandomState(11)
    yy, xx = np.mgrid[0:28, 0:28]
    out = []
    for i in range(M):
        blob = 1.0 / (1.0 + np.exp(-(5.0 + i % 4 - np.hypot(yy - 12 - i % 3, xx - 15 + i % 5)) * 0.8))
        out.append(np.full((28, 28), 0.6, np.float32) if i == CONSTANT else (0.02 + 0.95 * blob + 0.03 * rng.rand(28, 28)).astype(np.float32))
    return np.stack(out) if out else np.zeros((0, 28, 28), np.float32)


@pytest.mark.parametrize("M", [0, 1, 5, 10])
def test_mask_paste_equals_the_host_path(ops, M):
    from image_captioning_amd import mask_rcnn_model as MR
    masks, boxes = paste_masks(M), np.array(BOXES[:M], np.int32).reshape(M, 4)
    G = 4096
    buf = torch.full((M * H * W + 2 * G,), 0xFF, dtype=torch.uint8, device="cuda")
    out = buf[G:G + M * H * W].view(M, H, W)
    got = ops.mask_paste(dev(masks), dev(boxes, torch.int32), H, W, out=out)
    assert got is out
    host = buf.cpu().numpy()
    assert (host[:G] == 0xFF).all() and (host[G + M * H * W:] == 0xFF).all(), "guard bytes were written"
    got = host[G:G + M * H * W].reshape(M, H, W)
    for i in range(M):
        want = MR.unmold_mask(masks[i], boxes[i], (H, W, 3))
        assert np.array_equal(got[i], want), (i, BOXES[i], int((got[i] != want).sum()))
        assert np.array_equal(want, R.unmold_mask(masks[i], boxes[i], (H, W, 3)))
    if M == 10:
        assert got[5].sum() > 0 and got[0].sum() > 0 and got[1].sum() > 0 and not got[7].any() and not got[8].any() and not got[CONSTANT].any()
        assert (got[0] & got[1]).any(), "the two overlapping boxes' masks should overlap"
    fresh = ops.mask_paste(dev(masks), dev(boxes, torch.int32), H, W)
    assert fresh.dtype == torch.uint8 and tuple(fresh.shape) == (M, H, W) and np.array_equal(fresh.cpu().numpy(), got)


def test_mask_paste_other_mask_sizes(ops):
    """Up to 64 x 64 and not square: the mask's own sides drive both passes."""
    from image_captioning_amd import mask_rcnn_model as MR
    rng = np.random.RandomState(3)
    for h, w in ((64, 64), (7, 40), (1, 1)):
        masks = rng.rand(3, h, w).astype(np.float32)
        boxes = np.array([(0, 0, H, W), (10, 20, 13, 120), (60, 60, 96, 61)], np.int32)
        got = ops.mask_paste(dev(masks), dev(boxes, torch.int32), H, W).cpu().numpy()
        for i in range(3):
            assert np.array_equal(got[i], MR.unmold_mask(masks[i], boxes[i], (H, W, 3))), (h, w, i)
