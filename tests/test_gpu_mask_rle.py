"""ops.mask_rle / dc_mask_rle_u32 and detect(mask_format="rle") on the device (-m gpu).  Every comparison is an equality: the oracle is
mask_rle.encode(mask_rcnn_model.unmold_mask(mask, box, (H, W))), the host path's plane encoded on the host, cross-checked once
against encode of ops.mask_paste's plane.

Shapes: a 97 x 131 image, 28 x 28 masks, at most 12 detections a call; and a 5 x 300 image, whose 301 column slots take 76 blocks of
four waves and a second 256-wide pass of the column prefix sum.  The boxes: interior, on each border, the full image, full height
(runs cross column boundaries), one pixel wide, one pixel tall, smaller than the mask in both directions (the shrinking branch of the
coefficient code), zero area, leaving the image.  The masks: random, constant (bytescale's zero range), a checkerboard (a transition
at almost every row of a column), one whose resized top-left pixel is set in a full-image box (counts[0] == 0), one whose last pixel
is set (an odd number of transitions), one that is set almost everywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from _detect_device import dev

pytestmark = pytest.mark.gpu
H, W = 97, 131
GUARD = 4096                                                                 # words behind counts / bytes behind the workspace

BOXES = [
    (20, 30, 60, 70),        # interior
    (0, 10, 30, 50),         # on the top border
    (10, 0, 40, 35),         # on the left border
    (60, 20, 97, 60),        # on the bottom border
    (15, 90, 50, 131),       # on the right border
    (0, 0, 97, 131),         # the full image
    (0, 40, 97, 75),         # full height
    (10, 50, 80, 51),        # one pixel wide
    (50, 3, 51, 43),         # one pixel tall
    (30, 40, 40, 45),        # 10 x 5: smaller than the mask in both directions
    (10, 10, 10, 30),        # zero area
    (90, 120, 98, 131),      # leaves the image
]


def _blob(cy, cx, radius):
    yy, xx = np.mgrid[0:28, 0:28]
    return (1.0 / (1.0 + np.exp(np.hypot(yy - cy, xx - cx) - radius))).astype(np.float32)


def _cases():
    rng = np.random.RandomState(5)
    board = ((np.add.outer(np.arange(28), np.arange(28)) & 1) * 0.9 + 0.05).astype(np.float32)
    hole = np.ones((28, 28), np.float32)
    hole[13, 14] = 0.0
    wide = np.array([(0, 0, 5, 300), (1, 10, 4, 290), (0, 100, 5, 300), (2, 299, 3, 300), (0, 0, 5, 1), (0, 255, 5, 258)], np.int32)
    return {
        "boxes_97x131": (rng.rand(12, 28, 28).astype(np.float32), np.array(BOXES, np.int32), H, W),
        "masks_97x131": (np.stack([rng.rand(28, 28).astype(np.float32), np.full((28, 28), 0.6, np.float32), board, board, _blob(0, 0, 9),
                                   _blob(27, 27, 9), hole, hole, _blob(27, 13, 6), 1.0 - board]),
                         np.array([(7, 9, 77, 101), (0, 0, 33, 57), (5, 5, 95, 125), (0, 0, 97, 131), (0, 0, 97, 131), (0, 0, 97, 131),
                                   (0, 0, 97, 131), (40, 60, 97, 131), (0, 30, 97, 90), (0, 0, 97, 131)], np.int32), H, W),
        "blocks_5x300": (rng.rand(6, 28, 28).astype(np.float32), wide, 5, 300),
    }


_ORACLE = {}


def oracle(name):
    """(masks, boxes, H, W, the encodings of the host path's planes): computed once, never changed."""
    if name not in _ORACLE:
        from image_captioning_amd import mask_rcnn_model as MR, mask_rle
        masks, boxes, h, w = _cases()[name]
        _ORACLE[name] = (masks, boxes, h, w, [mask_rle.encode(MR.unmold_mask(masks[i], boxes[i], (h, w))) for i in range(len(masks))])
    return _ORACLE[name]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def _same_lists(got, want):
    assert len(got) == len(want)
    for i, (g, w_) in enumerate(zip(got, want)):
        assert g["size"] == w_["size"] and g["counts"].dtype == np.uint32, i
        assert int(g["counts"].astype(np.int64).sum()) == g["size"][0] * g["size"][1], i          # the sum check, on every result
        assert np.array_equal(g["counts"], w_["counts"]), (i, g["counts"][:12], w_["counts"][:12])


def raw(masks, boxes, h, w, capacity, fill=0x5A5A5A5A, workspace=None, workspace_bytes=None):
    """dc_mask_rle_u32 itself: offsets and counts sit in patterned buffers with GUARD words behind them.  Returns (return code, offsets
    [M+1], the whole counts buffer [capacity + GUARD] as uint32) on the host."""
    from image_captioning_amd import _lib
    lib = _lib.load()
    M = masks.shape[0]
    offsets = torch.full((M + 1 + GUARD,), 77, dtype=torch.int32, device="cuda")
    counts = torch.full((capacity + GUARD,), fill, dtype=torch.int32, device="cuda")
    d = _lib.MaskRleDesc()
    d.M, d.h, d.w, d.H, d.W, d.capacity = M, masks.shape[1], masks.shape[2], h, w, capacity
    d.masks, d.boxes, d.offsets, d.counts = masks.data_ptr(), boxes.data_ptr(), offsets.data_ptr(), counts.data_ptr()
    need = lib.dc_mask_rle_workspace_bytes(C.byref(d))
    if workspace is None:
        workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device="cuda")
        workspace_bytes = need
    d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace_bytes
    rc = lib.dc_mask_rle_u32(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    off = offsets.cpu().numpy()
    assert (off[M + 1:] == 77).all(), "words behind offsets were written"
    return rc, off[:M + 1], counts.cpu().numpy().view(np.uint32), need


def _lists(off, counts, h, w):
    return [{"size": [h, w], "counts": counts[off[m]:off[m + 1]].copy()} for m in range(len(off) - 1)]


@pytest.mark.parametrize("name", sorted(_cases()))
def test_mask_rle_equals_the_encoded_host_planes(ops, name):
    from image_captioning_amd import mask_rle
    masks, boxes, h, w, want = oracle(name)
    run = ops.mask_rle(dev(masks), dev(boxes, torch.int32), h, w)
    got = run.rles()
    total = sum(len(r["counts"]) for r in want)
    assert run.launches == (1 if total <= ops.mask_rle_capacity(len(masks), h, w) else 2)            # (both happen among the cases)
    assert run.offsets.dtype == torch.int32 and tuple(run.offsets.shape) == (len(masks) + 1,)
    _same_lists(got, want)
    planes = ops.mask_paste(dev(masks), dev(boxes, torch.int32), h, w).cpu().numpy()               # the cross-check: the device's own planes
    for i in range(len(masks)):
        assert np.array_equal(mask_rle.decode(got[i]), planes[i]), i
        assert np.array_equal(mask_rle.encode(planes[i])["counts"], got[i]["counts"]), i
    off = run.offsets.cpu().numpy()
    assert off[0] == 0 and np.array_equal(np.diff(off), [len(r["counts"]) for r in want])


def test_the_cases_hold_what_they_claim():
    """(on the oracle alone: a case that lost its edge would test nothing)"""
    _, boxes, h, w, want = oracle("boxes_97x131")
    assert want[10]["counts"].tolist() == [h * w] and want[11]["counts"].tolist() == [h * w]         # zero area, leaving the image
    assert all(len(r["counts"]) > 1 for r in want[:10])
    masks_, boxes_, _, _, wm = oracle("masks_97x131")
    assert wm[1]["counts"].tolist() == [h * w]                                                       # the constant mask
    assert len(wm[3]["counts"]) > 20 * w                                                             # the checkerboard: many runs a column
    assert wm[4]["counts"][0] == 0 and wm[6]["counts"][0] == 0                                       # pixel (0, 0) is set
    assert len(wm[5]["counts"]) % 2 == 0 and len(wm[6]["counts"]) % 2 == 0                           # the last pixel is set: T is odd
    assert len(wm[7]["counts"]) % 2 == 0 and len(wm[8]["counts"]) > 3
    _, _, _, _, wb = oracle("blocks_5x300")
    assert all(len(r["counts"]) > 1 for r in wb)


def test_a_small_capacity_keeps_offsets_exact_and_touches_nothing_beyond(ops):
    masks, boxes, h, w, want = oracle("boxes_97x131")
    m_t, b_t = dev(masks), dev(boxes, torch.int32)
    total = sum(len(r["counts"]) for r in want)
    rc, off_full, counts_full, _ = raw(m_t, b_t, h, w, total)
    assert rc == 0 and off_full[-1] == total
    _same_lists(_lists(off_full, counts_full, h, w), want)
    assert (counts_full[total:] == 0x5A5A5A5A).all()
    for capacity in (3, 0, total - 1):
        rc, off, counts, _ = raw(m_t, b_t, h, w, capacity)
        assert rc == 0 and np.array_equal(off, off_full)
        assert np.array_equal(counts[:capacity], counts_full[:capacity])
        assert (counts[capacity:] == 0x5A5A5A5A).all(), "words at or beyond capacity were written"
    run = ops.mask_rle(m_t, b_t, h, w, capacity=3)                                                    # the wrapper's second launch
    got = run.rles()
    assert run.launches == 2 and run.capacity == total
    _same_lists(got, want)


def test_an_exact_workspace_with_a_guard_behind_it(ops):
    masks, boxes, h, w, want = oracle("masks_97x131")
    m_t, b_t = dev(masks), dev(boxes, torch.int32)
    total = sum(len(r["counts"]) for r in want)
    _, _, _, need = raw(m_t, b_t, h, w, total)
    assert need > 0
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, off, counts, _ = raw(m_t, b_t, h, w, total, workspace=ws, workspace_bytes=need)
    assert rc == 0
    _same_lists(_lists(off, counts, h, w), want)
    assert (ws[need:].cpu().numpy() == 0xA5).all(), "bytes behind the workspace were written"
    from image_captioning_amd import _lib
    rc, _, counts, _ = raw(m_t, b_t, h, w, total, workspace=ws, workspace_bytes=need - 1)            # a byte short: refused, nothing runs
    assert rc == _lib.EWORKSPACE and (counts == 0x5A5A5A5A).all()


def test_two_calls_give_identical_bytes(ops):
    masks, boxes, h, w, _ = oracle("masks_97x131")
    m_t, b_t = dev(masks), dev(boxes, torch.int32)
    first = ops.mask_rle(m_t, b_t, h, w, capacity=40000)
    a = first.pack.cpu().numpy().copy()
    used = len(masks) + 1 + int(a[len(masks)])
    b = ops.mask_rle(m_t, b_t, h, w, capacity=40000).pack.cpu().numpy()
    assert used <= 40000 and np.array_equal(a[:used], b[:used])


def test_no_detections(ops):
    run = ops.mask_rle(torch.zeros((0, 28, 28), device="cuda"), torch.zeros((0, 4), dtype=torch.int32, device="cuda"), H, W)
    assert run.rles() == [] and run.offsets.cpu().numpy().tolist() == [0]
    rc, off, counts, need = raw(torch.zeros((0, 28, 28), device="cuda"), torch.zeros((0, 4), dtype=torch.int32, device="cuda"), H, W, 8)
    assert rc == 0 and off.tolist() == [0] and (counts == 0x5A5A5A5A).all()


def test_the_entry_refuses_what_the_header_says(ops):
    from image_captioning_amd import _lib
    lib = _lib.load()
    masks, boxes, h, w, _ = oracle("boxes_97x131")
    m_t, b_t = dev(masks), dev(boxes, torch.int32)
    out = torch.zeros((64,), dtype=torch.int32, device="cuda")

    def call(**over):
        d = _lib.MaskRleDesc()
        d.M, d.h, d.w, d.H, d.W, d.capacity = 12, 28, 28, h, w, 16
        d.masks, d.boxes, d.offsets, d.counts = m_t.data_ptr(), b_t.data_ptr(), out.data_ptr(), out[32:].data_ptr()
        for k, v in over.items():
            setattr(d, k, v)
        return lib.dc_mask_rle_u32(C.byref(d), None), lib.dc_mask_rle_workspace_bytes(C.byref(d))
    for over in (dict(capacity=-1), dict(offsets=None), dict(counts=None), dict(masks=None), dict(boxes=None), dict(h=65), dict(H=0), dict(M=-1),
                 dict(M=70000), dict(H=1 << 14, W=1 << 14), dict(offsets=out.data_ptr() + 2)):
        assert call(**over) == (_lib.EINVAL, 0), over
    assert call()[0] == _lib.EWORKSPACE                                      # (no workspace in the descriptor)


@pytest.mark.parametrize("refine", ["host", "device"])
def test_detect_rle_equals_the_dense_host_path_for_two_images_of_different_sizes(ops, refine):
    from image_captioning_amd import mask_rle
    from test_gpu_maskrcnn_model import S, image, make_model
    model, cfg, _ = make_model(images=2)
    imgs = [image(7, 96, S), image(8, S, 80)]
    dense = model.detect(imgs, postprocess="host", refine=refine)
    on_host = model.detect(imgs, postprocess="host", refine=refine, mask_format="rle")
    on_device = model.detect(imgs, postprocess="device", refine=refine, mask_format="rle")
    assert sum(len(r["rois"]) for r in dense) >= 1 and any(r["masks"].any() for r in dense if len(r["rois"]))
    for b in range(2):
        n = len(dense[b]["rois"])
        print("refine=%s image %d (%s): %d detections" % (refine, b, imgs[b].shape[:2], n))
        for r in (on_host[b], on_device[b]):
            assert np.array_equal(r["rois"], dense[b]["rois"]) and np.array_equal(r["class_ids"], dense[b]["class_ids"])
            assert np.array_equal(r["scores"].view(np.int32), dense[b]["scores"].view(np.int32))
            assert isinstance(r["masks"], list) and len(r["masks"]) == n
        _same_lists(on_device[b]["masks"], on_host[b]["masks"])
        for i in range(n):
            assert on_device[b]["masks"][i]["size"] == list(imgs[b].shape[:2])
            assert np.array_equal(mask_rle.decode(on_device[b]["masks"][i]), dense[b]["masks"][:, :, i]), (b, i)
        assert [tuple(m.shape) for m in model.last_class_masks] == [(len(r["rois"]), 28, 28) for r in dense]
    with pytest.raises(ValueError, match="mask_format"):
        model.detect(imgs, mask_format="polygon")


def test_detect_rle_without_a_detection_returns_empty_lists(ops):
    from test_gpu_maskrcnn_model import detect_weights, image, make_model
    model, cfg, _ = make_model(Wt=detect_weights(background=1000.0))       # the background wins every RoI
    for refine in ("host", "device"):
        for post in ("host", "device"):
            out = model.detect([image()], postprocess=post, refine=refine, mask_format="rle")[0]
            assert out["masks"] == [] and out["rois"].shape == (0, 4)
