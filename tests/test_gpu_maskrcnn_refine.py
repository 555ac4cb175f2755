"""MaskRCNN.detect(refine="device") on the device (-m gpu): the rois, class ids, scores and mask bytes of detect(refine="host") on the
same images, for postprocess "host" and "device", with device_masks and with mold="device", for two images of different sizes and
for an image without a detection -- and no device-to-host copy before the packed one.

The host refinement of the device's own selection is the yardstick, so each comparison first asserts that this selection is decided
(tests/_refine_det_ref.decided: a float64 exp one ulp off either way gives the same outputs) -- the only thing that separates the
device's exp from np.exp cannot show then -- and that its candidates' scores are pairwise distinct (the host path's default sort
promises no order among ties).  The factory is tests/test_gpu_maskrcnn_model.py's: S = 128, one stage-4 block, 60 proposals, 9 classes,
10 detections."""
import types

import numpy as np
import pytest
import torch

import _refine_det_ref as RD
import test_gpu_maskrcnn_model as MASK

pytestmark = pytest.mark.gpu
FORWARD, UPLOAD = "plan.forward", "upload:refine_consts"


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def selection_case(model, images):
    """The device's own selection of the last detect(refine="host") call as a case of the restatement."""
    from image_captioning_amd.mask_rcnn_model import detection_constants
    cfg = model.config
    windows = model.mold_inputs(images)[2]
    sel = model.last_selection
    return dict(name="selection", rois=np.stack([s[0] for s in sel]), class_ids=np.stack([s[1] for s in sel]), scores=np.stack([s[2] for s in sel]),
                deltas=np.stack([s[3] for s in sel]), std=tuple(cfg.BBOX_STD_DEV), min_confidence=cfg.DETECTION_MIN_CONFIDENCE,
                threshold=cfg.DETECTION_NMS_THRESHOLD, max_instances=cfg.DETECTION_MAX_INSTANCES, hw=tuple(cfg.IMAGE_SHAPE[:2]),
                windows=list(windows), image_shapes=[im.shape for im in images],
                consts=np.stack([detection_constants(windows[b], cfg, images[b].shape) for b in range(len(images))]))


def host_then_device(model, images):
    """detect(refine="host") as the yardstick, its selection asserted decided and free of ties; then the device mode's results by
    (postprocess, mold) and with device_masks."""
    base = model.detect(images)
    case = selection_case(model, images)
    assert RD.decided(case) and RD.distinct_scores(case)
    want = RD.refine(case)                                               # (and the restatement agrees with the yardstick)
    for b in range(len(images)):
        n = int(want["count"][b])
        assert np.array_equal(want["rois"][b, :n], base[b]["rois"]) and np.array_equal(want["class_ids"][b, :n], base[b]["class_ids"])
    got = {(post, mold): model.detect(images, postprocess=post, mold=mold, refine="device") for post in ("host", "device") for mold in ("host", "device")}
    return base, case, want, got


def test_one_image_every_mode_returns_the_host_refinements_result(gpu):
    model, cfg, _ = MASK.make_model()
    img = MASK.image()
    base, case, want, got = host_then_device(model, [img])
    n = len(base[0]["rois"])
    print("one image: %d detections, classes %s" % (n, base[0]["class_ids"].tolist()))
    assert n >= 5 and len(set(base[0]["class_ids"].tolist())) >= 2
    for key, res in got.items():
        MASK._same(res[0], base[0])
    # what the call leaves behind: the selection on the device, the detections from the packed copy, the class masks as device views
    sel = model.last_selection
    assert len(sel) == 4 and all(isinstance(t, torch.Tensor) and t.is_cuda for t in sel)
    assert [tuple(t.shape) for t in sel] == [(1, 60, 4), (1, 60), (1, 60), (1, 60, 4)]
    for t, k in zip(sel, ("rois", "class_ids", "scores", "deltas")):
        assert np.array_equal(t.cpu().numpy().view(np.int32), case[k].view(np.int32)), k
    det = model.last_detections[0]
    assert set(det) == {"boxes", "class_ids", "scores", "rois"}
    assert np.array_equal(det["boxes"], want["boxes"][0, :n]) and np.array_equal(det["rois"], base[0]["rois"]) and det["boxes"].dtype == np.int32
    assert np.array_equal(det["scores"].view(np.int32), base[0]["scores"].view(np.int32)) and det["scores"].dtype == np.float32
    m = model.last_class_masks[0]
    assert isinstance(m, torch.Tensor) and m.is_cuda and tuple(m.shape) == (n, 28, 28)
    model.detect([img], postprocess="host", refine="device")
    m_host = model.last_class_masks[0]
    model.detect([img], postprocess="host")
    assert isinstance(m_host, np.ndarray) and np.array_equal(m_host.view(np.int32), np.asarray(model.last_class_masks[0]).view(np.int32))
    out = model.detect([img], postprocess="device", device_masks=True, refine="device")[0]
    assert isinstance(out["masks"], torch.Tensor) and out["masks"].is_cuda and out["masks"].dtype == torch.uint8
    assert tuple(out["masks"].shape) == (n,) + img.shape[:2] and np.array_equal(out["masks"].cpu().numpy().transpose(1, 2, 0), base[0]["masks"])
    assert np.array_equal(out["rois"], base[0]["rois"])
    with pytest.raises(ValueError, match="refine must be 'host' or 'device'"):
        model.detect([img], refine="gpu")


def test_two_images_of_different_sizes(gpu):
    model, cfg, _ = MASK.make_model(images=2)
    imgs = [MASK.image(7, 96, MASK.S), MASK.image(8, MASK.S, 80)]
    base, case, want, got = host_then_device(model, imgs)
    assert len(base[0]["rois"]) + len(base[1]["rois"]) >= 5
    for b in range(2):
        n = len(base[b]["rois"])
        print("image %d (%s): %d detections, %d mask pixels" % (b, imgs[b].shape[:2], n, int(base[b]["masks"].sum())))
        assert n >= 1 and base[b]["masks"].any()
        for key, res in got.items():
            MASK._same(res[b], base[b])
    dev = model.detect(imgs, postprocess="device", device_masks=True, refine="device")
    for b in range(2):
        m = dev[b]["masks"]
        assert m.is_cuda and tuple(m.shape) == (len(base[b]["rois"]),) + imgs[b].shape[:2]
        assert np.array_equal(m.cpu().numpy().transpose(1, 2, 0), base[b]["masks"])


def test_an_image_without_a_detection(gpu):
    model, cfg, _ = MASK.make_model(Wt=MASK.detect_weights(background=1000.0))       # the background wins every RoI
    img = MASK.image()
    base, case, want, got = host_then_device(model, [img])
    assert base[0]["rois"].shape == (0, 4) and want["count"].tolist() == [0]
    for key, res in got.items():
        out = res[0]
        assert out["rois"].shape == (0, 4) and out["class_ids"].shape == (0,) and out["scores"].shape == (0,) and out["masks"].shape == (0, 28, 28)
        assert out["rois"].dtype == np.int32 and out["class_ids"].dtype == np.int32 and out["scores"].dtype == np.float32
    assert bool((model.last_selection[1] == 0).all())
    out = model.detect([img], postprocess="device", device_masks=True, refine="device")[0]
    assert tuple(out["masks"].shape) == (0, 96, MASK.S) and out["masks"].dtype == torch.uint8 and out["masks"].is_cuda


# ---- the call's timeline: ops and device-to-host copies in one list ------------------------------------------------------------------
HEAD = ["gemm", "bn_relu_fwd"] * 2
CHAIN = ([UPLOAD, FORWARD, "rpn_proposals", "roi_align_pyramid"] + HEAD + ["gemm", "gemm", "class_select", "refine_detections", "roi_align_pyramid"]
         + ["conv2d"] * 4 + ["mask_head_tail"])
COPY = ["copy:cpu", "copy:numpy"]


def timeline(model, img, monkeypatch, **kw):
    """Every public ops call (top level), the encoder pass, the upload of the constants and every Tensor.cpu / .item / .numpy / .tolist
    of one detect(refine="device") call, in the order issued."""
    from image_captioning_amd import _lib, ops
    model.detect([img], refine="device", **kw)                          # warm: buffers, the plan's graph
    seq, depth = [], [0]

    def wrap(name, fn):
        def call(*a, **k):
            if depth[0] == 0:
                seq.append(name)
            depth[0] += 1
            try:
                return fn(*a, **k)
            finally:
                depth[0] -= 1
        return call
    p = model.plan()
    with monkeypatch.context() as mp:
        for n, f in list(vars(ops).items()):
            if isinstance(f, types.FunctionType) and not n.startswith("_"):
                mp.setattr(ops, n, wrap(n, f))
        forward, to = p.forward, torch.Tensor.to
        mp.setattr(p, "forward", wrap(FORWARD, forward), raising=False)      # (its own launches, eager or replayed, are its business)

        def to_device(self, *a, **k):
            if not self.is_cuda and self.dtype == torch.float64 and self.dim() == 2 and self.shape[1] == _lib.REFINE_CONSTS:
                seq.append(UPLOAD)
            return to(self, *a, **k)
        mp.setattr(torch.Tensor, "to", to_device)
        for name in ("cpu", "item", "numpy", "tolist"):
            orig = getattr(torch.Tensor, name)
            mp.setattr(torch.Tensor, name, (lambda o, n: lambda self, *a, **k: (seq.append("copy:" + n), o(self, *a, **k))[1])(orig, name))
        res = model.detect([img], refine="device", **kw)
    torch.cuda.synchronize()
    return seq, res


def test_no_device_to_host_copy_before_the_packed_one(gpu, monkeypatch):
    model, cfg, _ = MASK.make_model()
    img = MASK.image()
    seq, res = timeline(model, img, monkeypatch, postprocess="device", device_masks=True)
    print("device masks: %r" % (seq,))
    assert seq == CHAIN + ["mask_paste"] + COPY and len(res[0]["rois"]) >= 5          # the packed copy ends the call
    seq, _ = timeline(model, img, monkeypatch, postprocess="device")
    assert seq == CHAIN + ["mask_paste"] + COPY + COPY                                # ... then the [:n] mask bytes
    seq, _ = timeline(model, img, monkeypatch, postprocess="host")
    assert seq == CHAIN + COPY + COPY                                                 # ... then the [B,M,28,28] class masks
    seq, _ = timeline(model, img, monkeypatch, postprocess="device", device_masks=True, mold="device")
    assert seq == ["pack_resize_batch", "resize_pad_packed"] + CHAIN + ["mask_paste"] + COPY
