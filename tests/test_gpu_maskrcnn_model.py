"""Mask R-CNN at inference (mask_rcnn_model.MaskRCNN.detect) on the device (-m gpu), compared stage by stage -- the argmax, the NMS and
np.rint make an end-to-end float comparison meaningless, so each stage is fed what the device's own previous stage produced:

  heads        last_heads against the float64 heads of tests/_maskrcnn_ref.py (the oracle's encoder, RoIAlign and RoI head) on the
               device's own proposals, at the tolerance the RoI tag model test holds its float64 comparison to (2e-4 of the largest value);
  selection    the selected classes equal the float64 argmax wherever the float64 top-two margin exceeds that tolerance; at most 10 % of
               the RoIs may be excused (the weight spread keeps the float64 reference itself inside that cap: 0 RoIs excused on the CPU);
  detections   last_detections equals the host refine_detections + unmold_boxes on the device's own last_selection, exactly;
  mask head    stage by stage on the device's own detection boxes and FPN maps (the encoder's error is the heads stage's business), each
               stage fed the device's own previous stage: RoIAlign at MASK_POOL_SIZE within 1e-5 and each of the four convolutions +
               frozen BN + ReLU within 2e-5 of max(1, its largest output) -- the figures tests/test_gpu_kernels.py holds RoIAlign and every
               fp32 convolution to --, then last_class_masks within the tail kernel's own running bound on the device's fourth layer;
               detect()'s internal chain is those launches bit for bit.  The synthetic mask weights are scaled so that activations are
               O(1) and the sigmoid does not saturate (tests/_maskrcnn_ref.scale_mask_weights); tests/test_maskrcnn_ref.py shows on the
               CPU that a dropped BatchNorm beta, bias, a wrong quadrant or class leaves these bounds;
  unmolding    postprocess="device" returns the bytes, boxes, ids and scores of postprocess="host", for two images of different sizes
               and with mold="device".

The factory is the RoI tag test's shape: S = 128, one stage-4 block, 60 proposals, NUM_CLASSES = 9, 10 detections, no confidence
floor, synthetic weights with mrcnn_class_logits spread by 10 (five classes win), mrcnn_bbox_fc damped to 0.3 and the mask head scaled
as said above."""
import numpy as np
import pytest
import torch

import _maskrcnn_ref as R

pytestmark = pytest.mark.gpu
MEAN = [123.7, 116.8, 103.9]
S, C, BLOCKS = 128, 9, 1
TOL = 2e-4


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max()) / max(1e-30, float(np.abs(want).max()))


def detect_weights(spread=10.0, background=None):
    from image_captioning_amd import synth
    Wt = dict(synth.encoder_weights(0, BLOCKS), **synth.rpn_weights(4))
    Wt['rpn_conv_shared/kernel'] = Wt['rpn_conv_shared/kernel'] * np.float32(0.05)
    Wt['rpn_bbox_pred/kernel'] = Wt['rpn_bbox_pred/kernel'] * np.float32(0.3)
    Wt.update(synth.head_weights(1))
    Wt['mrcnn_class_conv1/kernel'] = Wt['mrcnn_class_conv1/kernel'] * np.float32(0.05)
    Wt.update(synth.detect_head_weights(6, C))
    Wt['mrcnn_class_logits/kernel'] = Wt['mrcnn_class_logits/kernel'] * np.float32(spread)
    Wt['mrcnn_bbox_fc/kernel'] = Wt['mrcnn_bbox_fc/kernel'] * np.float32(0.3)
    Wt = R.scale_mask_weights(Wt)
    if background is not None:
        Wt['mrcnn_class_logits/bias'] = Wt['mrcnn_class_logits/bias'].copy()
        Wt['mrcnn_class_logits/bias'][0] = background
    return Wt


def make_model(images=1, Wt=None, **over):
    from image_captioning_amd.mask_rcnn_model import MaskRCNN, MaskRCNNConfig

    class Cfg(MaskRCNNConfig):
        NAME = "maskrcnn"
        IMAGES_PER_GPU = images
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
        POST_NMS_ROIS_INFERENCE = 60
        DETECTION_MAX_INSTANCES = 10
        DETECTION_MIN_CONFIDENCE = 0
    for k, v in over.items():
        setattr(Cfg, k, v)
    cfg = Cfg(C)
    Wt = detect_weights() if Wt is None else Wt
    model = MaskRCNN("inference", cfg, "logs", stage4_blocks=BLOCKS)
    model.set_weights(Wt)
    return model, cfg, Wt


def image(seed=7, h=96, w=S):
    from image_captioning_amd import synth
    return synth.images(seed, 1, h, w)[0]


_RUN = {}


def one_run():
    """The model, one detect() on a 96 x 128 image and everything the device kept of it; the float64 encoder maps: once."""
    if not _RUN:
        model, cfg, Wt = make_model()
        img = image()
        res = model.detect([img])[0]
        keep = dict(res=res, props=model.last_proposals.cpu().numpy()[0].copy(), z=model.last_heads[0].cpu().numpy().copy(),
                    d=model.last_heads[1].cpu().numpy().copy(), sel=model.last_selection[0], det=model.last_detections[0],
                    masks=np.asarray(model.last_class_masks[0]).copy(), maps=[m.cpu().numpy().astype(np.float64) for m in model.plan().P])
        # the mask head once more, launch by launch, on the maps and detections of that call: every stage's output
        from image_captioning_amd import ops
        det, top, p = keep['det'], model.caption_model, model.plan()
        norm = (det['boxes'].astype(np.float32) / np.array([S, S, S, S])).astype(np.float32)
        x = ops.roi_align_pyramid(list(p.P), torch.tensor(norm[None], device=model.device), float(S * S), 14)[0]
        ids_dev = torch.tensor(det['class_ids'], dtype=torch.int32, device=model.device)
        stages = [x]
        for i in range(4):
            stages.append(top.mask_layer(i, stages[-1]))
        keep.update(norm=norm, stages=[t.cpu().numpy().copy() for t in stages], trunk=top.mask_trunk(x).cpu().numpy().copy(),
                    chain=top.class_masks(x, ids_dev).cpu().numpy().copy())
        molded, _, windows = model.mold_inputs([img])
        W64 = {k: np.asarray(v, np.float64) for k, v in Wt.items()}
        maps64, hw = R.encoder_maps(W64, molded[0], MEAN, BLOCKS)
        _RUN.update(model=model, cfg=cfg, Wt=Wt, W64=W64, img=img, window=windows[0], maps64=maps64, hw=hw, **keep)
    return _RUN


def test_heads_match_the_float64_heads_on_the_devices_proposals(gpu):
    s = one_run()
    z64, d64 = R.detection_heads(s['W64'], s['maps64'], s['hw'], s['props'])
    s['z64'] = z64
    ez, ed = rel_err(s['z'], z64), rel_err(s['d'], d64)
    print("heads: logits err %.3e (|z| up to %.2f), deltas err %.3e (|d| up to %.2f)" % (ez, np.abs(z64).max(), ed, np.abs(d64).max()))
    assert s['z'].shape == (60, C) and s['d'].shape == (60, 4 * C)
    assert ez < TOL and ed < TOL


def test_selected_classes_are_the_float64_argmax_outside_the_margin(gpu):
    s = one_run()
    z64 = s.get('z64')
    if z64 is None:
        z64, _ = R.detection_heads(s['W64'], s['maps64'], s['hw'], s['props'])
    rois, ids, scores, deltas = s['sel']
    top2 = np.sort(z64, axis=1)[:, -2:]
    excused = (top2[:, 1] - top2[:, 0]) <= TOL * np.abs(z64).max()
    winners = np.bincount(z64.argmax(axis=1), minlength=C)
    print("selection: float64 winners per class %s, %d of %d RoIs excused" % (winners.tolist(), excused.sum(), len(ids)))
    assert excused.sum() <= 0.1 * len(ids)
    assert (winners > 0).sum() >= 3, "several classes should win"
    assert np.array_equal(ids[~excused], z64.argmax(axis=1)[~excused])
    # the selection is the kernel's on the device's own heads: ids, scores and deltas against float64 on THOSE logits
    want_ids, want_scores, want_d, d_max = R.class_select(s['z'], s['d'])
    assert np.array_equal(ids, want_ids) and np.array_equal(deltas.view(np.int32), want_d.view(np.int32))
    assert (np.abs(scores - want_scores) <= (d_max + C + 8) * R.U * want_scores).all()
    assert np.array_equal(rois, s['props'])


def test_detections_are_the_host_refinement_of_the_devices_selection(gpu):
    from image_captioning_amd import mask_rcnn_model as MR
    s = one_run()
    rois, ids, scores, deltas = s['sel']
    boxes, cls, sc, keep = MR.refine_detections(rois, ids, scores, deltas, np.asarray(s['window'], np.float32), s['cfg'])
    final, ok = MR.unmold_boxes(boxes, s['img'].shape, s['window'])
    det, res = s['det'], s['res']
    print("detections: %d refined, %d with area; classes %s" % (len(boxes), ok.sum(), cls[ok].tolist()))
    assert ok.sum() >= 5 and len(set(cls[ok].tolist())) >= 2
    assert np.array_equal(det['boxes'], boxes[ok]) and np.array_equal(det['class_ids'], cls[ok]) and np.array_equal(det['scores'], sc[ok])
    assert np.array_equal(det['rois'], final[ok])
    assert set(res) == {"rois", "class_ids", "scores", "masks"}
    assert np.array_equal(res['rois'], final[ok]) and res['rois'].dtype == np.int32
    assert np.array_equal(res['class_ids'], cls[ok]) and res['class_ids'].dtype == np.int32
    assert np.array_equal(res['scores'], sc[ok]) and res['scores'].dtype == np.float32
    assert (np.diff(res['scores']) <= 0).all() and (res['class_ids'] > 0).all()
    H, W = s['img'].shape[:2]
    assert res['masks'].shape == (H, W, ok.sum()) and res['masks'].dtype == np.uint8 and set(np.unique(res['masks'])) <= {0, 1}
    assert res['rois'].min() >= 0 and res['rois'][:, 2].max() <= H and res['rois'][:, 3].max() <= W


def test_mask_head_stage_by_stage(gpu):
    s = one_run()
    det, stages, W64 = s['det'], s['stages'], s['W64']
    n = len(det['boxes'])
    from oracle import np_oracle as O
    want0 = O.pyramid_roi_align(s['norm'][None], s['maps'], (S, S, 3), 14)[0]
    e0 = np.abs(stages[0] - want0).max()
    print("mask head: %d detections; RoIAlign 14 err %.3e (bound %.3e, |x| up to %.1f)" % (n, e0, R.layer_tol(want0, R.ROI_TOL), np.abs(want0).max()))
    assert stages[0].shape == (n, 14, 14, 256) and n >= 5 and e0 <= R.layer_tol(want0, R.ROI_TOL)
    for i in (1, 2, 3, 4):
        want = R.mask_layer(W64, i, stages[i - 1])                       # float64 on the device's own input of this layer
        err, bound = np.abs(stages[i] - want).max(), R.layer_tol(want)
        print("  mrcnn_mask_conv%d + bn + relu: err %.3e, bound %.3e, |y| up to %.2f, %.0f %% positive" % (i, err, bound, np.abs(want).max(), 100 * (want > 0).mean()))
        assert err <= bound
        assert 0.3 < np.abs(want).max() < 30 and (want > 0).mean() > 0.1, "the activations should be O(1) and alive"
    want, z, A = R.mask_tail_of(W64, stages[4], det['class_ids'])
    tol = R.mask_tail_tol(A, 256, 256)
    got = s['masks']
    err = np.abs(got.astype(np.float64) - want)
    print("  tail: worst error %.3e, worst error / bound %.3f, bound up to %.2e, masks in [%.3f, %.3f] std %.3f"
          % (err.max(), (err / tol).max(), tol.max(), want.min(), want.max(), want.std()))
    assert got.shape == (n, 28, 28) and got.dtype == np.float32 and (err <= tol).all()
    assert want.std() > 0.05 and want.min() > 0.01 and want.max() < 0.99 and tol.max() < 2e-3, "the masks should vary and stay out of saturation"
    # detect()'s own chain is these launches: the trunk's output and the class masks, bit for bit
    assert np.array_equal(s['trunk'].view(np.int32), stages[4].view(np.int32))
    assert np.array_equal(s['chain'].view(np.int32), got.view(np.int32))
    # end to end, the bound the whole head is given: the float64 mask head on the FLOAT64 encoder's maps, within the tail's bound widened
    # by the four convolutions' tolerance (their sum taken as a uniform error of the tail's input, times its worst-case gain on z).  Loose
    # beside the stage checks above, which are the ones that bite; it ties the chain to the float64 encoder as well.
    e2e, xs64 = R.mask_head(W64, s['maps64'], s['hw'], s['norm'], det['class_ids'])
    A64 = R.mask_tail_of(W64, xs64[4], det['class_ids'])[2]
    dx = sum(R.layer_tol(x) for x in xs64[1:])
    gain = R.tail_gain(W64, det['class_ids'])[:, None, :, None, :] * np.ones((1, 14, 1, 14, 1))
    tol2 = ((256 + 256 + 4) * R.U * A64 + dx * gain.reshape(n, 28, 28)) / 4.0 + 4.0 * R.U
    err2 = np.abs(got - e2e)
    print("  end to end against the float64 encoder + mask head: worst difference %.3e, bound up to %.2e" % (err2.max(), tol2.max()))
    assert (err2 <= tol2).all()
    # and the returned masks are the host unmolding of exactly these class masks
    from image_captioning_amd import mask_rcnn_model as MR
    for i in range(n):
        assert np.array_equal(s['res']['masks'][:, :, i], MR.unmold_mask(got[i], det['rois'][i], s['img'].shape))


def _same(a, b):
    assert np.array_equal(a['rois'], b['rois']) and np.array_equal(a['class_ids'], b['class_ids'])
    assert np.array_equal(a['scores'].view(np.int32), b['scores'].view(np.int32))
    assert a['masks'].shape == b['masks'].shape and a['masks'].dtype == b['masks'].dtype and np.array_equal(a['masks'], b['masks'])


def test_device_and_host_unmolding_agree_for_two_images_of_different_sizes(gpu):
    model, cfg, _ = make_model(images=2)
    imgs = [image(7, 96, S), image(8, S, 80)]
    res = {(post, mold): model.detect(imgs, postprocess=post, mold=mold) for post in ("host", "device") for mold in ("host", "device")}
    base = res["host", "host"]
    for b in range(2):
        n = len(base[b]['rois'])
        print("image %d (%s): %d detections, %d mask pixels" % (b, imgs[b].shape[:2], n, int(base[b]['masks'].sum())))
        assert n >= 1 and base[b]['masks'].shape == imgs[b].shape[:2] + (n,) and base[b]['masks'].any()
        for key, r in res.items():
            _same(r[b], base[b])
    assert len(base[0]['rois']) + len(base[1]['rois']) >= 5
    dev_res = model.detect(imgs, postprocess="device", device_masks=True)
    for b in range(2):
        m = dev_res[b]['masks']
        assert isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.uint8 and tuple(m.shape) == (len(base[b]['rois']),) + imgs[b].shape[:2]
        assert np.array_equal(m.cpu().numpy().transpose(1, 2, 0), base[b]['masks'])
        assert np.array_equal(dev_res[b]['rois'], base[b]['rois'])


def test_one_image_device_path_and_device_masks(gpu):
    s = one_run()
    model = s['model']
    for mold in ("host", "device"):
        _same(model.detect([s['img']], postprocess="device", mold=mold)[0], s['res'])
    out = model.detect([s['img']], postprocess="device", device_masks=True)[0]
    assert isinstance(out['masks'], torch.Tensor) and np.array_equal(out['masks'].cpu().numpy().transpose(1, 2, 0), s['res']['masks'])
    assert np.array_equal(np.asarray(model.last_class_masks[0].cpu()), s['masks'])
    with pytest.raises(ValueError, match="postprocess"):
        model.detect([s['img']], postprocess="gpu")
    with pytest.raises(ValueError, match="device_masks"):
        model.detect([s['img']], device_masks=True)


def test_an_image_without_a_detection_returns_the_empty_shapes(gpu):
    model, cfg, _ = make_model(Wt=detect_weights(background=1000.0))       # the background wins every RoI
    img = image()
    for post in ("host", "device"):
        out = model.detect([img], postprocess=post)[0]
        assert out['rois'].shape == (0, 4) and out['class_ids'].shape == (0,) and out['scores'].shape == (0,)
        assert out['masks'].shape == (0, 28, 28)
    assert (model.last_selection[0][1] == 0).all()
    out = model.detect([img], postprocess="device", device_masks=True)[0]
    assert tuple(out['masks'].shape) == (0, 96, S) and out['masks'].dtype == torch.uint8


def test_weights_saved_and_reloaded_by_name_give_identical_results(gpu, tmp_path):
    s = one_run()
    model = s['model']
    back = model.get_weights_dict()
    assert set(back) == set(s['Wt']) and all(np.array_equal(back[k], np.asarray(s['Wt'][k], np.float32)) for k in s['Wt'])
    assert back['mrcnn_class_logits/kernel'].shape == (1024, C) and back['mrcnn_mask/kernel'].shape == (1, 1, 256, C)
    for name in ("maskrcnn.h5", "maskrcnn.npz"):
        path = str(tmp_path / name)
        model.save_weights(path)
        other, _, _ = make_model(Wt=detect_weights(spread=3.0))
        other.load_weights(path, by_name=True)
        a, b = model.get_weights_dict(), other.get_weights_dict()
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a), name
        _same(other.detect([s['img']])[0], s['res'])
    partial, _, _ = make_model(Wt=detect_weights(spread=3.0))
    partial.load_weights(path, by_name=True, exclude=["mrcnn_class_logits", "mrcnn_bbox_fc", "mrcnn_mask"])
    c = partial.get_weights_dict()
    assert np.array_equal(c['mrcnn_mask_deconv/kernel'], a['mrcnn_mask_deconv/kernel'])
    assert not np.array_equal(c['mrcnn_class_logits/kernel'], a['mrcnn_class_logits/kernel'])


def test_refusals_on_the_device(gpu):
    from image_captioning_amd.mask_rcnn_model import MaskRCNN
    s = one_run()
    model, cfg = s['model'], s['cfg']
    with pytest.raises(ValueError, match='mode="training"'):
        MaskRCNN("training", cfg, "logs", stage4_blocks=BLOCKS)
    with pytest.raises(ValueError, match="bf16"):
        MaskRCNN("inference", cfg, "logs", stage4_blocks=BLOCKS, compute_dtype="bf16")
    for call in (lambda: model.train(None, None, 0.001, 1, "all"), lambda: model.compile(0.001), lambda: model.train_on_batch([])):
        with pytest.raises(ValueError, match="training is not built"):
            call()
    with pytest.raises(ValueError, match="use detect"):
        model.generate_captions([s['img']])
