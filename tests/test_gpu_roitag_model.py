"""The RoI tag model (roi_tag_model.ROITagRCNN) on the device (-m gpu): one step against the float64 tag joint step of
tests/_roitag_ref.py (the oracle's joint step with the caption decoder replaced by head + Dense + focal loss), the batch of two, the
degenerate sample, validation, training, checkpoints, train() and the inference path.  The factory is tests/_joint_cases.make_joint's
shape with a tag top: S = 128, one stage-4 block, 12 train RoIs, NUM_CLASSES = 40."""
import numpy as np
import pytest
import torch

from _joint_cases import joint_inputs
import _parity_cuts as PC
import _roitag_ref as R

pytestmark = pytest.mark.gpu
MEAN = [123.7, 116.8, 103.9]
S, C, BLOCKS = 128, 40, 1
LOSSES = ('roi_tag_classes_loss', 'rpn_class_loss', 'rpn_bbox_loss', 'reg_loss', 'loss')
# GT boxes: joint_inputs' three and a fourth; TAGLESS of them carries no tag (its row of gt_classes is zero), the others 1 to 3 tags
FOURTH_BOX = [60, 0, 128, 60]
TAGLESS = 3


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


def tag_weights(spread=1.0, bias=None):
    from image_captioning_amd import synth
    Wt = dict(synth.encoder_weights(0, BLOCKS), **synth.rpn_weights(4))
    Wt['rpn_conv_shared/kernel'] = Wt['rpn_conv_shared/kernel'] * np.float32(0.05)
    Wt['rpn_bbox_pred/kernel'] = Wt['rpn_bbox_pred/kernel'] * np.float32(0.3)
    Wt.update(synth.head_weights(1))
    Wt['mrcnn_class_conv1/kernel'] = Wt['mrcnn_class_conv1/kernel'] * np.float32(0.05)
    Wt.update(synth.tag_head_weights(6, C))
    Wt['roitag_class_logits/kernel'] = Wt['roitag_class_logits/kernel'] * np.float32(spread)
    if bias is not None:
        Wt['roitag_class_logits/bias'] = np.full(C, bias, np.float32)
    return Wt


def make_tag(mode="training", images=1, rois=12, Wt=None, model_dir="logs", **over):
    from image_captioning_amd.roi_tag_model import ROITagRCNN
    from image_captioning_amd.train_roi_tags import RoiTagConfig

    class Cfg(RoiTagConfig):
        NAME = "roitag"
        IMAGES_PER_GPU = images
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
        POST_NMS_ROIS_TRAINING = 60
        TRAIN_ROIS_PER_IMAGE = rois
    for k, v in over.items():
        setattr(Cfg, k, v)
    cfg = Cfg(C)
    Wt = tag_weights() if Wt is None else Wt
    model = ROITagRCNN(mode, cfg, model_dir, stage4_blocks=BLOCKS)
    model.set_weights(Wt)
    return model, cfg, Wt


def tag_inputs(seed=8, tagless=TAGLESS):
    """joint_inputs' image, anchors and boxes plus FOURTH_BOX; position 4 = gt_classes [1,6,C] int32."""
    inputs = joint_inputs(S, 24, 5, seed=seed)
    inputs[5][0, 3] = FOURTH_BOX
    gt = np.zeros((1, 6, C), np.int32)
    tags = [[3], [0, 17, 39], [8, 21], [5, 30]]
    for g, cols in enumerate(tags):
        if g != tagless:
            gt[0, g, cols] = 1
    inputs[4] = gt
    return inputs


def oracle_cfg(cfg):
    return dict(mean_pixel=MEAN, scales=cfg.RPN_ANCHOR_SCALES, ratios=cfg.RPN_ANCHOR_RATIOS, strides=cfg.BACKBONE_STRIDES,
                proposal_count=cfg.POST_NMS_ROIS_TRAINING, nms=cfg.RPN_NMS_THRESHOLD, train_rois=cfg.TRAIN_ROIS_PER_IMAGE,
                positive_ratio=cfg.ROI_POSITIVE_RATIO, weight_decay=cfg.WEIGHT_DECAY)


def grads_as_reference(model):
    """The flat gradient bucket re-expressed with the reference's layer names and HWIO kernels."""
    st = model.store
    saved = st.flat.clone()
    st.flat.copy_(st.flat_grad)
    try:
        return model.get_weights_dict()
    finally:
        st.flat.copy_(saved)


_STEP = {}


def one_step():
    """The model, its inputs, the device's losses / gradients / sample of one step and the float64 reference on that sample: once."""
    if not _STEP:
        model, cfg, Wt = make_tag()
        inputs = tag_inputs()
        losses = model._loss_list(model.forward_backward(inputs, shuffle=None))
        tg = model.last_targets
        got = grads_as_reference(model)
        rows = model.caption_model._bufs['loss_rows'].cpu().numpy().copy()
        dz = model.caption_model._bufs['dlogits'].cpu().numpy().copy()
        W64 = {k: np.asarray(v, np.float64) for k, v in Wt.items()}
        want, G, aux = R.tag_joint_loss_and_grads(W64, inputs[0][0], inputs[2][0, :, 0], inputs[3][0], oracle_cfg(cfg), (tg['rois'], tg['caps']),
                                                  stage4_blocks=BLOCKS)
        _STEP.update(model=model, cfg=cfg, Wt=Wt, inputs=inputs, losses=losses, tg=tg, got=got, rows=rows, dz=dz, want=want, G=G, aux=aux)
    return _STEP


def test_tag_model_step_matches_the_float64_reference(gpu):
    s = one_step()
    tg, losses, want = s['tg'], s['losses'], s['want']
    live = (tg['caps'] == 1).any(axis=1)
    print("sample: npos %d nneg %d live rows %d; losses %s" % (tg['npos'], tg['nneg'], live.sum(), {k: round(losses[k], 6) for k in LOSSES}))
    assert tg['caps'].shape == (12, C) and live.sum() > 0, "no live RoI: the tag loss is not exercised"
    agree = sum(1 for r in tg['rois'] if np.abs(s['aux']['proposals'] - r).sum(1).min() < 1e-5)
    assert agree >= 0.8 * (tg['npos'] + tg['nneg'])
    # exactly: the proposals from the device's own scores, every sampled RoI one of them bit for bit, and the sample what
    # DetectionTargetLayer selects from them and the step's GT rows.  (tests/_roitag_ref.py restates the tag step behind the sample, not
    # the sampler; the tag model samples with the joint model's DetectionTargetLayer, whose reference is the oracle's, with the tag rows
    # in the captions' place.  The reference's aux carries no RPN head outputs: the heads are compared in the joint model's tests.)
    plan, inputs = s['model'].plan(), s['inputs']
    props = PC.check_proposals_from_device_scores(plan, plan.anchors.cpu().numpy(), oracle_cfg(s['cfg']), 1)
    PC.assert_rois_are_proposals(tg['rois'], tg['npos'] + tg['nneg'], props[0])
    PC.check_sample(tg, props, inputs[4], inputs[5], S, S, s['cfg'])
    assert want['roi_tag_classes_loss'] > 0
    for k in LOSSES:
        print("  %s: got %.8f want %.8f" % (k, losses[k], want[k]))
        assert abs(losses[k] - want[k]) < 1e-4 * max(1.0, abs(want[k])), (k, losses[k], want[k])
    worst = {k: rel_err(s['got'][k], s['G'][k]) for k in R.tag_trainable(s['Wt'])}
    print("  worst gradients:", sorted(worst.items(), key=lambda kv: -kv[1])[:4])
    assert {'roitag_class_logits/kernel', 'roitag_class_logits/bias', 'mrcnn_class_bn1/gamma', 'mrcnn_class_conv2/kernel', 'fpn_p2/kernel',
            'rpn_bbox_pred/bias'} <= set(worst) and len(worst) == len(s['G'])
    for k, e in worst.items():
        assert e < 2e-4, (k, e)


def test_positive_roi_of_the_tagless_box_contributes_nothing(gpu):
    from image_captioning_amd.dense_model import box_iou_f32
    s = one_step()
    tg, inputs = s['tg'], s['inputs']
    gt_norm = inputs[5][0, :4] / np.float32(S)
    iou = box_iou_f32(tg['rois'][:tg['npos']], gt_norm)
    best = iou.argmax(axis=1)
    print("positives' GT boxes:", best.tolist(), "IoU", iou.max(axis=1).round(3).tolist())
    mine = np.flatnonzero(best == TAGLESS)
    assert len(mine) > 0 and (iou.max(axis=1) >= 0.5).all(), "the sample holds no positive RoI of the tag-less GT box"
    assert len(mine) < tg['npos'], "every positive RoI belongs to the tag-less box"
    for r in mine:
        assert not tg['caps'][r].any()
        assert s['rows'].view(np.int32)[r] == 0 and not s['dz'].view(np.int32)[r].any()
    live = (tg['caps'] == 1).any(axis=1)
    assert (s['rows'][~live] == 0).all() and (s['rows'][live] > 0).all()
    assert abs(s['losses']['roi_tag_classes_loss'] - s['aux']['loss_rows'][live].sum()) < 1e-4 * max(1.0, s['want']['roi_tag_classes_loss'])


def test_two_images_per_gpu_sum_over_both_images(gpu):
    model, cfg, Wt = make_tag(images=2)
    one, two = tag_inputs(seed=8), tag_inputs(seed=9, tagless=0)
    two[5][0, 1] = 0                                          # image 1: three GT boxes, another tag-less one, another anchor selection
    two[4][0, 1] = 0
    inputs = [np.concatenate([a, b]) for a, b in zip(one, two)]
    losses = model._loss_list(model.forward_backward(inputs, shuffle=None))
    tg = model.last_targets
    live = (tg['caps'] == 1).any(axis=2)
    print("live rows per image:", live.sum(axis=1).tolist(), "npos", tg['npos'].tolist())
    assert tg['rois'].shape == (2, 12, 4) and tg['caps'].shape == (2, 12, C) and (live.sum(axis=1) > 0).all()
    W64 = {k: np.asarray(v, np.float64) for k, v in Wt.items()}
    want, G, auxes = R.tag_joint_loss_and_grads_batch(W64, inputs[0], inputs[2][:, :, 0], inputs[3], oracle_cfg(cfg), (tg['rois'], tg['caps']),
                                                      stage4_blocks=BLOCKS)
    per_image = [a['loss_rows'].sum() for a in auxes]
    assert abs(want['roi_tag_classes_loss'] - sum(per_image)) < 1e-12 and min(per_image) > 0
    for k in LOSSES:
        print("  %s: got %.8f want %.8f" % (k, losses[k], want[k]))
        assert abs(losses[k] - want[k]) < 1e-4 * max(1.0, abs(want[k])), (k, losses[k], want[k])
    got = grads_as_reference(model)
    worst = {k: rel_err(got[k], G[k]) for k in R.tag_trainable(Wt)}
    print("  worst gradients:", sorted(worst.items(), key=lambda kv: -kv[1])[:4])
    assert max(worst.values()) < 2e-4, sorted(worst.items(), key=lambda kv: -kv[1])[:5]


def test_a_sample_without_a_live_row(gpu):
    """No GT box carries a tag: the tag loss is exactly 0, the head's and roitag_'s gradients are exactly zero, the RPN's are those of
    the ordinary step, nothing is NaN or Inf, and an optimizer step still works."""
    s = one_step()
    model, cfg, Wt = make_tag()
    inputs = tag_inputs()
    inputs[4] = np.zeros_like(inputs[4])
    raw = model.forward_backward(inputs, shuffle=None)
    assert torch.isfinite(raw).all() and torch.isfinite(model.store.flat_grad).all()
    losses = model._loss_list(raw)
    tg = model.last_targets
    assert tg['npos'] == s['tg']['npos'] and not tg['caps'].any()            # the same RoIs were drawn, none of them live
    assert losses['roi_tag_classes_loss'] == 0.0
    for k in ('rpn_class_loss', 'rpn_bbox_loss', 'reg_loss'):                     # (the RPN loss sums are float atomics: last bits may differ)
        assert abs(losses[k] - s['losses'][k]) < 1e-6 * max(1.0, abs(s['losses'][k])), k
    got = grads_as_reference(model)
    wd = np.float64(cfg.WEIGHT_DECAY)
    for k in R.tag_trainable(Wt):
        if k.startswith(('mrcnn_', 'roitag_')):
            # the bucket holds loss gradient + the L2 term 2 * (WEIGHT_DECAY / size) * w, added in float32: with a loss gradient of exactly
            # zero that is the float32 product itself (BN gamma / beta are not regularised: exact zeros)
            w32 = np.asarray(Wt[k], np.float32)
            reg = np.zeros_like(w32) if k.endswith(('gamma', 'beta')) else (np.float32(2.0) * np.float32(wd / w32.size)) * w32
            assert np.array_equal(np.asarray(got[k]).view(np.int32), reg.view(np.int32)), k
        elif k.startswith('rpn_'):
            assert rel_err(got[k], s['got'][k]) < 1e-6, k                        # the RPN branch does not see the tags
    model.compile(1e-3)
    assert np.isfinite(model.train_on_batch(inputs)).all()


def test_validation_is_forward_only(gpu):
    model, cfg, Wt = make_tag()
    inputs = tag_inputs()
    model.forward_backward(inputs)
    g0 = model.store.flat_grad.clone()
    state = model._dt_step
    out = model.test_on_batch(inputs)
    assert len(out) == 4 and np.isfinite(out).all() and out[3] == model.last_losses['roi_tag_classes_loss']
    assert torch.equal(model.store.flat_grad, g0) and model._dt_step == state and model._dt_val_step == 1
    fwd = model._loss_list(model.forward_backward(inputs, shuffle=None, backward=False))
    assert torch.equal(model.store.flat_grad, g0)
    full = model._loss_list(model.forward_backward(inputs, shuffle=None))
    for k in full:
        assert abs(fwd[k] - full[k]) < 1e-6 * max(1.0, abs(full[k])), (k, fwd[k], full[k])


def test_training_lowers_the_loss_and_weights_round_trip(gpu, tmp_path):
    from image_captioning_amd.params import SGD
    model, cfg, Wt = make_tag()
    back = model.get_weights_dict()
    assert set(back) == set(Wt) and all(np.array_equal(back[k], np.asarray(Wt[k], np.float32)) for k in Wt)
    inputs = tag_inputs()
    model.compile(cfg.LEARNING_RATE, cfg.LEARNING_MOMENTUM)
    opt = model.optimizer
    assert isinstance(opt, SGD) and (opt.lr, opt.momentum, opt.clipnorm) == (0.001, 0.9, 5.0) and not model.use_step_graph
    first = model.train_on_batch(inputs)
    assert len(first) == 4 and abs(first[0] - (first[1] + first[2] + first[3] + model.last_losses['reg_loss'])) < 1e-5
    hist = [first] + [model.train_on_batch(inputs) for _ in range(7)]
    print("total loss over eight steps:", [round(h[0], 5) for h in hist])
    assert np.isfinite(hist).all() and hist[-1][0] < hist[0][0]
    assert not model._graphs and opt.iterations == 8
    path = str(tmp_path / "roitag.npz")
    model.save_weights(path)
    other, _, _ = make_tag(Wt=tag_weights(spread=0.5))
    other.load_weights(path)
    a, b = model.get_weights_dict(), other.get_weights_dict()
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    nxt = model._loss_list(model.forward_backward(inputs, shuffle=None))       # the next step's losses (the RPN sums are float atomics)
    again = other._loss_list(other.forward_backward(inputs, shuffle=None))
    for k in nxt:
        assert abs(again[k] - nxt[k]) <= 1e-6 * max(1.0, abs(nxt[k])), (k, again[k], nxt[k])
    assert again['roi_tag_classes_loss'] == nxt['roi_tag_classes_loss']


def _toy_datasets(cfg):
    from image_captioning_amd.train_roi_tags import VisualGenomeDataset
    sets = []
    for ids in (range(4), range(4, 6)):
        ds = VisualGenomeDataset({}, {})
        ds.tag_to_class_id = {"t%d" % i: i for i in range(C)}
        for i in ids:
            r = np.random.RandomState(100 + i)
            n = 2 + i % 3
            y, x = r.randint(0, 60, n), r.randint(0, 60, n)
            rois = np.stack([y, x, y + r.randint(20, 60, n), x + r.randint(20, 60, n)], axis=1)
            tags = (r.rand(n, C) < 0.05).astype(np.int32)
            tags[0, i] = 1
            ds.add_image("toy", image_id=i, path=None, rois=rois.tolist(), captions=[[""]] * n, tags=tags,
                         pixels=np.random.RandomState(i).randint(0, 255, (S, S, 3)).astype(np.uint8))
        ds.prepare()
        sets.append(ds)
    return sets


def test_train_moves_stage_5_into_the_bucket_and_refuses_no_rpn(gpu, tmp_path):
    import os
    model, cfg, Wt = make_tag(images=2, model_dir=str(tmp_path / "logs"), STEPS_PER_EPOCH=2, MAX_GT_INSTANCES=6)
    train, val = _toy_datasets(cfg)
    with pytest.raises(ValueError, match="no_rpn.*backbone_from"):
        model.train(train, val, learning_rate=1e-4, epochs=1, layers="no_rpn")
    assert model.backbone_from is None
    np.random.seed(5)
    hist = model.train(train, val, learning_rate=1e-4, epochs=1, layers="5+")
    assert model.backbone_from == 5 and len(model._plans) == 1                # the serial loop: no second plan
    assert len(hist) == 1 and set(hist[0]) == {p + n for p in ("", "val_") for n in ("loss",) + model.LOSS_NAMES}
    assert all(np.isfinite(v) for v in hist[0].values())
    after = model.get_weights_dict()
    assert 'res5a_branch2a/kernel' in model.store.w and not np.array_equal(after['res5a_branch2a/kernel'], np.asarray(Wt['res5a_branch2a/kernel'], np.float32))
    assert not np.array_equal(after['roitag_class_logits/kernel'], np.asarray(Wt['roitag_class_logits/kernel'], np.float32))
    assert np.array_equal(after['res4a_branch2a/kernel'], np.asarray(Wt['res4a_branch2a/kernel'], np.float32))
    log_dir, last = model.find_last()
    assert last is not None and os.path.basename(last) == "img_cap_roitag_0001.npz" and model.epoch == 1


def test_refusals(gpu):
    from image_captioning_amd.parallel_model import ParallelModel
    from image_captioning_amd.pipeline import JointTrainPipeline
    from image_captioning_amd.roi_tag_model import ROITagRCNN
    s = one_step()
    model, cfg = s['model'], s['cfg']
    with pytest.raises(ValueError, match="bf16"):
        ROITagRCNN("training", cfg, "logs", stage4_blocks=BLOCKS, compute_dtype="bf16")
    with pytest.raises(ValueError, match="JointTrainPipeline"):
        JointTrainPipeline(model)
    with pytest.raises(ValueError, match="step graph"):
        model.use_step_graph = True
    with pytest.raises(ValueError, match="ParallelModel"):
        ParallelModel(model, 1)
    assert model.grad_sync is None and model._outer is model and not model.use_step_graph
    cfg2 = type(cfg)(C)
    cfg2.GPU_COUNT = 2
    with pytest.raises(ValueError, match="GPU_COUNT"):
        ROITagRCNN("training", cfg2, "logs", stage4_blocks=BLOCKS)


# ---- inference ---------------------------------------------------------------------------------------------------------------------
def _restated_generations(rois, classes, scores, window, image_shape, cfg):
    """roi_tag_classification/model.py:631-669 + unmold_generations, restated: boxes to pixels of the molded image, clipped to the
    window; greedy NMS over the clipped boxes in score order (equal scores in np.argsort(kind='stable')[::-1] order, the order both of
    the package's paths use); the best DETECTION_MAX_INSTANCES, rounded; shifted and scaled back to the original image, empty boxes
    dropped."""
    h, w = cfg.IMAGE_SHAPE[:2]
    boxes = np.asarray(rois, np.float64) * np.array([h, w, h, w], np.float64)
    boxes[:, 0] = np.maximum(np.minimum(boxes[:, 0], window[2]), window[0])
    boxes[:, 1] = np.maximum(np.minimum(boxes[:, 1], window[3]), window[1])
    boxes[:, 2] = np.maximum(np.minimum(boxes[:, 2], window[2]), window[0])
    boxes[:, 3] = np.maximum(np.minimum(boxes[:, 3], window[3]), window[1])
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    order = list(np.argsort(np.asarray(scores, np.float64), kind="stable")[::-1])
    keep = []
    while order:
        i = order.pop(0)
        keep.append(i)
        rest = []
        for j in order:
            ih = max(min(boxes[i, 2], boxes[j, 2]) - max(boxes[i, 0], boxes[j, 0]), 0.0)
            iw = max(min(boxes[i, 3], boxes[j, 3]) - max(boxes[i, 1], boxes[j, 1]), 0.0)
            union = area[i] + area[j] - ih * iw
            if not (union > 0 and ih * iw / union > cfg.DETECTION_NMS_THRESHOLD):
                rest.append(j)
        order = rest
    keep = np.asarray(keep[:cfg.DETECTION_MAX_INSTANCES], np.int64)
    refined = np.rint(boxes[keep]).astype(np.int32)
    scale = min(image_shape[0] / (window[2] - window[0]), image_shape[1] / (window[3] - window[1]))
    final = ((refined - np.array([window[0], window[1], window[0], window[1]])) * scale).astype(np.int32)
    ok = (final[:, 2] - final[:, 0]) * (final[:, 3] - final[:, 1]) > 0
    return final[ok], classes[keep[ok]]


def test_generate_roi_tags(gpu):
    from image_captioning_amd import synth
    Wt = tag_weights(spread=5.0, bias=0.0)                   # logits spread around 0 instead of the initialiser's -log(99)
    model, cfg, _ = make_tag("inference", Wt=Wt, POST_NMS_ROIS_INFERENCE=50, DETECTION_MAX_INSTANCES=10)
    img = synth.images(7, 1, 96, S)[0]                       # 96 x 128: a window narrower than the molded image
    # the threshold that leaves half of the RoIs with a confident class (distinct scores) while the other half shares -3.4e38: the
    # median over the RoIs of their largest probability, read from a first pass
    model.generate_roi_tags([img])
    cfg.DETECTION_MIN_CONFIDENCE = float(np.median(model.last_tags[0].cpu().numpy().max(axis=1)))
    assert 0.0 < cfg.DETECTION_MIN_CONFIDENCE < 1.0
    res = {}
    for post in ("host", "device"):
        for mold in ("host", "device"):
            out = model.generate_roi_tags([img], postprocess=post, mold=mold)
            assert len(out) == 1 and set(out[0]) == {"rois", "tags"}
            res[post, mold] = out[0]
    base = res["host", "host"]
    K = base["rois"].shape[0]
    assert 0 < K <= 10 and base["rois"].dtype == np.int32 and base["rois"].shape == (K, 4)
    assert base["tags"].dtype == np.float32 and base["tags"].shape == (K, C) and (base["tags"] > 0).all() and (base["tags"] < 1).all()
    assert np.all(base["rois"][:, 2] > base["rois"][:, 0]) and base["rois"].min() >= 0 and base["rois"][:, [0, 2]].max() <= 96
    for key, r in res.items():
        assert np.array_equal(r["rois"], base["rois"]) and r["rois"].dtype == np.int32, key
        assert np.array_equal(r["tags"].view(np.int32), base["tags"].view(np.int32)), key
    props = model.last_proposals.cpu().numpy()[0]
    probs, scores = (t.cpu().numpy() for t in model.last_tags)
    none = scores == R.NO_SCORE
    print("generate_roi_tags: K %d, %d of %d RoIs without a confident class, p in [%.4f, %.4f]" % (K, none.sum(), len(scores), probs.min(), probs.max()))
    assert 0 < none.sum() < len(scores), "the case should hold scored RoIs and RoIs that share -3.4e38"
    want_scores = R.tag_scores(probs, cfg.DETECTION_MIN_CONFIDENCE)
    assert np.array_equal(none, want_scores == R.NO_SCORE)
    assert (np.abs(scores[~none].astype(np.float64) - want_scores[~none]) <= 1e-6 * np.maximum(1.0, np.abs(want_scores[~none]))).all()
    window = model.mold_inputs([img])[2][0]
    want_rois, want_tags = _restated_generations(props, probs, scores, window, img.shape, cfg)
    assert np.array_equal(want_rois, base["rois"]) and np.array_equal(want_tags.view(np.int32), base["tags"].view(np.int32))
    with pytest.raises(ValueError, match="postprocess"):
        model.generate_roi_tags([img], postprocess="gpu")
