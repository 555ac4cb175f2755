"""Every single-GPU BASELINE config held to the float64 oracle AT ITS OWN SIZE AND DEPTH.

The other model-level files compare with the oracle at reduced sizes (256 px / 2 stage-4 blocks, V = 1000, B = 4) and cover the full
sizes through properties.  Here the oracle itself runs at full size -- it is seconds to tens of seconds of NumPy:

  configs[2]  one 1024 x 1024 image, all 22 stage-4 blocks (101 convolutions, 37 of them in the Winograd form), 32 RoIs: P2..P5 and
              the RoI features of the default plan and of the bf16x3 plan, then those features through the v2-inject decoder at
              V = 10 000 / T = 15: log-probabilities within north_star's 1e-3, greedy token ids bit-exact
              (feature_generation/dense_model.py:143-173,1404-1427; text_generation_model_v2.py:140-166,328-346)
  configs[1]  the v2-inject decoder as written: 64 samples, V = 10 000, window 10 -- predict, loss, every gradient, 2 AMSGrad steps
  configs[0]  the v1 decoder: B = 8, T = 10, V = 1000, trainable RoI head -- dropout off and with replayed recurrent-dropout masks
              (text_generation_model.py:130-294)
  configs[4]  the joint model at 512 x 512, 22 stage-4 blocks, 2000 proposals -> 200 RoIs, V = 50 000: fp32 model against
              M.joint_loss_and_grads (losses 1e-4, gradients 5e-4), bf16 model at its bf16 tolerances
              (dense_img_cap/dense_model.py:1429-1629)

The measured errors are written to gpurun_out/r06_fullsize_parity.json (copied to profiles/ by hand) and quoted in DESIGN.md."""
import json
import os
import time

import numpy as np
import pytest
import torch

from oracle import np_models as M
from oracle import np_oracle as O

import _parity_cuts as PC

pytestmark = pytest.mark.gpu
MEAN = [123.7, 116.8, 103.9]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = {}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    yield torch.device("cuda:0")
    if not MEASURED:                                       # a filtered run that measured nothing leaves the last full record alone
        return
    try:                                                   # the record of what was measured (best effort: the tests do not depend on it)
        out = os.path.join(ROOT, "gpurun_out")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "r06_fullsize_parity.json"), "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)
    except OSError:
        pass


def rel_err(got, want):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    return float(np.abs(got - want).max()) / max(1e-30, float(np.abs(want).max()))


def rel_l2(got, want):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    return float(np.linalg.norm(got - want)) / max(1e-30, float(np.linalg.norm(want)))


def f64(W):
    return {k: np.asarray(v, np.float64) for k, v in W.items()}


# ---------------------------------------------------------------------------------------------
# configs[2]: encoder at 1024 x 1024 x 22 blocks + v2-inject decoder at V = 10 000
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def encoder_oracle(gpu):
    from image_captioning_amd import synth
    W = synth.encoder_weights(0, 22)
    img = synth.images(5, 1, 1024, 1024)
    rois = synth.rois(3, 1, 32, 1024, 1024)
    t0 = time.time()
    feat, maps = M.encoder_features(img, rois, W, MEAN, stage4_blocks=22, return_maps=True)
    MEASURED["configs2_oracle_seconds"] = round(time.time() - t0, 1)
    return W, img, rois, feat, [np.asarray(m) for m in maps[4:]]


@pytest.mark.parametrize("math", ["f32", "f32-wino-f32", "bf16x3"])
def test_configs2_encoder_at_1024px_22_blocks_matches_the_float64_oracle(gpu, encoder_oracle, math):
    """P2..P5 and the 32 RoI features of ONE 1024 x 1024 image through the whole ResNet-101 + FPN (22 stage-4 blocks) against the float64
    oracle.  Default plan ('f32'): fp32 MFMA products on the 1x1 / strided layers, the 37 frozen 3x3 / stride-1 layers in the Winograd
    F(2x2,3x3) form with their products on the bf16 pipe in split arithmetic (wino_products='b3', round 5); 'f32-wino-f32': the same
    layers with fp32 MFMA products (round 3/4's default); bf16x3: the split arithmetic everywhere.  Tolerance 2e-4 of each map's scale -- the same as the 256 px / 2-block test: depth did not cost accuracy (measured:
    see MEASURED / DESIGN.md section 3b)."""
    from image_captioning_amd.encoder import EncoderPlan
    W, img, rois, want_feat, want_maps = encoder_oracle
    plan = EncoderPlan(W, 1, 1024, 1024, "cuda", mean_pixel=MEAN, math=math.split("-")[0], wino_products="f32" if math.endswith("wino-f32") else None)
    if math.startswith("f32"):
        assert len(plan._wwino) == 3 + 4 + 23 + 3 + 4
        kernels = {k for (_, _, _, _, _, k) in plan.conv_table() if k.startswith("wino")}
        assert kernels == ({"wino64_kernel", "wino32_kernel"} if math.endswith("wino-f32") else {"wino32b_kernel"}), kernels
        chained = [n for (n, _, _, _, _, k) in plan.conv_table() if "+" in n]
        assert len(chained) == 2 + 3 and not any(n.startswith("res4") for n in chained)     # one image: stage 4's 128 blocks stay two launches
    for rep in range(3):                                    # eager, capture, replay: the replay is what is compared
        P = plan.forward(torch.as_tensor(img).cuda())
    errs = {}
    for name, a, b in zip(("P2", "P3", "P4", "P5"), P, want_maps):
        errs[name] = rel_err(a.cpu().numpy(), b)
    feat = plan.roi_features(rois).cpu().numpy()
    errs["roi_features"] = rel_err(feat, want_feat)
    errs["roi_features_rel_l2"] = rel_l2(feat, want_feat)
    MEASURED["configs2_encoder_%s" % math] = errs
    for k, v in errs.items():
        assert v < 2e-4, (math, k, v)


def test_configs2_end_to_end_logits_and_greedy_ids_at_full_size(gpu, encoder_oracle):
    """configs[2] end to end at its own size: the device's RoI features (default plan) through the device's v2-inject decoder
    (V = 10 000, window 15) against the oracle's features through the oracle's decoder -- log-probabilities of every as-written
    (RoI, prefix) sample within north_star's 1e-3, greedy token ids of all 32 RoIs bit-exact (the reference's test loop,
    text_generation_model_v2.py:328-346)."""
    from image_captioning_amd import synth
    from image_captioning_amd.encoder import EncoderPlan
    from image_captioning_amd.text_generation_model_v2 import DenseCapConfig, build_model, Adam
    W, img, rois, want_feat, _ = encoder_oracle
    V, Tw = 10000, 15
    plan = EncoderPlan(W, 1, 1024, 1024, "cuda", mean_pixel=MEAN)
    plan.forward(torch.as_tensor(img).cuda())
    feat = plan.roi_features(rois)[0]                                    # [32,7,7,256] on the device
    cfg = DenseCapConfig(V, synth.embedding_matrix(3, V))
    cfg.PADDING_SIZE = Tw
    model = build_model((7, 7, 256), (Tw,), cfg, 256, True, seed=0)
    model.compile(optimizer=Adam(amsgrad=True), loss="categorical_crossentropy")
    Wt = f64(model.get_weights_dict())
    caps = synth.captions_v2(2, 32, Tw, V, full=False, lmin=3)
    roi, words, tgt = M.v2_expand_samples(caps, Tw)
    probs = model.predict([feat.cpu().numpy()[roi], words])
    want_p, _ = M.v2_forward(Wt, want_feat[0][roi], words, True)
    dlog = float(np.abs(np.log(probs + 1e-30) - np.log(want_p + 1e-30)).max())
    MEASURED["configs2_end_to_end"] = dict(samples=int(len(roi)), logprob_abs_err=dlog, prob_abs_err=float(np.abs(probs - want_p).max()))
    assert dlog < 1e-3, dlog
    worst = 0.0
    for r in range(32):
        ids, rows = model.greedy_decode(feat[r])
        want_ids, want_rows = M.v2_greedy_decode(Wt, want_feat[0][r], Tw, Tw - 1)
        np.testing.assert_array_equal(ids, want_ids)
        worst = max(worst, float(np.abs(rows - want_rows).max()))
    MEASURED["configs2_end_to_end"]["greedy_prob_abs_err"] = worst
    assert worst < 1e-4


# ---------------------------------------------------------------------------------------------
# configs[1]: v2-inject decoder as written, 64 samples, V = 10 000, window 10
# ---------------------------------------------------------------------------------------------

def test_configs1_as_written_at_full_size(gpu):
    """text_generation_model_v2.py as the script runs it: batch = 64 (RoI, prefix) samples, word window 10, V = 10 000 --
    predict, Keras categorical cross-entropy, the gradient of every trainable weight, two AMSGrad steps."""
    from image_captioning_amd import synth
    from image_captioning_amd.text_generation_model_v2 import DenseCapConfig, build_model, Adam
    V, Tw, B = 10000, 10, 64
    cfg = DenseCapConfig(V, synth.embedding_matrix(3, V))
    cfg.PADDING_SIZE = Tw
    model = build_model((7, 7, 256), (Tw,), cfg, 256, True, seed=0)
    model.compile(optimizer=Adam(amsgrad=True), loss="categorical_crossentropy")
    Wt = f64(model.get_weights_dict())
    rng = np.random.default_rng(1)
    feat_r = rng.standard_normal((12, 7, 7, 256)).astype(np.float32)
    caps = synth.captions_v2(2, 12, Tw + 3, V, full=False, lmin=2)      # some prefixes longer than the window
    roi, words, tgt = M.v2_expand_samples(caps, Tw)
    assert len(roi) >= B
    roi, words, tgt = roi[:B], words[:B], tgt[:B]
    feat = feat_r[roi]
    onehot = np.zeros((B, V), np.float32)
    onehot[np.arange(B), tgt] = 1
    probs = model.predict([feat, words])
    want_p, _ = M.v2_forward(Wt, feat, words, True)
    rec = dict(logprob_abs_err=float(np.abs(np.log(probs + 1e-30) - np.log(want_p + 1e-30)).max()), grad_rel_err={}, weight_abs_err={})
    assert np.abs(probs - want_p).max() < 1e-5 and rec["logprob_abs_err"] < 1e-3
    opt = M.AMSGrad()
    for step in range(2):
        loss, G, _ = M.v2_loss_and_grads(Wt, feat, words, tgt, True)
        got_loss = model.train_on_batch([feat, words], onehot)
        assert abs(got_loss - loss) < 1e-4 * max(1.0, abs(loss)), (step, got_loss, loss)
        for k in G:
            if np.abs(G[k]).max() < 1e-12:
                continue
            e = rel_err(model.store.grad[k].cpu().numpy(), G[k])
            rec["grad_rel_err"][k] = max(rec["grad_rel_err"].get(k, 0.0), e)
            assert e < 2e-4, (k, step, e)
        opt.step(Wt, G)
        for k in G:
            e = float(np.abs(model.store.w[k].cpu().numpy() - Wt[k]).max())
            rec["weight_abs_err"][k] = max(rec["weight_abs_err"].get(k, 0.0), e)
            assert e < 2e-5, (k, step, e)
    MEASURED["configs1_as_written"] = rec


# ---------------------------------------------------------------------------------------------
# configs[0]: v1 decoder, B = 8, T = 10, V = 1000, trainable head
# ---------------------------------------------------------------------------------------------

def _make_v1(V, T, B, seed=0):
    from image_captioning_amd import synth
    from image_captioning_amd.text_generation_model import DenseCapConfig, build_lstm_model, Adam, roi_caption_loss
    cfg = DenseCapConfig(V, synth.embedding_matrix(seed + 3, V), B)
    cfg.PADDING_SIZE = T
    model = build_lstm_model([7, 7, 256], cfg, 512, 'training', seed=seed)
    model.compile(optimizer=Adam(amsgrad=True), loss=roi_caption_loss)
    return model, cfg


def test_configs0_v1_decoder_at_full_size_dropout_off(gpu):
    """text_generation_model.py at configs[0]'s size (B = 8 RoIs, T = 10, V = 1000, the RoI head trainable): the single masked pass
    against the oracle's T-prefix TimeDistributed graph -- probabilities, roi_caption_loss, every gradient, two AMSGrad steps."""
    from image_captioning_amd import synth
    from image_captioning_amd.text_generation_model import caption_targets
    V, T, B = 1000, 10, 8
    model, cfg = _make_v1(V, T, B)
    model.recurrent_dropout = 0.0
    Wt = f64(model.get_weights_dict())
    rng = np.random.default_rng(21)
    feat = rng.standard_normal((B, 7, 7, 256)).astype(np.float32)
    caps = synth.captions_v1(22, B, T, V, lmin=1, lmax=8)
    probs = model.predict([feat, caps])
    want_p, _ = M.v1_training_forward(Wt, feat, caps)
    rec = dict(logprob_abs_err=float(np.abs(np.log(probs + 1e-30) - np.log(want_p + 1e-30)).max()), grad_rel_err={})
    assert probs.shape == (B, T, V) and np.abs(probs - want_p).max() < 1e-5 and rec["logprob_abs_err"] < 1e-3
    onehot = caption_targets(caps, V)
    opt = M.AMSGrad()
    for step in range(2):
        loss, G, _ = M.v1_loss_and_grads(Wt, feat, caps)
        got = model.train_on_batch([feat, caps], onehot)
        assert abs(got - loss) < 1e-4 * max(1.0, abs(loss))
        assert set(G) == set(model.trainable_weights)
        for k in G:
            e = rel_err(model.store.grad[k].cpu().numpy(), G[k])
            rec["grad_rel_err"][k] = max(rec["grad_rel_err"].get(k, 0.0), e)
            assert e < 3e-4, (k, step, e)
        opt.step(Wt, G)
        for k in G:
            assert np.abs(model.store.w[k].cpu().numpy() - Wt[k]).max() < 2e-5, (k, step)
    MEASURED["configs0_dropout_off"] = rec


def test_configs0_v1_decoder_at_full_size_with_replayed_dropout_masks(gpu):
    """The same size with the reference's recurrent_dropout = 0.2 (text_generation_model.py:141-142): the device draws the masks, the
    oracle's T-prefix graph replays them -- loss and every gradient."""
    from image_captioning_amd import synth
    from image_captioning_amd.text_generation_model import caption_targets
    V, T, B = 1000, 10, 8
    model, cfg = _make_v1(V, T, B)
    assert model.recurrent_dropout == 0.2
    Wt = f64(model.get_weights_dict())
    rng = np.random.default_rng(1)
    feat = rng.standard_normal((B, 7, 7, 256)).astype(np.float32)
    caps = synth.captions_v1(2, B, T, V, lmin=1, lmax=8)
    tg = caption_targets(caps)
    loss_rows, _ = model._forward_train(model._dev_feat(feat), caps, tg, want_grad=True)
    model._backward()
    masks = [m.astype(np.float64) for m in model.last_rec_masks]
    assert all(set(np.unique(m)) <= {0.0, 1.25} and m.shape == (4, B, 512) for m in masks)
    want_loss, G, _ = M.v1_loss_and_grads(Wt, feat.astype(np.float64), caps, rec_masks=tuple(masks))
    got_loss = float(loss_rows.mean().item())
    assert abs(got_loss - want_loss) < 1e-5 * max(1.0, abs(want_loss))
    rec = {}
    for k, g in G.items():
        rec[k] = rel_err(model.store.grad[k].cpu().numpy(), g)
        assert rec[k] < 3e-4, (k, rec[k])
    MEASURED["configs0_dropout_replayed"] = dict(grad_rel_err=rec)


# ---------------------------------------------------------------------------------------------
# configs[4]: joint model at 512 x 512 x 22 blocks, 2000 -> 200 RoIs, V = 50 000
# ---------------------------------------------------------------------------------------------

def _joint_full(compute_dtype, conv_math, S=512, V=50000, T=15, blocks=22, B=1):
    """Model, config, reference-layout weights and one step's generator inputs for B images (IMAGES_PER_GPU = B)."""
    from image_captioning_amd import synth, utils
    from image_captioning_amd.config import Config
    from image_captioning_amd.dense_model import DenseImageCapRCNN, build_rpn_targets

    class Cfg(Config):
        NAME = "joint"
        IMAGES_PER_GPU = B
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
        PADDING_SIZE = T
        VOCABULARY_SIZE = V
        EMBEDDING_SIZE = 300
        RECURRENT_DROPOUT = 0.0          # parity against the deterministic oracle graph
    cfg = Cfg()
    assert cfg.POST_NMS_ROIS_TRAINING == 2000 and cfg.TRAIN_ROIS_PER_IMAGE == 200          # the reference's own budget
    Wt = dict(synth.encoder_weights(0, blocks), **synth.rpn_weights(4))
    Wt['rpn_conv_shared/kernel'] = Wt['rpn_conv_shared/kernel'] * np.float32(0.02)
    Wt['rpn_bbox_pred/kernel'] = Wt['rpn_bbox_pred/kernel'] * np.float32(0.3)
    Wt.update(synth.head_weights(1))
    Wt['mrcnn_class_conv1/kernel'] = Wt['mrcnn_class_conv1/kernel'] * np.float32(0.05)
    Wt.update(synth.v1_weights(2, V))
    Wt['imgcap_embedding_layer/embeddings'] = synth.embedding_matrix(3, V)
    cfg.EMBEDDING_WEIGHTS = Wt['imgcap_embedding_layer/embeddings']
    model = DenseImageCapRCNN("training", cfg, "logs", stage4_blocks=blocks, compute_dtype=compute_dtype, conv_math=conv_math)
    model.set_weights(Wt)
    rng = np.random.RandomState(0)
    img = synth.images(7, B, S, S)
    # ground truth = some of the (random-weight) RPN's own proposals, so that DetectionTargetLayer finds positive RoIs; with B > 1 the
    # images get DIFFERENT numbers of GT boxes, positive anchors and caption lengths: the pooled means then differ from means of means
    plan = model.plan()
    plan.forward(torch.as_tensor(img))
    props_all = plan.proposals().cpu().numpy().astype(np.float64) * S
    anchors = utils.generate_pyramid_anchors(cfg.RPN_ANCHOR_SCALES, cfg.RPN_ANCHOR_RATIOS, cfg.BACKBONE_SHAPES, cfg.BACKBONE_STRIDES, 1)
    gt_caps = np.zeros((B, cfg.MAX_GT_INSTANCES, T), np.int32)
    gt_boxes = np.zeros((B, cfg.MAX_GT_INSTANCES, 4), np.int32)
    matches, deltas_all = [], []
    for b in range(B):
        props = props_all[b]
        big = props[((props[:, 2] - props[:, 0]) >= 24) & ((props[:, 3] - props[:, 1]) >= 24)]
        boxes = np.rint(big[:40 if b == 0 else 12]).astype(np.int32)
        n_gt = boxes.shape[0]
        assert n_gt >= 8, "the random RPN produced too few usable proposals"
        caps = synth.captions_v1(9 + b, n_gt, T, V, lmin=3, lmax=min(12, T - 2) if b == 0 else max(3, min(6, T - 4))).astype(np.int32)
        match, deltas = build_rpn_targets(img[b].shape, anchors, caps, boxes, cfg, rng)
        gt_caps[b, :n_gt], gt_boxes[b, :n_gt] = caps, boxes
        matches.append(match[:, None])
        deltas_all.append(deltas)
    return model, cfg, Wt, [img, np.zeros((B, 12)), np.stack(matches), np.stack(deltas_all), gt_caps, gt_boxes]


def _oracle_cfg(cfg):
    return dict(mean_pixel=MEAN, scales=cfg.RPN_ANCHOR_SCALES, ratios=cfg.RPN_ANCHOR_RATIOS, strides=cfg.BACKBONE_STRIDES,
                proposal_count=cfg.POST_NMS_ROIS_TRAINING, nms=cfg.RPN_NMS_THRESHOLD, train_rois=cfg.TRAIN_ROIS_PER_IMAGE,
                positive_ratio=cfg.ROI_POSITIVE_RATIO, weight_decay=cfg.WEIGHT_DECAY, T=cfg.PADDING_SIZE)


TRUNK_CACHE = {}          # the float64 ResNet maps of the configs[4] test image: computed by the first leg, reused by a later evaluation
ORACLE_CACHE = {}         # the fp32 leg's RoI sample and the oracle's result on it: the bf16 leg reuses both


def _joint_oracle(Wt, cfg, inputs, targets, blocks, head_masks=None):
    img, _, match, tdelta, gt_caps, gt_boxes = inputs
    return M.joint_loss_and_grads(f64(Wt), img[0], match[0, :, 0], tdelta[0], gt_caps[0], gt_boxes[0], _oracle_cfg(cfg), stage4_blocks=blocks,
                                  targets_override=targets, trunk_cache=TRUNK_CACHE.setdefault((img.shape, blocks), {}), head_masks=head_masks)


def _grads_as_reference(model):
    st = model.store
    saved = st.flat.clone()
    st.flat.copy_(st.flat_grad)
    try:
        return model.get_weights_dict()
    finally:
        st.flat.copy_(saved)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_configs4_joint_step_at_512px_22_blocks_50k_vocabulary(gpu, dtype):
    """configs[4] with the reference's own budgets (2000 proposals -> 200 RoIs, <= 66 positive, 15-token captions, V = 50 000, all 22
    stage-4 blocks) at 512 x 512: the four loss terms and the gradient of every trainable weight against the float64 oracle, given the
    RoI sample the device drew and (fp32 leg) the RoI head's ReLU decisions the device took -- both checked first: the RPN heads against
    the oracle's, the proposals exactly from the device's scores, the sample exactly from those proposals and the step's ground truth, the
    head's GEMM outputs and masks against the oracle's pre-activations (tests/_parity_cuts.py).  fp32 model: losses 1e-4, gradients 5e-4
    of each tensor's largest entry.  (The bf16 leg is not handed masks of its own: re-running the oracle's backward with them would be a
    second decoder evaluation; it keeps its tolerances against the fp32 leg's result.)  bf16 model (compute_dtype
    'bf16' + bf16 storage between the convolutions -- configs[4] as specified): losses 1e-2, gradients 5e-2 ... 1e-1 in relative L2
    norm (the tolerances of the reduced-size bf16 tests).  That states how far bf16 training is from fp32; how the bf16 step is WIRED --
    which products run on the bf16 pipe, what each of them reads, every scale and count -- is held at 128 px by
    tests/test_gpu_models.py::test_joint_model_bf16_step_tracks_the_fp32_oracle against the oracle that rounds where the device rounds
    (3e-7 ... 3e-6), with the product sites asserted equal to this size's (tests/_bf16_sites.py); a second float64 evaluation at 512 px
    would cost minutes."""
    bf = dtype == "bf16"
    blocks = 22
    model, cfg, Wt, inputs = _joint_full("bf16" if bf else "f32", "bf16" if bf else None)
    # ONE oracle evaluation serves both legs: the fp32 leg draws the RoI sample on the device and evaluates the oracle
    # on it; the bf16 leg is handed the same sample (forward_backward(targets=)) and is held to the same oracle result.  (The oracle's
    # cost is its T-prefix decoder at 50 000 words in float64, not the trunk: sharing the trunk alone saved nothing.)
    shared = ORACLE_CACHE.get("configs4_512")
    if bf and shared is not None:
        inputs = shared["inputs"]                          # (_joint_full draws the ground truth from the model's OWN proposals: the legs share the fp32 leg's)
    for rep in range(2):                                   # eager plan, then captured graph
        if bf and shared is not None:
            losses = model._loss_list(model.forward_backward(inputs, targets=shared["targets"]))
        else:
            losses = model._loss_list(model.forward_backward(inputs, shuffle=None))
    tg = model.last_targets
    assert 0 < tg['npos'] <= 66 and tg['npos'] + tg['nneg'] <= 200
    t0 = time.time()
    if bf and shared is not None:
        want, G, aux = shared["result"]
    else:
        dev_acc, dev_hact = PC.device_head_buffers(model.caption_model)
        want, G, aux = _joint_oracle(Wt, cfg, inputs, (tg['rois'], tg['caps']), blocks, head_masks=None if bf else PC.device_head_masks(dev_hact))
        if not bf:
            ORACLE_CACHE["configs4_512"] = dict(inputs=inputs, targets=(tg['rois'], tg['caps']), result=(want, G, aux))
    rec = dict(oracle_seconds=round(time.time() - t0, 1), npos=int(tg['npos']), nneg=int(tg['nneg']), losses={}, grads={})
    rec["oracle_shared_with_the_fp32_leg"] = bool(bf and shared is not None)
    if not bf:                                              # the device's own proposals reproduce the oracle's sample unless near-tied scores swapped
        agree = sum(1 for r in tg['rois'][:tg['npos'] + tg['nneg']] if np.abs(aux['proposals'] - r).sum(1).min() < 1e-5)
        rec["rois_found_among_the_oracles_proposals"] = agree
        assert agree >= 0.8 * (tg['npos'] + tg['nneg'])
        _, head_errs = PC.check_step_decisions(model, tg, aux, _oracle_cfg(cfg), inputs[4], inputs[5])
        rec["rpn_heads_worst_rel_err"] = max(head_errs.values())
        _, rec["head_decisions"] = PC.check_head_decisions(dev_acc, dev_hact, PC.oracle_head_cache(aux), Wt)
        rec["head_decisions"]["c_acc"] = list(PC.C_ACC)
    ltol = 1e-2 if bf else 1e-4
    for k in ('imgcap_loss', 'rpn_class_loss', 'rpn_bbox_loss', 'reg_loss', 'loss'):
        rec["losses"][k] = (float(losses[k]), float(want[k]))
        assert abs(losses[k] - want[k]) < ltol * max(1.0, abs(want[k])), (k, losses[k], want[k])
    got = _grads_as_reference(model)
    for k in M.joint_trainable(Wt):
        rec["grads"][k] = rel_l2(got[k], G[k]) if bf else rel_err(got[k], G[k])
    MEASURED["configs4_joint_512px_%s" % dtype] = rec
    worst = sorted(rec["grads"].items(), key=lambda kv: -kv[1])[:6]
    assert all(np.isfinite(v) for v in rec["grads"].values())
    assert worst[0][1] < (1e-1 if bf else 5e-4), worst
    del model
    torch.cuda.empty_cache()


def test_configs4_joint_step_two_images_per_gpu_pools_the_losses_over_the_batch(gpu):
    """IMAGES_PER_GPU = 2 (the reference's batched graph: config.py:35, DetectionTargetLayer over utils.batch_slice
    dense_model.py:531-572): two 512 x 512 images with DIFFERENT numbers of GT boxes / positive anchors / caption tokens in one step.
    Losses and every gradient against M.joint_loss_and_grads_batch -- each loss the mean over the batch's union of anchors / caption
    positions (rpn_class_loss_graph :877-900, rpn_bbox_loss_graph :903-933, imgcap_caption_loss_graph :936-946), given the RoI samples
    the device drew and the RoI head's ReLU decisions it took; fp32: losses 1e-4, gradients 5e-4 of each tensor's largest entry, the
    head's included, with nothing set aside.  What is handed to the oracle is checked first (tests/_parity_cuts.py): the RPN heads per
    image, the proposals exactly from the device's scores, each image's sample exactly from ITS proposals and ITS ground truth, the head's
    GEMM outputs within c_acc u |x| @ |K| and its masks equal to the oracle's signs outside the close set.  Full depth is the one-image test's job: two
    stage-4 blocks and V = 10 000 here keep the float64 oracle at seconds (8-token captions: its T-prefix decoder is quadratic in T)."""
    blocks, V = 2, 10000
    model, cfg, Wt, inputs = _joint_full("f32", None, V=V, T=8, blocks=blocks, B=2)      # (T = 8: the oracle's T-prefix graph costs T^2 LSTM steps per RoI)
    for rep in range(2):
        losses = model._loss_list(model.forward_backward(inputs, shuffle=None))
    tg = model.last_targets
    assert tg['rois'].shape == (2, 200, 4) and np.all(tg['npos'] > 0) and np.all(tg['npos'] + tg['nneg'] <= 200)
    match = inputs[2][:, :, 0]
    dev_acc, dev_hact = PC.device_head_buffers(model.caption_model)
    want, G, auxes = M.joint_loss_and_grads_batch(f64(Wt), inputs[0], match, inputs[3], inputs[4], inputs[5], _oracle_cfg(cfg),
                                                  (tg['rois'], tg['caps']), stage4_blocks=blocks, head_masks=PC.device_head_masks(dev_hact))
    _, head_errs = PC.check_step_decisions(model, tg, auxes, _oracle_cfg(cfg), inputs[4], inputs[5])
    _, decisions = PC.check_head_decisions(dev_acc, dev_hact, PC.oracle_head_cache(auxes), Wt)
    # the pooled means are not the means of the per-image means here (the images' counts differ on purpose)
    n_sel = (match != 0).sum(1)
    tok = np.array([a['count'] for a in auxes])
    assert tok[0] != tok[1] and (match == 1).sum(1)[0] != (match == 1).sum(1)[1], (tok, n_sel)
    rec = dict(losses={}, grads={}, tokens=tok.tolist(), positives=(match == 1).sum(1).tolist())
    for k in ('imgcap_loss', 'rpn_class_loss', 'rpn_bbox_loss', 'reg_loss', 'loss'):
        rec["losses"][k] = (float(losses[k]), float(want[k]))
        assert abs(losses[k] - want[k]) < 1e-4 * max(1.0, abs(want[k])), (k, losses[k], want[k])
    got = _grads_as_reference(model)
    for k in M.joint_trainable(Wt):
        rec["grads"][k] = rel_err(got[k], G[k])
    rec["head_decisions"] = dict(decisions, c_acc=list(PC.C_ACC))
    rec["rpn_heads_worst_rel_err"] = max(head_errs.values())
    MEASURED["configs4_joint_2_images_per_gpu"] = rec
    worst = sorted(rec["grads"].items(), key=lambda kv: -kv[1])[:6]
    assert worst[0][1] < 5e-4, (worst, decisions)                           # every trainable tensor, mrcnn_class_* included: no channel set aside
    # one captured optimizer step on the same batch: the step graph takes the batched launches too
    model.compile(1e-3)
    before = model.store.flat.clone()
    for _ in range(4):
        out = model.train_on_batch(inputs)
    assert np.isfinite(out).all() and not torch.equal(before, model.store.flat)
    del model
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_configs4_joint_step_is_bit_identical_from_call_to_call(gpu, dtype):
    """The same weights and the same batch through the whole configs[4] step (every kernel of the path at its real shape, ~430 launches,
    ~10^5 workgroups): the four losses and the gradient of every trainable weight come out with identical bits every time -- nothing in the
    path is order-dependent (no float atomics; every reduction has a fixed order).  Round 6 found a kernel that did not hold this
    (tests/test_gpu_bf16.py::test_vocab_ce_is_bit_identical_from_call_to_call); this is the same check over the whole step."""
    bf = dtype == "bf16"
    model, cfg, Wt, inputs = _joint_full("bf16" if bf else "f32", "bf16" if bf else None)
    first = None
    for call in range(14 if bf else 6):                    # call 0: eager plan; later calls: the captured graph
        losses = model.forward_backward(inputs, shuffle=None)
        got = (losses.clone() if torch.is_tensor(losses) else torch.as_tensor(np.asarray(losses)), model.store.flat_grad.clone())
        if first is None:
            first = got
            continue
        assert torch.equal(got[0], first[0]), (call, got[0].tolist(), first[0].tolist())
        diff = got[1] != first[1]
        assert not bool(diff.any()), "call %d: %d gradient entries differ from the first call's (first at flat index %d)" % (
            call, int(diff.sum()), int(torch.nonzero(diff)[0]))
    del model
    torch.cuda.empty_cache()
