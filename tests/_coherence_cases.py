"""What tests/test_gpu_weight_coherence.py and tests/test_coherence_inventory.py share.  A plain module, no fixtures; the package is
imported inside the functions, as in the test files.

Kernels do not read master weights: they read copies derived from them (Winograd packs, chained-pointwise packs, folded BatchNorm
operands, bf16 mirrors and casts, data-gradient packs, packed recurrent kernels) and captured graphs that bake their addresses.  The GPU
file holds every model to one rule -- after a HISTORY that created those copies and a weight-change EVENT, a model gives, bit for bit,
the OBSERVABLES of a fresh model that was built on the resulting weights and never ran the history.  This module has

  DERIVED_FORMS      every call site of a weight-derivation function in the package -> the GPU test that covers it (the CPU inventory
                     test keeps the table complete against the package's source),
  the model kinds    (a factory on given weights, a history, observables, for training models one further step) and the events,
  the two comparisons: same() -- torch.equal / np.array_equal -- and moved(), the guard against a vacuous case: on FRESH models alone,
                     the old and the new weights give observables more than 1e-3 of the largest magnitude apart.
"""
import numpy as np

# ------------------------------------------------------------------------------------------------------------------------------------
# the inventory: (file under image-captioning_amd/, enclosing function, callee) -> a test function of GPU_FILE, or REBUILT
# ------------------------------------------------------------------------------------------------------------------------------------
GPU_FILE = "test_gpu_weight_coherence.py"
REBUILT = "rebuilt on every call"        # valid only for a call that is under no `is None` / membership (cache-miss) branch

DERIVED_FUNCTIONS = ("winograd_pack", "winograd_pack_b3", "pw_chain_pack", "pw_chain_pack_b3", "lstm_pack_urec", "conv_weight_dgrad_pack",
                     "bn_fold", "fold_bn", "refresh_shadow", "to_bf16")

_JOINT = "test_joint_training_follows_a_weight_event"
_TRUNK = "test_joint_trainable_stage_follows_a_weight_event"

DERIVED_FORMS = {
    # the encoder plan: once per plan -- the plan goes when a backbone tensor changes
    ("encoder.py", "EncoderPlan._upload", "fold_bn"): _JOINT,                       # plan-owned folded BN of the frozen backbone
    ("encoder.py", "EncoderPlan._conv", "winograd_pack"): _JOINT,                   # U packs, fp32 products (DCAP_WINO_PRODUCTS=f32) ...
    ("encoder.py", "EncoderPlan._conv", "winograd_pack_b3"): _JOINT,                # ... and split-bf16, the default
    ("encoder.py", "EncoderPlan._chain", "pw_chain_pack"): _JOINT,                  # the stage-2 seam takes fp32 products ...
    ("encoder.py", "EncoderPlan._chain", "pw_chain_pack_b3"): _JOINT,               # ... the stage-3 / 4 tile form split-bf16
    ("encoder.py", "EncoderPlan._conv_bf16", "to_bf16"): _JOINT,                    # per-plan bf16 cast of a frozen kernel (_wb)
    ("encoder.py", "EncoderPlan._run_ops", "to_bf16"): REBUILT,                     # the plan's cast ops: inside every forward
    ("encoder.py", "EncoderPlan._run_ops", "bn_fold"): REBUILT,                     # trainable stages: folded inside every forward
    # the joint step's data-gradient packs and per-step bf16 casts
    ("dense_model.py", "DenseImageCapRCNN._rpn_backward", "conv_weight_dgrad_pack"): _JOINT,
    ("dense_model.py", "DenseImageCapRCNN._fpn_backward", "conv_weight_dgrad_pack"): _JOINT,
    ("dense_model.py", "DenseImageCapRCNN._stage_backward", "conv_weight_dgrad_pack"): _TRUNK,
    ("dense_model.py", "DenseImageCapRCNN._cast_cached", "to_bf16"): _JOINT,        # one cast per step and key (the rotated RPN kernel)
    # the bf16 shadow of the parameter bucket
    ("params.py", "ParamStore.enable_bf16_shadow", "refresh_shadow"): _JOINT,
    ("params.py", "ParamStore.refresh_shadow", "to_bf16"): _JOINT,
    ("params.py", "ParamStore.assign", "refresh_shadow"): "test_store_assign_refreshes_the_shadow_of_a_mirrored_weight",
    ("keras_like.py", "KerasLikeModel._weights_changed", "refresh_shadow"): _JOINT,
    # folded heads
    ("mask_rcnn_model.py", "DetectTop.folded", "bn_fold"): "test_maskrcnn_folded_mask_head_follows_every_way_its_weights_change",
    ("text_generation_model_v2.py", "CaptionModelV2._weights_changed", "refresh_shadow"): "test_v2_decoder_follows_a_weight_event",
    ("text_generation_model_v2.py", "CaptionModelV2._weights_changed", "fold_bn"): "test_v2_decoder_follows_a_weight_event",
    # packed recurrent kernels: once per decode call
    ("text_generation_model_v2.py", "CaptionModelV2._decode_setup", "lstm_pack_urec"): "test_v2_decoder_follows_a_weight_event",
    ("text_generation_model.py", "CaptionModelV1._decode_setup", "lstm_pack_urec"): "test_v1_decoder_follows_a_weight_event",
}

# to_bf16 of something that is no weight (activations, gradients): (file, enclosing function).  Every to_bf16 call site of the package
# is in DERIVED_FORMS or here, so a new one has to be classified.
BF16_CASTS_OF_NON_WEIGHTS = {
    ("dense_model.py", "DenseImageCapRCNN._wgrad"),                # a convolution's input activations
    ("text_generation_model.py", "_Act.b"),                       # an activation / gradient matrix of the GEMM engine
    ("parallel_model.py", "GradAllReduce._round"),                # a gradient range going on the wire
}

# ------------------------------------------------------------------------------------------------------------------------------------
# comparisons
# ------------------------------------------------------------------------------------------------------------------------------------
GUARD = 1e-3


def _np(x):
    import torch
    if isinstance(x, torch.Tensor):
        x = x.detach()
        return (x.float() if x.dtype == torch.bfloat16 else x).cpu().numpy()
    return np.asarray(x)


def same(got, want, where=""):
    """Bit for bit, every observable (dicts of tensors / arrays with the same keys)."""
    assert sorted(got) == sorted(want), (where, sorted(got), sorted(want))
    for k in sorted(want):
        a, b = _np(got[k]), _np(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (where, k, a.shape, b.shape, a.dtype, b.dtype)
        if not np.array_equal(a, b):
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            raise AssertionError("%s: %s differs from the fresh model's: %d of %d elements, largest difference %.3e (largest magnitude %.3e)"
                                 % (where, k, int((a != b).sum()), a.size, d.max(), np.abs(b.astype(np.float64)).max()))


def distance(old, new):
    """Largest difference over the largest magnitude of `new`; inf when the shapes differ (another number of detections)."""
    a, b = _np(old).astype(np.float64), _np(new).astype(np.float64)
    if a.shape != b.shape:
        return float("inf")
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-30)


def moved(old, new, moves, where=""):
    """The guard, on fresh models' observables: each float observable named in `moves` is more than GUARD of its largest magnitude
    away from what the old weights give -- a stale copy cannot hide in rounding.  The float observables NOT named lie upstream of the
    changed tensor: they must not have moved at all."""
    floats = [k for k in sorted(new) if _np(new[k]).dtype.kind == "f"]
    assert set(moves) <= set(floats), (where, moves, floats)
    bad = [k for k in floats for o in (old, new) if not np.isfinite(_np(o[k])).all()]
    assert not bad, "%s: %s is not finite: nothing can be compared" % (where, bad)
    for k in floats:
        d = distance(old[k], new[k])
        print("  guard %-28s %-14s old -> new weights: %.3e of the largest magnitude" % (where, k, d))
        if k in moves:
            assert d > GUARD, "%s: the event moves %s by only %.3e: the case could not see a stale copy" % (where, k, d)
        else:
            assert d == 0.0, "%s: %s is upstream of the changed tensor and moved by %.3e" % (where, k, d)


def bumped(name, array):
    """The single-tensor event's new value: a bias, beta or moving mean + 0.5, anything else x 1.5."""
    a = np.asarray(array, np.float32)
    return a + np.float32(0.5) if name.rsplit("/", 1)[1] in ("bias", "beta", "moving_mean") else a * np.float32(1.5)


_OLD = {}


def old_observables(key, make):
    """The observables of a fresh model on the OLD weights, once per kind (its history is deterministic: so are the old weights)."""
    if key not in _OLD:
        _OLD[key] = make()
    return _OLD[key]


# ------------------------------------------------------------------------------------------------------------------------------------
# the joint model (tests/_joint_cases.make_joint's shape: S = 128, V = 24, T = 5, one stage-4 block, 12 train RoIs)
# ------------------------------------------------------------------------------------------------------------------------------------
S, V, T, BLOCKS, ROIS = 128, 24, 5, 1, 12
LR = 1e-4
_W = {}


def backbone_weights(variant):
    from image_captioning_amd import synth
    s = 10 * variant
    Wt = dict(synth.encoder_weights(s, BLOCKS), **synth.rpn_weights(4 + s))
    Wt['rpn_conv_shared/kernel'] = Wt['rpn_conv_shared/kernel'] * np.float32(0.05)
    Wt['rpn_bbox_pred/kernel'] = Wt['rpn_bbox_pred/kernel'] * np.float32(0.3)
    Wt.update(synth.head_weights(1 + s))
    Wt['mrcnn_class_conv1/kernel'] = Wt['mrcnn_class_conv1/kernel'] * np.float32(0.05)
    return Wt


def joint_weights(variant=0):
    """variant 0: make_joint's weights; 1: the same layers drawn from other seeds (the event's W').  The arrays are shared: read only."""
    if ("joint", variant) not in _W:
        from image_captioning_amd import synth
        Wt = backbone_weights(variant)
        Wt.update(synth.v1_weights(2 + 10 * variant, V))
        Wt['imgcap_embedding_layer/embeddings'] = synth.embedding_matrix(3 + 10 * variant, V)
        _W[("joint", variant)] = Wt
    return dict(_W[("joint", variant)])


def _joint_config(W):
    from image_captioning_amd.config import Config

    class Cfg(Config):
        NAME = "joint"
        IMAGES_PER_GPU = 1
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
        POST_NMS_ROIS_TRAINING = 60
        POST_NMS_ROIS_INFERENCE = 40
        DETECTION_MAX_INSTANCES = 10
        TRAIN_ROIS_PER_IMAGE = ROIS
        PADDING_SIZE = T
        VOCABULARY_SIZE = V
        EMBEDDING_SIZE = 300
        RECURRENT_DROPOUT = 0.0
    cfg = Cfg()
    cfg.EMBEDDING_WEIGHTS = W['imgcap_embedding_layer/embeddings']
    return cfg


def joint_model(W, mode="training", dtype="f32", layers=None):
    """A fresh joint model on the weights W; layers: set_trainable(LAYER_REGEX[layers]) first (ResNet stages join the bucket)."""
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    model = DenseImageCapRCNN(mode, _joint_config(W), "logs", stage4_blocks=BLOCKS, compute_dtype=dtype, conv_math="bf16" if dtype == "bf16" else None)
    if layers is not None:
        model.set_trainable(model.LAYER_REGEX[layers])
    model.set_weights(W)
    return model


def train_inputs(seed=8):
    import torch
    from _joint_cases import joint_inputs
    inputs = joint_inputs(S, V, T, seed=seed)
    inputs[0] = torch.tensor(inputs[0], device="cuda")
    return inputs


def fixed_sample(inputs, caps=None):
    """A DetectionTargetLayer sample that does not depend on the weights: the three GT boxes and a shifted copy of each with their
    targets (positives), four boxes elsewhere (negatives), two rows of padding."""
    gt = np.asarray(inputs[5][0, :3], np.float32) / np.float32(S)
    caps = np.asarray(inputs[4][0, :3]) if caps is None else caps
    rois = np.zeros((ROIS, 4), np.float32)
    rows = np.zeros((ROIS,) + caps.shape[1:], caps.dtype)
    rois[:3], rows[:3] = gt, caps
    rois[3:6], rows[3:6] = np.clip(gt + np.float32(0.03), 0, 1), caps
    rois[6:10] = np.array([[0.5, 0.5, 0.9, 0.95], [0.05, 0.6, 0.3, 0.9], [0.6, 0.05, 0.95, 0.4], [0.2, 0.2, 0.8, 0.8]], np.float32)
    return rois, rows


def train_history(model, inputs, steps=4, graph=True):
    """h2: train_on_batch on one batch shape; with graph the step is captured on the third call and replayed on the fourth."""
    model.compile(LR)
    if graph:
        model.use_step_graph = True
    for _ in range(steps):
        model.train_on_batch(inputs)
    if graph:
        cs = [c for k, c in model._steps.items() if k[0] == "train"]
        assert model._graphs and len(cs) == 1 and cs[0].last == "replay", "the history did not capture and replay the step"
    assert model._plan is not None and model._plans


def step_observables(model, inputs, sample):
    """Loss terms and the gradient bucket of forward_backward on the fixed sample (RECURRENT_DROPOUT = 0: deterministic)."""
    losses = model.forward_backward(inputs, shuffle=None, targets=sample).clone()
    return dict(losses=losses, flat_grad=model.store.flat_grad.clone())


def adopt_training_state(fresh, aged, compile_fresh):
    """set_weights does not reset the optimizer (as in Keras), and the detection-target and dropout streams go on: the further step
    of the comparison starts from the aged model's optimizer state and stream positions, copied into the fresh one."""
    compile_fresh(fresh)
    fo, ao = fresh.optimizer, aged.optimizer
    assert type(fo) is type(ao)
    if ao._state is not None:
        fo._init(fresh.store)
        for a, b in zip(fo._state, ao._state):
            a.copy_(b)
        fo._gnorm.copy_(ao._gnorm)
    fo.iterations = ao.iterations
    for owner in ("", "caption_model"):
        f, a = (getattr(fresh, owner, None), getattr(aged, owner, None)) if owner else (fresh, aged)
        for attr in ("_dt_step", "_dt_val_step", "_drop_step"):
            if a is not None and attr in getattr(a, "__dict__", {}):
                setattr(f, attr, getattr(a, attr))


def stale_shadow(store):
    """The mirrored weights whose range of store.flat_bf16 is NOT torch's round-to-nearest-even cast of the master weights."""
    import torch
    assert store.wb, "no mirrored weight"
    return [n for n in store.wb if not torch.equal(store.wb[n], store.w[n].to(torch.bfloat16))]


# ------------------------------------------------------------------------------------------------------------------------------------
# the detection and tag models, the feature extractor, the decoders
# ------------------------------------------------------------------------------------------------------------------------------------
MASK_CLASSES, TAG_CLASSES = 9, 40


def detect_weights(variant=0):
    if ("detect", variant) not in _W:
        import _maskrcnn_ref as R
        from image_captioning_amd import synth
        Wt = backbone_weights(variant)
        Wt.update(synth.detect_head_weights(6 + 10 * variant, MASK_CLASSES))
        Wt['mrcnn_class_logits/kernel'] = Wt['mrcnn_class_logits/kernel'] * np.float32(10.0)
        Wt['mrcnn_bbox_fc/kernel'] = Wt['mrcnn_bbox_fc/kernel'] * np.float32(0.3)
        _W[("detect", variant)] = R.scale_mask_weights(Wt)
    return dict(_W[("detect", variant)])


def detect_model(W):
    from image_captioning_amd.mask_rcnn_model import MaskRCNN, MaskRCNNConfig

    class Cfg(MaskRCNNConfig):
        NAME = "maskrcnn"
        IMAGES_PER_GPU = 1
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
        POST_NMS_ROIS_INFERENCE = 60
        DETECTION_MAX_INSTANCES = 10
        DETECTION_MIN_CONFIDENCE = 0
    model = MaskRCNN("inference", Cfg(MASK_CLASSES), "logs", stage4_blocks=BLOCKS)
    model.set_weights(W)
    return model


def detect_observables(model, img):
    res = model.detect([img])[0]
    return dict(rois=res["rois"], class_ids=res["class_ids"], scores=res["scores"], masks=np.ascontiguousarray(res["masks"]),
                logits=model.last_heads[0].clone(), deltas=model.last_heads[1].clone(), class_masks=np.array(model.last_class_masks[0], np.float32))


def tag_weights(variant=0):
    if ("tag", variant) not in _W:
        from image_captioning_amd import synth
        Wt = backbone_weights(variant)
        Wt.update(synth.tag_head_weights(6 + 10 * variant, TAG_CLASSES))
        _W[("tag", variant)] = Wt
    return dict(_W[("tag", variant)])


def tag_model(W):
    from image_captioning_amd.roi_tag_model import ROITagRCNN
    from image_captioning_amd.train_roi_tags import RoiTagConfig

    class Cfg(RoiTagConfig):
        NAME = "roitag"
        IMAGES_PER_GPU = 1
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
        POST_NMS_ROIS_TRAINING = 60
        TRAIN_ROIS_PER_IMAGE = ROIS
    model = ROITagRCNN("training", Cfg(TAG_CLASSES), "logs", stage4_blocks=BLOCKS)
    model.set_weights(W)
    return model


def tag_inputs():
    """tests/test_gpu_roitag_model.tag_inputs: the joint batch with multi-hot tag rows at position 4."""
    inputs = train_inputs()
    gt = np.zeros((1, 6, TAG_CLASSES), np.int32)
    for g, cols in enumerate([[3], [0, 17, 39], [8, 21]]):
        gt[0, g, cols] = 1
    inputs[4] = gt
    return inputs


EXTRACTOR_SHAPES = ((1, 128, 128), (2, 64, 128))


def extractor_weights(variant=0):
    if ("extractor", variant) not in _W:
        from image_captioning_amd import synth
        _W[("extractor", variant)] = synth.encoder_weights(10 * variant, BLOCKS)
    return dict(_W[("extractor", variant)])


def extractor_model(W):
    from image_captioning_amd.config import Config
    from image_captioning_amd.modified_dense_model import DenseImageCapRCNN

    class Cfg(Config):
        NAME = "extractor"
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
    model = DenseImageCapRCNN("inference", Cfg(), "logs", use_generated_rois=False, stage4_blocks=BLOCKS)
    model.set_weights(W)
    return model


def extractor_observables(model):
    from image_captioning_amd import synth
    out = {}
    for b, h, w in EXTRACTOR_SHAPES:
        feats = model.extract_features(synth.images(5 + b, b, h, w), synth.rois(6 + b, b, ROIS, h, w, lo=8, hi=64))
        out["features_%dx%dx%d" % (b, h, w)] = feats.clone()
    return out


def decoder_features(seed, R):
    return np.random.default_rng(seed).standard_normal((R, 7, 7, 256)).astype(np.float32)


V2_T, V2_R = 5, 6


def v2_weights(variant=0):
    if ("v2", variant) not in _W:
        from image_captioning_amd import synth
        Wt = dict(synth.head_weights(1 + 10 * variant, 7, 256, 1024))
        Wt.update(synth.v2_weights(2 + 10 * variant, V, 300, 1024, 256, True, 1024))
        Wt['imgcap_embedding_layer/embeddings'] = synth.embedding_matrix(3 + 10 * variant, V)
        _W[("v2", variant)] = Wt
    return dict(_W[("v2", variant)])


def v2_model(W):
    from image_captioning_amd.text_generation_model_v2 import Adam, DenseCapConfig, build_model
    cfg = DenseCapConfig(V, W['imgcap_embedding_layer/embeddings'])
    cfg.PADDING_SIZE = V2_T
    model = build_model((7, 7, 256), (V2_T,), cfg, 256, True, seed=0)
    model.load_weights(W)
    model.compile(optimizer=Adam(amsgrad=True), loss="categorical_crossentropy")
    return model


def v2_batch():
    rng = np.random.default_rng(11)
    words = rng.integers(0, V, (V2_R, V2_T)).astype(np.int32)
    return decoder_features(12, V2_R), words, np.eye(V, dtype=np.float32)[rng.integers(1, V, V2_R)]


def v2_observables(model):
    feat, words, _ = v2_batch()
    ids, scores = model.generate(feat, decoder="incremental")
    toks, beam_scores = model.generate(feat, decoder="beam", beam_size=3)
    return dict(probs=model.predict([feat, words]), greedy_ids=ids, greedy_scores=scores, beam_ids=toks, beam_scores=beam_scores)


V1_V, V1_B = 24, 4


def v1_weights(variant=0):
    if ("v1", variant) not in _W:
        from image_captioning_amd import synth
        Wt = dict(synth.head_weights(1 + 10 * variant, 7, 256, 1024))
        Wt.update(synth.v1_weights(2 + 10 * variant, V1_V))
        # (as tests/_decode_cases.v1_model's scale: unscaled, the 24 words are near-uniform and logits that move by 1e-3 -- all the
        # recurrent kernels contribute beside the 1024 RoI features -- move no probability by 1e-3 of the largest)
        Wt['imgcap_lstm_d2/kernel'] = Wt['imgcap_lstm_d2/kernel'] * np.float32(8.0)
        Wt['imgcap_embedding_layer/embeddings'] = synth.embedding_matrix(3 + 10 * variant, V1_V)
        _W[("v1", variant)] = Wt
    return dict(_W[("v1", variant)])


def v1_model(W, dtype):
    from image_captioning_amd.text_generation_model import Adam, CaptionModelV1, DenseCapConfig
    cfg = DenseCapConfig(V1_V, W['imgcap_embedding_layer/embeddings'], V1_B)
    cfg.PADDING_SIZE = T
    model = CaptionModelV1([7, 7, 256], cfg, 512, 'training', seed=0, compute_dtype=dtype)
    model.recurrent_dropout = 0.0
    model.load_weights(W)
    # (lr: Adam's +-lr on each of conv1's 12 544 inputs per unit adds up; at Keras' 1e-3 four steps on these synthetic weights
    # drive word probabilities to exactly 0 and the beams' log scores to -inf, where nothing can be compared)
    model.compile(optimizer=Adam(lr=2e-5, amsgrad=True), loss="categorical_crossentropy")
    return model


def v1_batch():
    from image_captioning_amd import synth
    from image_captioning_amd.text_generation_model import caption_targets
    caps = synth.captions_v1(30, V1_B, T, V1_V, lmin=1, lmax=3)
    return decoder_features(31, V1_B), caps, caption_targets(caps, V1_V)


def v1_observables(model):
    feat, caps, _ = v1_batch()
    math = "bf16" if model.compute_dtype == "bf16" else None
    _, ids, scores = model.generate(feat, return_probabilities=False, decoder="incremental", vocab_math=math)
    # (score="prob", the sum of the word probabilities: a sum of five log p of magnitude 16 shows a change of the word probabilities
    # by half a percent as 1e-3 of itself, at the guard's own level)
    _, toks, beam_scores = model.generate(feat, return_probabilities=False, decoder="beam", beam_size=3, score="prob", vocab_math=math)
    return dict(probs=model.predict([feat, caps]), greedy_ids=ids, greedy_scores=scores, beam_ids=toks, beam_scores=beam_scores)


WI_SIZES = dict(input_dim=64, word_dim=32, language_units=32, merged_units=40)        # merged LSTM 40 held as 64: padded units
WI_CFG = dict(embedding_dim=32, vocabulary_size=52, max_caption_length=4, batch_size=37)


def whole_image_weights(variant=0):
    if ("wi", variant) not in _W:
        from image_captioning_amd import synth
        _W[("wi", variant)] = synth.whole_image_weights(10 * variant, 52, 32, 64, 32, 32, 40)
    return dict(_W[("wi", variant)])


def whole_image_model(W):
    from image_captioning_amd.whole_image.model import create_model
    model = create_model(WI_CFG, seed=0, **WI_SIZES)
    model.set_weights(W)
    return model


def whole_image_batch():
    rng = np.random.default_rng(21)
    return rng.standard_normal((37, 64)).astype(np.float32), rng.integers(0, 52, (37, 4)).astype(np.int32), rng.integers(0, 52, 37).astype(np.int32)


def whole_image_observables(model):
    feat, words, _ = whole_image_batch()
    toks, scores = model.generate(feat[:5], beam_size=3, start_id=1)
    return dict(probs=model.predict([feat, words]), beam_ids=toks, beam_scores=scores)


def padding_is_zero(model):
    import torch
    return [k for k in model.weight_names if not bool(torch.all(model.store.w[k][torch.tensor(model.padding_mask(k), device=model.device)] == 0))]
