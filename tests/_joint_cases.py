"""What the joint-model test files (test_gpu_models.py, test_gpu_joint_launch_sequence.py, the data-parallel workers) share: the factory
of the small joint model on synthetic weights and one batch of its six training inputs.  A plain module, no fixtures; the package is
imported inside the functions, as in the test files."""
import numpy as np


def joint_config(S=128, V=24, T=5, rois=12):
    """The small joint model's config (no device needed)."""
    from image_captioning_amd.config import Config

    class Cfg(Config):
        NAME = "joint"
        IMAGES_PER_GPU = 1
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
        POST_NMS_ROIS_TRAINING = 60
        TRAIN_ROIS_PER_IMAGE = rois
        PADDING_SIZE = T
        VOCABULARY_SIZE = V
        EMBEDDING_SIZE = 300
        RECURRENT_DROPOUT = 0.0          # parity against the deterministic oracle graph (the training default is the reference's 0.2)
    return Cfg()


def joint_weights(V=24, blocks=1):
    """The small joint model's synthetic weights (no device needed)."""
    from image_captioning_amd import synth
    Wt = dict(synth.encoder_weights(0, blocks), **synth.rpn_weights(4))
    Wt['rpn_conv_shared/kernel'] = Wt['rpn_conv_shared/kernel'] * np.float32(0.05)
    Wt['rpn_bbox_pred/kernel'] = Wt['rpn_bbox_pred/kernel'] * np.float32(0.3)
    Wt.update(synth.head_weights(1))
    Wt['mrcnn_class_conv1/kernel'] = Wt['mrcnn_class_conv1/kernel'] * np.float32(0.05)   # random FPN maps are O(10): keep the
    Wt.update(synth.v1_weights(2, V))                                                    # vocabulary softmax out of saturation
    Wt['imgcap_embedding_layer/embeddings'] = synth.embedding_matrix(3, V)
    return Wt


def oracle_cfg(cfg, mean_pixel=(123.7, 116.8, 103.9)):
    """The config values oracle.np_models.joint_loss_and_grads reads."""
    return dict(mean_pixel=list(mean_pixel), scales=cfg.RPN_ANCHOR_SCALES, ratios=cfg.RPN_ANCHOR_RATIOS, strides=cfg.BACKBONE_STRIDES,
                proposal_count=cfg.POST_NMS_ROIS_TRAINING, nms=cfg.RPN_NMS_THRESHOLD, train_rois=cfg.TRAIN_ROIS_PER_IMAGE,
                positive_ratio=cfg.ROI_POSITIVE_RATIO, weight_decay=cfg.WEIGHT_DECAY, T=cfg.PADDING_SIZE)


def make_joint(S=128, V=24, T=5, blocks=1, rois=12, compute_dtype="f32", conv_math=None):
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    cfg, Wt = joint_config(S, V, T, rois), joint_weights(V, blocks)
    cfg.EMBEDDING_WEIGHTS = Wt['imgcap_embedding_layer/embeddings']
    model = DenseImageCapRCNN("training", cfg, "logs", stage4_blocks=blocks, compute_dtype=compute_dtype, conv_math=conv_math)
    model.set_weights(Wt)
    return model, cfg, Wt


def joint_inputs(S, V, T, seed=8):
    from image_captioning_amd import synth
    rng = np.random.default_rng(seed)
    img = synth.images(7, 1, S, S)
    gt_boxes = np.zeros((1, 6, 4), np.float32)
    gt_boxes[0, :3] = np.array([[10, 12, 70, 90], [40, 30, 120, 128], [0, 0, 50, 40]], np.float32) * (S / 128.0)
    gt_caps = np.zeros((1, 6, T), np.int32)
    gt_caps[0, :3] = synth.captions_v1(9, 3, T, V, lmin=1, lmax=3)
    n_anchor = sum((S // s) ** 2 for s in (4, 8, 16, 32, 64)) * 3
    match = np.zeros((1, n_anchor, 1), np.int32)
    match[0, rng.choice(n_anchor, 40, replace=False), 0] = np.where(rng.random(40) < 0.4, 1, -1)
    tdelta = rng.standard_normal((1, 64, 4))
    return [img, np.zeros((1, 12)), match, tdelta, gt_caps, gt_boxes]
