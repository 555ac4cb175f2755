"""The RoI tag classifier behind the reference's module interface (roi_tag_classification/model.py: ROITagRCNN :1350, build :1365-1538,
classifier_graph :777-801, focal_loss :48-66, roi_tag_classes_loss_graph :877-887, compile :1603-1640, train :1720-1790,
refine_generations :631-669, generate_roi_tags).

The joint dense-captioning graph (dense_model.DenseImageCapRCNN) with the caption decoder replaced by a multi-label tag head:

  ResNet-101 -> FPN -> RPN -> ProposalLayer -> detection targets (a positive RoI carries its GT box's multi-hot tag row)
  -> PyramidROIAlign -> mrcnn_class_conv1/bn1/conv2/bn2 -> roitag_class_logits = Dense(NUM_CLASSES) -> sigmoid
  losses: focal loss summed over the RoIs with at least one tag (ops.tag_focal: sigmoid, loss and gradient in one launch), RPN class
  CE, RPN smooth-L1, L2(w)/size(w);  SGD(momentum, clipnorm=5.0) over the one flat bucket.

Everything below the top is DenseImageCapRCNN's step, unchanged: ROITagRCNN sub-classes it and puts TagTop where the caption model
sits (DenseImageCapRCNN._make_top).  The detection-target kernel gathers any int32 [n_gt, T] rows, so it runs as it is with
T = NUM_CLASSES; negatives and padding come out as all-zero rows, which the loss kernel treats as dead: no count, no row weights.
Inference shares the parent's pieces too: generate_roi_tags starts with its front (_proposal_features: mold, encoder pass, proposals,
RoIAlign) and packs postprocess='device' results with dense_model.pack_survivors; save_weights is the parent's (no layer groups).

Not in this class (each is refused with a ValueError that names it): compute_dtype="bf16", GPU_COUNT > 1 / ParallelModel,
pipeline.JointTrainPipeline (train() runs the serial loop) and captured step graphs -- every step is issued eagerly and
DCAP_STEP_GRAPH does not apply."""
import numpy as np
import torch

from . import dense_model, ops, synth, utils
from .dense_model import DenseImageCapRCNN
from .params import SGD
from .text_generation_model import RoiHead

def load_rois_and_tags(dataset, image_id):
    """data_generator's loader for tag datasets: (boxes [G,4], multi-hot tag rows int32 [G,NUM_CLASSES])."""
    boxes, tags = dataset.load_rois_and_tags(image_id)
    return np.asarray(boxes), np.asarray(tags).astype(np.int32).reshape(len(boxes), -1)


def data_generator(dataset, config, **kw):
    """dense_model.data_generator with the tag loader: the reference's six training inputs, position 4 = gt_classes
    [B, MAX_GT_INSTANCES, NUM_CLASSES] int32 (model.py:1221-1330)."""
    return dense_model.data_generator(dataset, config, loader=load_rois_and_tags, **kw)


def refine_tag_generations(rois, scores, window, config):
    """GenerationMatchLayer's refine_generations for one image (model.py:631-669): rois [N,4] normalised, scores [N] the RoIs'
    classes_scores (:644-646: the sum of log p over the classes with p > DETECTION_MIN_CONFIDENCE, or -3.4e38 -- computed on the
    device, ops.tag_scores); boxes to pixels of the molded image, clipped to the window;
    NMS(DETECTION_NMS_THRESHOLD) by score on the clipped boxes; the best DETECTION_MAX_INSTANCES survive, rounded.  Equal scores --
    every RoI without a confident class shares -3.4e38 -- are taken in the order np.argsort(kind='stable')[::-1] gives, which is also
    the device path's (ops.refine_generations); NumPy's default sort promises none.  Returns (int32 boxes [K,4], kept indices [K]);
    the survivors' tags are the kept rows of the probabilities."""
    s = np.asarray(scores, np.float64)
    rank = np.empty(len(s), np.float64)
    rank[np.argsort(s, kind="stable")] = np.arange(len(s))           # distinct stand-ins in the scores' stable order
    return dense_model.refine_generations(rois, None, window, config, caption_scores=rank)


class TagTop(RoiHead):
    """The trainable top on the pooled RoI features: the shared RoI head, roitag_class_logits and the focal loss.  Owns the flat
    parameter bucket like CaptionModelV1 does in the caption model (extra_params: the FPN / RPN / trainable ResNet weights)."""
    compute_dtype = "f32"
    recurrent_dropout = 0.0              # (what the joint step asks of its top: this one has no dropout and no per-step stream)
    dropout_rows = "roi"
    _drop_step = 0

    def __init__(self, features_input, num_classes, device, seed=0, extra_params=(), alpha=0.25, gamma=2.0):
        self.C = int(num_classes)
        if self.C < 4 or self.C % 4:
            raise ValueError("NUM_CLASSES must be a positive multiple of 4 (16-byte rows of roitag_class_logits/kernel), got %r: pad the "
                             "tag list with unused classes" % (num_classes,))
        self.alpha, self.gamma = float(alpha), float(gamma)
        self.device = torch.device(device)
        pool, cin = features_input[0], features_input[2]
        W = dict(synth.head_weights(seed + 1, pool, cin, self.FEAT))
        W.update(synth.tag_head_weights(seed + 6, self.C, self.FEAT))
        self.store = self._build_store(W, lambda k: 'moving_' in k, extra_params)
        self._init_runtime()

    def _prefix_rows(self, training):
        return False

    def logits(self, feat):
        """feat [R,7,7,256] (or [R,12544]) -> roitag_class_logits' output [R,C], the bias added by the GEMM's epilogue."""
        w = self.store.w
        R = feat.shape[0]
        f = self._head_forward(feat.reshape(R, -1))
        return f, ops.gemm(f.f, w['roitag_class_logits/kernel'], shift=w['roitag_class_logits/bias'], out=self._buf('logits', (R, self.C)))

    def _forward_train(self, feat, classes, want_grad=False):
        """feat [R,7,7,256], classes int32 [R,C] on the device (multi-hot; all-zero rows are dead) -> (loss_rows [R], None): each live
        row's summed focal loss; with want_grad d(sum of loss_rows)/d(logits) is kept for _backward."""
        R = feat.shape[0]
        f, z = self.logits(feat)
        loss_rows = self._buf('loss_rows', (R,))
        dz = self._buf('dlogits', (R, self.C)) if want_grad else None
        ops.tag_focal(z, classes, self.alpha, self.gamma, 1.0, loss_rows=loss_rows, dlogits=dz)
        self._ctx = (f, dz)
        return loss_rows, None

    def _backward(self, want_dx=False, ready=None):
        ready = (lambda *layers: None) if ready is None else ready
        w, g = self.store.w, self.store.grad
        f, dz = self._ctx
        ops.gemm(f.f, dz, a_trans=True, out=g['roitag_class_logits/kernel'])
        ops.colsum(dz, out=g['roitag_class_logits/bias'])
        ready('roitag_class_logits')
        df = ops.gemm(dz, w['roitag_class_logits/kernel'], b_trans=True, out=self._buf('df', (dz.shape[0], self.FEAT)))
        return self._head_backward(df, dz.shape[0], ready, want_dx)


class ROITagRCNN(DenseImageCapRCNN):
    LOSS_NAMES = ("rpn_class_loss", "rpn_bbox_loss", "roi_tag_classes_loss")
    LAYER_REGEX = {                       # roi_tag_classification/model.py:1740-1750
        "no_backbone": r"(roitag\_.*)|(rpn\_.*)|(fpn\_.*)|(mrcnn\_.*)",
        "no_rpn": r"(res.*)|(bn3.*)|(roitag\_.*)|(fpn\_.*)|(mrcnn\_.*)",
        "3+": r"(res3.*)|(bn3.*)|(res4.*)|(bn4.*)|(res5.*)|(bn5.*)|(roitag\_.*)|(rpn\_.*)|(fpn\_.*)|(mrcnn\_.*)",
        "4+": r"(res4.*)|(bn4.*)|(res5.*)|(bn5.*)|(roitag\_.*)|(rpn\_.*)|(fpn\_.*)|(mrcnn\_.*)",
        "5+": r"(res5.*)|(bn5.*)|(roitag\_.*)|(rpn\_.*)|(fpn\_.*)|(mrcnn\_.*)",
        "all": ".*",
    }
    SAVE_LAYER_GROUPS = SAVE_GROUP_MEMBER_ORDER = None       # every layer of this model is a top-level Keras layer
    GT_LOADER = staticmethod(load_rois_and_tags)
    PIPELINED_FIT = False
    FOCAL_ALPHA, FOCAL_GAMMA = 0.25, 2.0  # focal_loss' defaults (model.py:48)

    def __init__(self, mode, config, model_dir, device=None, stage4_blocks=22, seed=0, conv_math=None, compute_dtype="f32", backbone_from=None):
        if compute_dtype != "f32":
            raise ValueError("ROITagRCNN: compute_dtype=%r is not available for the tag head (compute_dtype=\"bf16\" is out of scope): use 'f32'"
                             % (compute_dtype,))
        if int(config.GPU_COUNT) > 1:
            raise ValueError("ROITagRCNN: GPU_COUNT = %d: data-parallel training (GPU_COUNT > 1 / ParallelModel) is not available for this class"
                             % config.GPU_COUNT)
        DenseImageCapRCNN.__init__(self, mode, config, model_dir, device=device, stage4_blocks=stage4_blocks, seed=seed, conv_math=conv_math,
                                   compute_dtype="f32", backbone_from=backbone_from)
        self._path.pin(False)             # every step eagerly: this class captures no step graph, DCAP_STEP_GRAPH does not apply

    def _make_top(self, cfg, dev, seed, extra):
        return TagTop([cfg.POOL_SIZE, cfg.POOL_SIZE, 256], cfg.NUM_CLASSES, dev, seed, extra_params=extra, alpha=self.FOCAL_ALPHA,
                      gamma=self.FOCAL_GAMMA)

    # ---- what this class refuses -------------------------------------------------------------
    NO_STEP_GRAPH = "captured step graphs are not available for this class (its steps are issued eagerly)"
    use_step_graph, grad_sync = dense_model.REFUSED_STEP_GRAPH, dense_model.REFUSED_GRAD_SYNC

    def plan_pair(self):
        raise ValueError("ROITagRCNN: pipeline.JointTrainPipeline is not available for this class: train() runs the serial loop")

    def generate_captions(self, *args, **kw):
        raise ValueError("ROITagRCNN has no caption decoder: use generate_roi_tags")

    # ---- the top's forward on a sample --------------------------------------------------------
    def _top_forward_device(self, feats, caps_d, R_all, T, backward, rpn_up):
        return self.caption_model._forward_train(feats, caps_d.view(R_all, T), want_grad=backward)[0]

    def _top_forward_host(self, feats, caps, want_grad):
        classes = torch.tensor(np.ascontiguousarray(caps, np.int32), device=self.device)
        return self.caption_model._forward_train(feats, classes, want_grad=want_grad)[0]

    @staticmethod
    def _given_positive_rows(caps):
        return int((np.asarray(caps) == 1).any(axis=1).sum())

    # ---- compile / train ----------------------------------------------------------------------
    def compile(self, learning_rate, momentum=None, optimizer=None):
        """SGD(lr=learning_rate, momentum, clipnorm=5.0) (model.py:1603-1609; momentum None: config.LEARNING_MOMENTUM), or `optimizer` as
        DenseImageCapRCNN.compile takes it; the losses are the three graph losses + L2(WEIGHT_DECAY)(w)/size(w) (:1610-1628)."""
        if optimizer is None:
            optimizer = SGD(lr=learning_rate, momentum=self.config.LEARNING_MOMENTUM if momentum is None else momentum, clipnorm=5.0)
        DenseImageCapRCNN.compile(self, learning_rate, optimizer)

    def train(self, train_dataset, val_dataset, learning_rate, epochs, layers, rpn_targets="host", mold="host", prefetch=0, optimizer=None):
        """model.py:1720-1790: the generators, set_trainable(layers), compile(learning_rate, config.LEARNING_MOMENTUM), a checkpoint per
        epoch; the keywords are DenseImageCapRCNN.train's.  layers="no_rpn" trains every ResNet convolution but only the bn3* BatchNorms:
        the trainable backbone here is a set of whole stages (backbone_from), which cannot express that, so it is refused."""
        if layers == "no_rpn" or layers == self.LAYER_REGEX["no_rpn"]:
            raise ValueError("ROITagRCNN.train: layers=\"no_rpn\" (every res* convolution trainable, of the BatchNorm layers only bn3*) cannot be "
                             "expressed by the stage-wise trainable backbone (backbone_from); use \"no_backbone\", \"3+\", \"4+\", \"5+\" or \"all\"")
        return DenseImageCapRCNN.train(self, train_dataset, val_dataset, learning_rate, epochs, layers, rpn_targets=rpn_targets, mold=mold,
                                       prefetch=prefetch, optimizer=optimizer)

    # ---- inference ------------------------------------------------------------------------------
    def generate_roi_tags(self, images, verbose=0, postprocess="host", mold="host"):
        """The inference graph (model.py:1519-1531) + generate_roi_tags: RPN proposals (POST_NMS_ROIS_INFERENCE) -> RoI features -> head
        -> sigmoid and classes_scores in one launch (ops.tag_scores) -> GenerationMatchLayer -> boxes in the original image.
        Returns [{'rois': int32 [K,4], 'tags': float32 [K,NUM_CLASSES] class probabilities}], K <= DETECTION_MAX_INSTANCES.
        postprocess='host': refine_tag_generations and unmold_generations in NumPy, image by image, on the device's float32 scores.
        'device': ONE ops.refine_generations for the batch on those same scores, a device gather of the survivors' probability rows and
        ONE device-to-host copy; the same results bit for bit.  mold: as DenseImageCapRCNN.generate_captions."""
        if postprocess not in ("host", "device"):
            raise ValueError("postprocess must be 'host' or 'device', got %r" % (postprocess,))
        utils.check_mold(mold, self.config.IMAGE_PADDING)
        _, images, windows, consts, proposals, feats = self._proposal_features(images, mold, want_consts=postprocess == "device")
        cfg, B = self.config, len(images)
        K, C, M = proposals.shape[1], self.caption_model.C, int(cfg.DETECTION_MAX_INSTANCES)
        _, z = self.caption_model.logits(feats.view(B * K, cfg.POOL_SIZE, cfg.POOL_SIZE, 256))
        probs, scores = ops.tag_scores(z, cfg.DETECTION_MIN_CONFIDENCE, probs=self._buf("tag_probs", (B * K, C)), scores=self._buf("tag_scores", (B * K,)))
        self.last_tags = (probs, scores)
        if postprocess == "device":
            boxes, keep, count, _ = ops.refine_generations(proposals, consts, cfg.DETECTION_NMS_THRESHOLD, M, caption_scores=scores)
            n, rois, (tags,) = dense_model.pack_survivors(count, boxes, keep, K, [probs])
            tags = tags.view(np.float32)
            return [{"rois": rois[b, :n[b]].copy(), "tags": tags[b, :n[b]].copy()} for b in range(B)]
        props_h, probs_h, scores_h = proposals.cpu().numpy(), probs.cpu().numpy().reshape(B, K, C), scores.cpu().numpy().reshape(B, K)
        results = []
        for b in range(B):
            boxes, keep = refine_tag_generations(props_h[b], scores_h[b], windows[b], cfg)
            final, ok = dense_model.unmold_generations(boxes, images[b].shape, windows[b])
            results.append({"rois": final[ok], "tags": probs_h[b][keep[ok]]})
        return results
