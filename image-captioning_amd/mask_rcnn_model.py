"""Mask R-CNN at inference behind the reference's module interface (mask_rcnn/mask_rcnn_model.py: MaskRCNN :1760, the inference branch of
build :1915-1942, fpn_classifier_graph :854-905, build_fpn_mask_graph :908-956, refine_detections :669-738, DetectionLayer :741-779,
unmold_detections :2253-2312, detect :2314-2354; mask_rcnn/utils.py: apply_box_deltas, non_max_suppression, unmold_mask).

  ResNet-101 -> FPN -> RPN -> ProposalLayer (POST_NMS_ROIS_INFERENCE)
  -> PyramidROIAlign(7) -> mrcnn_class_conv1/bn1/conv2/bn2 -> mrcnn_class_logits, mrcnn_bbox_fc (two GEMMs, bias in the epilogue)
  -> ops.class_select: per RoI the winning class, its softmax probability and its four deltas -- 6 words per RoI to the host
  -> refine_detections + the box part of unmold_detections on the host in NumPy (the reference runs the former in a py_func)
  -> ONE packed upload: the detection boxes normalised, their class ids, their boxes in the original image
  -> PyramidROIAlign(MASK_POOL_SIZE) -> mrcnn_mask_conv1..4 + frozen BN + ReLU (four dc_conv2d_nhwc_f32 launches)
  -> ops.mask_head_tail: mrcnn_mask_deconv + ReLU + mrcnn_mask + sigmoid for each detection's OWN class: [M,28,28]
  -> utils.unmold_mask: postprocess="host" in NumPy / PIL, "device" ops.mask_paste and one copy of the [M,H,W] bytes.
detect(refine="device") replaces the three middle steps by ops.refine_detections on the device (one launch, no host read before the
results come down) and runs the mask head on DETECTION_MAX_INSTANCES rows per image.
detect(mask_format="rle") returns the masks as COCO run-length encodings (mask_rle.py); with postprocess="device" ops.mask_rle builds
them from the [M,28,28] masks and the boxes in place of ops.mask_paste, and the [M,H,W] bytes never exist.
evaluate() scores detect()'s results against annotated images -- utils.compute_ap's rule (detection_eval.py) on mask IoU of the
run-length encodings or on box IoU --; backend="device" keeps the encodings on the device (ops.rle_iou / ops.box_iou, ops.detection_ap).

Everything below the heads is DenseImageCapRCNN's, unchanged: MaskRCNN sub-classes it and puts DetectTop where the caption model sits.
detect() starts with the parent's inference front (_proposal_features: mold, encoder pass, proposals, RoIAlign(7)); save_weights is the
parent's (no layer groups), and the use_step_graph / grad_sync refusals are dense_model's shared properties.

Not in this class (each is refused with a ValueError that names it): mode="training" and the parent's training surface -- train, compile,
train_on_batch(_device), test_on_batch(_device), forward_backward, set_trainable, plan_pair, use_step_graph, grad_sync -- (the detection
targets and the class, box and mask losses are not built), compute_dtype="bf16", GPU_COUNT > 1 and generate_captions."""
import numpy as np
import torch

from . import dense_model, mask_rle, ops, synth, utils
from .config import Config
from .dense_model import DenseImageCapRCNN
from .packing import pack_conv_kernel, pack_mask_tail
from .text_generation_model import RoiHead

MASK_CONVS = tuple(("mrcnn_mask_conv%d" % i, "mrcnn_mask_bn%d" % i) for i in (1, 2, 3, 4))
MASK_CHANNELS = 256


class MaskRCNNConfig(Config):
    """mask_rcnn/config.py's fields that config.Config (the captioning models' copy) does not carry."""
    NAME = "mask_rcnn"
    NUM_CLASSES = 1                       # background + the dataset's classes (COCO: 81); the reference's default
    USE_MINI_MASK = True                  # training-side fields, kept for scripts that set them
    MINI_MASK_SHAPE = (56, 56)

    def __init__(self, num_classes=None):
        super(MaskRCNNConfig, self).__init__()
        if num_classes is not None:
            self.NUM_CLASSES = int(num_classes)


# ------------------------------------------------------------------------------------------------ the host side, restated
def apply_box_deltas(boxes, deltas):
    """utils.apply_box_deltas with the reference's number formats: float32 boxes, sizes and centres; the deltas arrive as float64
    (refine_detections multiplies them by the float64 BBOX_STD_DEV) and enter through IN-PLACE updates, i.e. each update is computed in
    float64 and rounded to float32 once; np.exp is NumPy's, on the host, as in the reference."""
    boxes = boxes.astype(np.float32)
    height = boxes[:, 2] - boxes[:, 0]
    width = boxes[:, 3] - boxes[:, 1]
    center_y = boxes[:, 0] + 0.5 * height
    center_x = boxes[:, 1] + 0.5 * width
    center_y += deltas[:, 0] * height
    center_x += deltas[:, 1] * width
    height *= np.exp(deltas[:, 2])
    width *= np.exp(deltas[:, 3])
    y1 = center_y - 0.5 * height
    x1 = center_x - 0.5 * width
    return np.stack([y1, x1, y1 + height, x1 + width], axis=1)


def clip_to_window(window, boxes):
    """In place, in the boxes' own dtype: the window is the float32 row of image_meta the DetectionLayer reads."""
    window = np.asarray(window, boxes.dtype)
    for col, lo, hi in ((0, 0, 2), (1, 1, 3), (2, 0, 2), (3, 1, 3)):
        boxes[:, col] = np.maximum(np.minimum(boxes[:, col], window[hi]), window[lo])
    return boxes


def refine_detections(rois, class_ids, class_scores, deltas_specific, window, config):
    """refine_detections (:689-738) for one image from line :689 on: what comes before it -- the argmax, the winner's probability and
    the winner's deltas (:684-688) -- is ops.class_select's output.  rois float32 [N,4] normalised, class_ids int [N], class_scores
    float32 [N], deltas_specific float32 [N,4], window (y1, x1, y2, x2) of the molded image.
    Returns (boxes int32 [K,4] in the molded image, class_ids int32 [K], scores float32 [K], the kept RoIs' indices [K]), best first."""
    class_ids = np.asarray(class_ids).astype(np.int64)
    class_scores = np.asarray(class_scores, np.float32)
    refined = apply_box_deltas(np.asarray(rois, np.float32), np.asarray(deltas_specific, np.float32) * config.BBOX_STD_DEV)
    height, width = config.IMAGE_SHAPE[:2]
    refined *= np.array([height, width, height, width])
    refined = clip_to_window(window, refined)
    refined = np.rint(refined).astype(np.int32)
    keep = np.where(class_ids > 0)[0]
    if config.DETECTION_MIN_CONFIDENCE:
        keep = np.intersect1d(keep, np.where(class_scores >= config.DETECTION_MIN_CONFIDENCE)[0])
    pre_ids, pre_scores, pre_rois = class_ids[keep], class_scores[keep], refined[keep]
    nms_keep = []
    for class_id in np.unique(pre_ids):
        ixs = np.where(pre_ids == class_id)[0]
        class_keep = utils.non_max_suppression(pre_rois[ixs], pre_scores[ixs], config.DETECTION_NMS_THRESHOLD)
        nms_keep = np.union1d(nms_keep, keep[ixs[class_keep]])
    keep = np.intersect1d(keep, nms_keep).astype(np.int32)
    top = np.argsort(class_scores[keep])[::-1][:config.DETECTION_MAX_INSTANCES]
    keep = keep[top]
    return refined[keep], class_ids[keep].astype(np.int32), class_scores[keep], keep


def unmold_boxes(boxes, image_shape, window):
    """The box part of unmold_detections (:2281-2301): shift by the window, scale to the original image in float64, truncate to int32.
    Returns (boxes int32 [K,4], mask of the boxes with a positive area: the others are deleted there)."""
    return dense_model.unmold_generations(boxes, image_shape, window)


def detection_constants(window, config, image_shape):
    """One image's row of ops.refine_detections' image_consts (float64 [_lib.REFINE_CONSTS]).  dense_model.refine_constants' row fits as
    it is: the window (the kernel reads it as the float32 values the DetectionLayer sees, np.asarray(window, np.float32)) and
    unmold_boxes' shift (y, x) and scale, computed as that function computes them; IMAGE_SHAPE's h and w sit in the row too, but
    ops.refine_detections takes them as image_hw."""
    return dense_model.refine_constants(window, config, image_shape)


def pack_detections(count, boxes, rois, class_ids, scores, keep):
    """ops.refine_detections' outputs (all but the normalised boxes) as ONE int32 buffer and ONE device-to-host copy, in the manner of
    dense_model.pack_survivors.  Returns on the host (n [B], boxes [B,M,4], rois [B,M,4], class_ids [B,M], scores float32 [B,M],
    keep [B,M]): image b's first n[b] rows count."""
    B, M = keep.shape
    packed = torch.cat([count, boxes.reshape(-1), rois.reshape(-1), class_ids.reshape(-1), scores.view(torch.int32).reshape(-1), keep.reshape(-1)])
    host = packed.cpu().numpy()                          # the one small device-to-host copy
    cuts = np.cumsum([0, B, B * M * 4, B * M * 4, B * M, B * M, B * M])
    n, bx, ro, ci, sc, kp = (host[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:]))
    return n, bx.reshape(B, M, 4), ro.reshape(B, M, 4), ci.reshape(B, M), sc.view(np.float32).reshape(B, M), kp.reshape(B, M)


def bytescale(mask):
    """scipy 1.0's misc.bytescale(mask) as imresize calls it (cmin / cmax the mask's own, low 0, high 255), with NumPy 1.x's arithmetic on
    a float32 array: the scale is 255.0 / range in float64, then cast to the array's float32 by the multiplication."""
    m = np.asarray(mask, np.float32)
    cmin, cmax = m.min(), m.max()
    rng = np.float32(cmax - cmin)
    if rng == 0:
        rng = np.float32(1.0)
    scale = np.float32(255.0 / float(rng))
    out = np.clip((m - cmin) * scale, np.float32(0.0), np.float32(255.0)) + np.float32(0.5)
    return out.astype(np.uint8)


def resize_mask(mask, bh, bw):
    """imresize(mask, (bh, bw), interp='bilinear') >= 128: uint8 [bh,bw] of 0 / 1 (byte / 255 >= 0.5 exactly when byte >= 128)."""
    from PIL import Image
    small = Image.fromarray(bytescale(mask), mode="L").resize((int(bw), int(bh)), resample=Image.BILINEAR)
    return (np.asarray(small) >= 128).astype(np.uint8)


def unmold_mask(mask, bbox, image_shape):
    """utils.unmold_mask: the [h,w] float mask of one detection -> uint8 [H,W] of the original image, 1 inside the box where the
    resized mask reaches 0.5.  A box without area or one that leaves the image gives zeros (the reference deletes the former before it
    gets here and cannot produce the latter)."""
    y1, x1, y2, x2 = (int(v) for v in bbox)
    full = np.zeros(tuple(image_shape[:2]), np.uint8)
    if 0 <= y1 < y2 <= full.shape[0] and 0 <= x1 < x2 <= full.shape[1]:
        full[y1:y2, x1:x2] = resize_mask(mask, y2 - y1, x2 - x1)
    return full


# ------------------------------------------------------------------------------------------------ the heads
class DetectTop(RoiHead):
    """What sits on the pooled RoI features: the shared head, the class / box GEMMs and the mask head's weights.  Owns the parameter
    store like TagTop; the detection layers are frozen entries (this class only runs inference).  Stored shapes: mrcnn_class_logits
    padded to a multiple of 4 columns (16-byte rows for the GEMM), the mask convolutions packed like every 3x3 kernel here,
    mrcnn_mask transposed to [C][256] (packing.pack_mask_tail); get_keras_weights / set_keras_weights speak Keras' shapes."""
    compute_dtype = "f32"

    def __init__(self, features_input, num_classes, device, seed=0, extra_params=(), mask_pool=14):
        self.C = int(num_classes)
        if self.C < 2:
            raise ValueError("NUM_CLASSES must be at least 2 (background and one class), got %r" % (num_classes,))
        self.Cp = (self.C + 3) // 4 * 4
        self.mask_pool = int(mask_pool)
        self.device = torch.device(device)
        pool, cin = features_input[0], features_input[2]
        # the detection layers: frozen entries in front of extra_params, in synth.detect_head_weights' order
        detect = [(k, v, False) for k, v in self.to_stored(synth.detect_head_weights(seed + 6, self.C, self.FEAT)).items()]
        self.store = self._build_store(synth.head_weights(seed + 1, pool, cin, self.FEAT), lambda k: 'moving_' in k, detect + list(extra_params))
        self._bufs = {}
        self._folded = None

    def to_stored(self, W):
        """Keras-shaped detection-head weights -> the shapes the store holds (any subset)."""
        out = {}
        for k, v in W.items():
            layer, wname = k.split("/")
            v = np.asarray(v, np.float32)
            if layer == "mrcnn_class_logits":
                want = (self.FEAT, self.C) if wname == "kernel" else (self.C,)
                if tuple(v.shape) != want:
                    raise ValueError("shape mismatch for %s: %s vs %s" % (k, v.shape, want))
                pad = np.zeros(want[:-1] + (self.Cp,), np.float32)
                pad[..., :self.C] = v
                v = pad
            elif layer.startswith("mrcnn_mask_conv") and wname == "kernel":
                v = pack_conv_kernel(v)
            elif layer == "mrcnn_mask" and wname == "kernel":
                v = pack_mask_tail(v)
            out[k] = v
        return out

    def from_stored(self, k, v):
        layer, wname = k.split("/")
        if layer == "mrcnn_class_logits":
            return np.ascontiguousarray(v[..., :self.C])
        if layer.startswith("mrcnn_mask_conv") and wname == "kernel":
            return np.ascontiguousarray(v.reshape(v.shape[0], 3, 3, -1).transpose(1, 2, 3, 0))
        if layer == "mrcnn_mask" and wname == "kernel":
            return np.ascontiguousarray(v.T)[None, None]
        return v

    def heads(self, feat):
        """feat [R,7,7,256] -> (logits [R,C] (a view of the padded [R,Cp] buffer), box deltas [R,4C])."""
        w = self.store.w
        R = feat.shape[0]
        f = self._head_forward(feat.reshape(R, -1))
        z = ops.gemm(f.f, w['mrcnn_class_logits/kernel'], shift=w['mrcnn_class_logits/bias'], out=self._buf('logits', (R, self.Cp)))
        d = ops.gemm(f.f, w['mrcnn_bbox_fc/kernel'], shift=w['mrcnn_bbox_fc/bias'], out=self._buf('bbox', (R, 4 * self.C)))
        return z[:, :self.C], d

    def folded(self):
        """The four mask convolutions' epilogue operands: frozen BN statistics and the convolution's bias folded on the device
        (dc_bn_fold_f32), once per set of weights."""
        if self._folded is None:
            w = self.store.w
            self._folded = []
            for conv, bn in MASK_CONVS:
                scale, shift = (torch.empty(MASK_CHANNELS, dtype=torch.float32, device=self.device) for _ in range(2))
                ops.bn_fold(w[bn + '/gamma'], w[bn + '/beta'], w[conv + '/bias'], w[bn + '/moving_mean'], w[bn + '/moving_variance'], scale, shift)
                self._folded.append((scale, shift))
        return self._folded

    def _weights_changed(self):
        """Weights rewritten (the model's set_weights, load_weights on this top, a broadcast): the folded operands are of the old ones."""
        self._folded = None
        RoiHead._weights_changed(self)

    def mask_layer(self, i, x, out=None):
        """mrcnn_mask_conv<i+1> + mrcnn_mask_bn<i+1> (frozen) + ReLU on x [M,P,P,256], one dc_conv2d_nhwc_f32 launch."""
        conv = MASK_CONVS[i][0]
        scale, shift = self.folded()[i]
        P = x.shape[1]
        return ops.conv2d(x, self.store.w[conv + '/kernel'], 3, 3, 1, 1, 1, P, P, scale=scale, shift=shift, relu=True, out=out)

    def mask_trunk(self, x):
        """x [M,P,P,256] -> the fourth convolution's output (conv + frozen BN + ReLU, four times, two buffers in turn)."""
        for i in range(len(MASK_CONVS)):
            x = self.mask_layer(i, x, out=self._buf('mask_act%d' % (i & 1), tuple(x.shape[:3]) + (MASK_CHANNELS,)))
        return x

    def class_masks(self, x, class_ids, out=None):
        """x [M,P,P,256] (RoIAlign at MASK_POOL_SIZE), class_ids int32 [M] on the device -> [M,2P,2P]: each detection's own class mask."""
        w = self.store.w
        return ops.mask_head_tail(self.mask_trunk(x), w['mrcnn_mask_deconv/kernel'], w['mrcnn_mask_deconv/bias'], w['mrcnn_mask/kernel'],
                                  w['mrcnn_mask/bias'], class_ids, out=out)


def _no_training(name):
    """A method of the parent's training surface as this inference-only class has it: refused by name."""
    def refuse(self, *args, **kw):
        raise ValueError("MaskRCNN.%s: training is not built (mode=\"training\": detection targets and the class, box and mask losses)" % name)
    refuse.__name__ = name
    return refuse


class MaskRCNN(DenseImageCapRCNN):
    LOSS_NAMES = ()
    # every layer of this model is a top-level Keras layer (TimeDistributed wrappers carry their inner layer's name)
    SAVE_LAYER_GROUPS = SAVE_GROUP_MEMBER_ORDER = None

    def __init__(self, mode, config, model_dir, device=None, stage4_blocks=22, seed=0, conv_math=None, compute_dtype="f32"):
        if mode != "inference":
            raise ValueError("MaskRCNN: mode=%r: only mode=\"inference\" is built (mode=\"training\" needs the class-id, box-delta and mask "
                             "detection targets and the class, box and mask losses)" % (mode,))
        if compute_dtype != "f32":
            raise ValueError("MaskRCNN: compute_dtype=%r is not available for the detection heads (compute_dtype=\"bf16\" is out of scope): "
                             "use 'f32'" % (compute_dtype,))
        if int(config.GPU_COUNT) > 1:
            raise ValueError("MaskRCNN: GPU_COUNT = %d: data-parallel runs (GPU_COUNT > 1 / ParallelModel) are not available for this class"
                             % config.GPU_COUNT)
        if int(getattr(config, "NUM_CLASSES", 0)) < 2:
            raise ValueError("MaskRCNN: NUM_CLASSES must be at least 2 (background and one class), got %r" % (getattr(config, "NUM_CLASSES", None),))
        DenseImageCapRCNN.__init__(self, mode, config, model_dir, device=device, stage4_blocks=stage4_blocks, seed=seed, conv_math=conv_math,
                                   compute_dtype="f32")
        self._path.pin(False)
        self.last_heads = self.last_selection = self.last_detections = self.last_class_masks = None

    def _make_top(self, cfg, dev, seed, extra):
        return DetectTop([cfg.POOL_SIZE, cfg.POOL_SIZE, 256], cfg.NUM_CLASSES, dev, seed, extra_params=extra, mask_pool=cfg.MASK_POOL_SIZE)

    # ---- what this class refuses -------------------------------------------------------------
    train, compile, train_on_batch, train_on_batch_device = (_no_training(n) for n in ("train", "compile", "train_on_batch", "train_on_batch_device"))
    test_on_batch, test_on_batch_device, forward_backward = (_no_training(n) for n in ("test_on_batch", "test_on_batch_device", "forward_backward"))
    set_trainable, plan_pair = _no_training("set_trainable"), _no_training("plan_pair")

    NO_STEP_GRAPH = "captured step graphs belong to training, which is not built for this class"
    use_step_graph, grad_sync = dense_model.REFUSED_STEP_GRAPH, dense_model.REFUSED_GRAD_SYNC

    def generate_captions(self, *args, **kw):
        raise ValueError("MaskRCNN has no caption decoder: use detect")

    # ---- weights -------------------------------------------------------------------------------
    def get_weights_dict(self):
        """'<layer>/<weight>' -> ndarray under the reference's layer names, in Keras' shapes (mrcnn_class_logits [1024,C],
        mrcnn_mask_conv* HWIO, mrcnn_mask_deconv [2,2,256,256], mrcnn_mask [1,1,256,C])."""
        out = DenseImageCapRCNN.get_weights_dict(self)
        top = self.caption_model
        return {k: top.from_stored(k, v) if k.startswith("mrcnn_") else v for k, v in out.items()}

    def set_weights(self, weights):
        top = self.caption_model
        W = dict(weights)
        W.update(top.to_stored({k: v for k, v in W.items() if k.split("/")[0] in ("mrcnn_class_logits", "mrcnn_mask") or
                                k.startswith("mrcnn_mask_conv")}))
        DenseImageCapRCNN.set_weights(self, W)             # (ends in the top's _weights_changed: the folded mask BatchNorms go)

    # ---- inference -----------------------------------------------------------------------------
    def detect(self, images, verbose=0, postprocess="host", mold="host", device_masks=False, refine="host", mask_format="dense"):
        """The inference graph + detect (:2314-2354).  Returns, per image, {"rois": int32 [N,4] in the original image, "class_ids": int32
        [N], "scores": float32 [N], "masks": uint8 [H,W,N] (a transposed view of [N,H,W]); (0,28,28) floats when nothing is detected, as
        the reference returns it}.  postprocess="host": the [N,28,28] class masks come to the host and utils.unmold_mask runs in NumPy /
        PIL; "device": ops.mask_paste and one copy of the finished bytes -- the same bytes.  mold: as DenseImageCapRCNN.generate_captions.
        device_masks=True (postprocess="device"): "masks" stays a uint8 [N,H,W] tensor on the device.
        refine="host" (default): the selection comes to the host (a device synchronisation in the middle of the call), refine_detections
        and unmold_boxes run in NumPy and the detections go up again; last_selection holds per image the four host arrays.
        refine="device": class_select -> ops.refine_detections (one launch) -> the mask head, with no host read in between; the mask
        head then always runs on B x DETECTION_MAX_INSTANCES rows (rows behind an image's last detection carry a zero box and class id
        -1 and give zero masks), whatever the images hold.  ONE small packed copy brings the counts and per row the boxes, rois, id,
        score and kept index (pack_detections); postprocess="device" pastes all rows first and, without device_masks, copies the [:n]
        mask bytes second; postprocess="host" copies the [B,M,28,28] class masks second.  last_selection holds the four DEVICE tensors
        (proposals [B,K,4], ids [B,K], scores [B,K], deltas [B,K,4]: buffers the next call reuses), last_class_masks device views as
        with postprocess="device".  Equal scores are ordered as np.argsort(kind="stable")[::-1] orders them (the host path's default
        sort promises no order), and the device's float64 exp is not np.exp bit for bit: see dc_refine_detections_f32.
        mask_format="rle": "masks" is a list of N COCO run-length encodings {"size": [H, W] of the original image, "counts": uint32
        ndarray} (mask_rle.py: decode, area, to_coco), an empty list when nothing is detected; decoded, each is the dense mode's plane
        byte for byte.  postprocess="host" encodes unmold_mask's planes with mask_rle.encode; postprocess="device" builds the encodings
        on the device (ops.mask_rle per image, in place of ops.mask_paste) and no [N,H,W] buffer exists anywhere.  The device mode
        makes TWO device-to-host copies per batch with refine="device" -- the detections pack and one pack of every image's offsets
        and counts -- and with refine="host" the selection copy and that one RLE pack; nothing reads the device between the image
        upload (refine="host": the detections' upload) and those copies.  Only where an image's encodings outgrow ops.mask_rle's
        capacity does that image cost a second launch and a copy of its own.  Not with device_masks=True."""
        if postprocess not in ("host", "device"):
            raise ValueError("postprocess must be 'host' or 'device', got %r" % (postprocess,))
        if device_masks and postprocess != "device":
            raise ValueError("device_masks=True needs postprocess='device'")
        if refine not in ("host", "device"):
            raise ValueError("refine must be 'host' or 'device', got %r" % (refine,))
        if mask_format not in ("dense", "rle"):
            raise ValueError("mask_format must be 'dense' or 'rle', got %r" % (mask_format,))
        if mask_format == "rle" and device_masks:
            raise ValueError("mask_format='rle' returns host run-length encodings: device_masks=True is not available with it")
        rle = mask_format == "rle"
        utils.check_mold(mold, self.config.IMAGE_PADDING)
        cfg, top, B = self.config, self.caption_model, len(images)
        if verbose:
            print("Processing %d images" % B)
        p, images, windows, consts, proposals, feats = self._proposal_features(images, mold, want_consts=refine == "device")
        K = proposals.shape[1]
        z, d = top.heads(feats.view(B * K, cfg.POOL_SIZE, cfg.POOL_SIZE, 256))
        self.last_heads = (z, d)
        if refine == "device":
            return self._detect_refined_on_device(p, images, consts, proposals, z, d, postprocess, device_masks, rle)
        # proposals, ids, scores and deltas leave in one buffer of 10 words per RoI: ids as their bits
        sel = self._buf("selection", (B * K, 10))
        sel[:, :4].copy_(proposals.view(B * K, 4))
        ids, scores, deltas = ops.class_select(z, d, class_ids=self._buf("sel_ids", (B * K,), torch.int32), scores=self._buf("sel_scores", (B * K,)),
                                               deltas_out=self._buf("sel_deltas", (B * K, 4)))
        sel[:, 4].copy_(ids.view(torch.float32))
        sel[:, 5].copy_(scores)
        sel[:, 6:].copy_(deltas)
        host = sel.cpu().numpy().reshape(B, K, 10)          # the one device-to-host copy of step 4
        self.last_selection = [(host[b, :, :4].copy(), host[b, :, 4].copy().view(np.int32), host[b, :, 5].copy(), host[b, :, 6:].copy())
                               for b in range(B)]
        h, w = cfg.IMAGE_SHAPE[:2]
        norm = np.array([h, w, h, w])
        dets, counts = [], []
        for b in range(B):
            rois_b, ids_b, scores_b, deltas_b = self.last_selection[b]
            boxes, cls, sc, _ = refine_detections(rois_b, ids_b, scores_b, deltas_b, np.asarray(windows[b], np.float32), cfg)
            final, ok = unmold_boxes(boxes, images[b].shape, windows[b])
            dets.append(dict(boxes=boxes[ok], class_ids=cls[ok], scores=sc[ok], rois=final[ok]))
            counts.append(int(ok.sum()))
        self.last_detections = dets
        M = max(counts)
        self.last_class_masks = [np.zeros((0, 2 * top.mask_pool, 2 * top.mask_pool), np.float32) for _ in range(B)]
        results = [{"rois": dt["rois"], "class_ids": dt["class_ids"], "scores": dt["scores"],
                    "masks": [] if rle else np.empty((0, 2 * top.mask_pool, 2 * top.mask_pool))} for dt in dets]
        if M == 0:
            if device_masks:
                for b in range(B):
                    results[b]["masks"] = torch.empty((0,) + tuple(images[b].shape[:2]), dtype=torch.uint8, device=self.device)
            return results
        # one packed upload: per image M rows of (normalised detection box as float32 bits, class id, box in the original image);
        # padding rows carry a zero box and class id -1, which gives zero masks
        pack = np.zeros((B, M, 9), np.int32)
        pack[:, :, 4] = -1
        for b, dt in enumerate(dets):
            n = counts[b]
            pack[b, :n, :4] = (dt["boxes"].astype(np.float32) / norm).astype(np.float32).view(np.int32)
            pack[b, :n, 4] = dt["class_ids"]
            pack[b, :n, 5:] = dt["rois"]
        up = torch.from_numpy(pack).to(self.device)
        det_norm = up[:, :, :4].contiguous().view(torch.float32)
        det_ids = up[:, :, 4].contiguous().view(B * M)
        P = top.mask_pool
        x = ops.roi_align_pyramid(list(p.P), det_norm, float(p.H * p.W), P, out=self._buf("mask_rois", (B, M, P, P, 256)))
        masks = top.class_masks(x.view(B * M, P, P, 256), det_ids, out=self._buf("class_masks", (B * M, 2 * P, 2 * P))).view(B, M, 2 * P, 2 * P)
        if postprocess == "host":
            masks_h = masks.cpu().numpy()
            for b in range(B):
                n = counts[b]
                self.last_class_masks[b] = masks_h[b, :n].copy()
                if n and rle:
                    results[b]["masks"] = [mask_rle.encode(unmold_mask(masks_h[b, i], dets[b]["rois"][i], images[b].shape)) for i in range(n)]
                elif n:
                    full = np.stack([unmold_mask(masks_h[b, i], dets[b]["rois"][i], images[b].shape) for i in range(n)])
                    results[b]["masks"] = full.transpose(1, 2, 0)
            return results
        if rle:
            runs = {b: ops.mask_rle(masks[b, :counts[b]], up[b, :counts[b], 5:].contiguous(), *images[b].shape[:2]) for b in range(B) if counts[b]}
            for b, found in self._rle_lists(runs).items():
                results[b]["masks"] = found
            self.last_class_masks = [masks[b, :counts[b]] for b in range(B)]
            return results
        keep = []
        for b in range(B):
            n = counts[b]
            if not n:
                if device_masks:
                    results[b]["masks"] = torch.empty((0,) + tuple(images[b].shape[:2]), dtype=torch.uint8, device=self.device)
                continue
            H0, W0 = images[b].shape[:2]
            full = ops.mask_paste(masks[b, :n], up[b, :n, 5:].contiguous(), H0, W0)
            keep.append((b, full))
        for b, full in keep:
            results[b]["masks"] = full if device_masks else full.cpu().numpy().transpose(1, 2, 0)
        self.last_class_masks = [masks[b, :counts[b]] for b in range(B)]     # (device views of a buffer the next call reuses)
        return results

    @staticmethod
    def _rle_lists(runs):
        """{image: ops.MaskRle} -> {image: list of RLE dicts}, with ONE device-to-host copy for all of them."""
        if not runs:
            return {}
        host = torch.cat([r.pack for r in runs.values()]).cpu().numpy()
        cuts = np.cumsum([0] + [r.pack.numel() for r in runs.values()])
        return {b: r.rles(host[lo:hi]) for (b, r), lo, hi in zip(runs.items(), cuts[:-1], cuts[1:])}

    def _detect_refined_on_device(self, p, images, consts, proposals, z, d, postprocess, device_masks, rle=False):
        """detect(refine="device") behind the heads: nothing here reads the device before pack_detections."""
        B, P = proposals.shape[0], self.caption_model.mask_pool
        count, boxes, rois, norm, cls, sc, keep = self._refine_on_device(consts, proposals, z, d)
        masks = self._class_masks_fixed(p, norm, cls)
        full = runs = None
        if postprocess == "device" and rle:              # padded rows carry zero boxes: they encode as [H * W] and are dropped below
            runs = {b: ops.mask_rle(masks[b], rois[b], *images[b].shape[:2]) for b in range(B)}
        elif postprocess == "device":
            full = [ops.mask_paste(masks[b], rois[b], *images[b].shape[:2]) for b in range(B)]
        n, boxes_h, rois_h, cls_h, sc_h, _ = pack_detections(count, boxes, rois, cls, sc, keep)
        self.last_detections = [dict(boxes=boxes_h[b, :n[b]], class_ids=cls_h[b, :n[b]], scores=sc_h[b, :n[b]], rois=rois_h[b, :n[b]]) for b in range(B)]
        results = [{"rois": dt["rois"], "class_ids": dt["class_ids"], "scores": dt["scores"],
                    "masks": [] if rle else np.empty((0, 2 * P, 2 * P))} for dt in self.last_detections]
        if postprocess == "host":
            masks_h = masks.cpu().numpy()
            self.last_class_masks = [masks_h[b, :n[b]].copy() for b in range(B)]
            for b in range(B):
                if n[b] and rle:
                    results[b]["masks"] = [mask_rle.encode(unmold_mask(masks_h[b, i], rois_h[b, i], images[b].shape)) for i in range(n[b])]
                elif n[b]:
                    full_b = np.stack([unmold_mask(masks_h[b, i], rois_h[b, i], images[b].shape) for i in range(n[b])])
                    results[b]["masks"] = full_b.transpose(1, 2, 0)
            return results
        if rle:
            for b, found in self._rle_lists(runs).items():
                results[b]["masks"] = found[:n[b]]
            self.last_class_masks = [masks[b, :n[b]] for b in range(B)]
            return results
        for b in range(B):
            if device_masks:
                results[b]["masks"] = full[b][:n[b]]
            elif n[b]:
                results[b]["masks"] = full[b][:n[b]].cpu().numpy().transpose(1, 2, 0)
        self.last_class_masks = [masks[b, :n[b]] for b in range(B)]          # (device views of a buffer the next call reuses)
        return results

    def _refine_on_device(self, consts, proposals, z, d):
        """class_select -> ops.refine_detections: its seven device tensors of DETECTION_MAX_INSTANCES rows per image."""
        cfg, (B, K) = self.config, proposals.shape[:2]
        ids, scores, deltas = ops.class_select(z, d, class_ids=self._buf("sel_ids", (B * K,), torch.int32), scores=self._buf("sel_scores", (B * K,)),
                                               deltas_out=self._buf("sel_deltas", (B * K, 4)))
        self.last_selection = (proposals, ids.view(B, K), scores.view(B, K), deltas.view(B, K, 4))
        return ops.refine_detections(*self.last_selection, consts, cfg.BBOX_STD_DEV, cfg.DETECTION_MIN_CONFIDENCE, cfg.DETECTION_NMS_THRESHOLD,
                                     int(cfg.DETECTION_MAX_INSTANCES), cfg.IMAGE_SHAPE[:2])

    def _class_masks_fixed(self, p, norm, cls):
        """The mask head on every row of ops.refine_detections' result: float32 [B,M,2P,2P] on the device."""
        top, (B, M) = self.caption_model, cls.shape
        P = top.mask_pool
        x = ops.roi_align_pyramid(list(p.P), norm, float(p.H * p.W), P, out=self._buf("mask_rois_fixed", (B, M, P, P, 256)))
        return top.class_masks(x.view(B * M, P, P, 256), cls.view(B * M), out=self._buf("class_masks_fixed", (B * M, 2 * P, 2 * P))).view(B, M, 2 * P, 2 * P)

    # ---- evaluation ----------------------------------------------------------------------------
    EVAL_RLE_CAPACITY = None       # evaluate(backend="device"): ops.mask_rle's first capacity in words; None: ops.mask_rle_capacity's

    @staticmethod
    def _eval_ground_truth(b, image, gt, overlap):
        """One image's ground truth, checked: (class_ids int32 [G], rles: list of G encodings or None, rois int32 [G,4], iscrowd uint8 [G])."""
        who = "evaluate: ground_truth[%d]" % b
        H, W = (int(v) for v in image.shape[:2])
        class_ids = np.asarray(gt["class_ids"]).reshape(-1)
        if class_ids.size and class_ids.dtype.kind not in "iu":
            raise ValueError("%s: class_ids must be integers, got %s" % (who, class_ids.dtype))
        G = class_ids.size
        if G > ops.EVAL_MAX:
            raise ValueError("%s: %d ground truths: more than %d ground truths in an image are not available" % (who, G, ops.EVAL_MAX))
        rles, masks = None, gt.get("masks")
        if masks is not None and not isinstance(masks, (list, tuple)):
            masks = np.asarray(masks)
            if masks.ndim != 3 or masks.dtype not in (np.dtype(bool), np.dtype(np.uint8)) or masks.shape[2] != G:
                raise ValueError("%s: dense masks must be a bool or uint8 [H,W,%d] array, got %s %s" % (who, G, masks.dtype, masks.shape))
            if tuple(masks.shape[:2]) != (H, W):
                raise ValueError("%s: the masks are %d x %d, the image %d x %d: a ground-truth mask of another size than its image is not "
                                 "available" % (who, masks.shape[0], masks.shape[1], H, W))
            rles = [mask_rle.encode(masks[:, :, g]) for g in range(G)]
        elif masks is not None:
            if len(masks) != G:
                raise ValueError("%s: %d masks for %d class ids" % (who, len(masks), G))
            for r in masks:
                if [int(v) for v in r["size"]] != [H, W]:
                    raise ValueError("%s: a mask is %s, the image %d x %d: a ground-truth mask of another size than its image is not "
                                     "available" % (who, list(r["size"]), H, W))
            rles = [{"size": [H, W], "counts": mask_rle._size_and_counts(r, "iou")[2].astype(np.uint32)} for r in masks]
        if overlap == "mask" and rles is None:
            raise ValueError("%s: overlap='mask' needs \"masks\"" % who)
        if gt.get("rois") is not None:
            rois = np.asarray(gt["rois"]).astype(np.int32).reshape(-1, 4)
            if rois.shape[0] != G:
                raise ValueError("%s: %d rois for %d class ids" % (who, rois.shape[0], G))
        elif rles is not None:
            rois = np.stack([mask_rle.to_bbox(r) for r in rles]).astype(np.int32) if G else np.zeros((0, 4), np.int32)
        else:
            raise ValueError("%s: overlap='box' needs \"rois\" or \"masks\" to take them from" % who)
        crowd = np.zeros(G, np.uint8) if gt.get("iscrowd") is None else (np.asarray(gt["iscrowd"]).reshape(-1) != 0).astype(np.uint8)
        if crowd.size != G:
            raise ValueError("%s: %d iscrowd flags for %d class ids" % (who, crowd.size, G))
        if overlap == "box" and crowd.any():
            raise ValueError("%s: iscrowd changes the mask IoU only: crowd flags with overlap='box' are not available" % who)
        return class_ids.astype(np.int32), rles, rois, crowd

    def evaluate(self, images, ground_truth, overlap="mask", iou_thresholds=None, backend="device", mold="host", verbose=0, **other):
        """Average precision of detect()'s results against annotated images: utils.compute_ap's rule (detection_eval.py states it and
        its two tie rules) on mask IoU (overlap="mask": pycocotools' rleIou on run-length encodings, mask_rle.iou) or box IoU
        (overlap="box": utils.compute_overlaps), at every threshold of iou_thresholds (default detection_eval.DEFAULT_THRESHOLDS, 0.5 to
        0.95; at most 16).  ground_truth[b]: {"class_ids": int [G]; "masks": dense [H,W,G] bool / uint8 or a list of G RLE dictionaries,
        in the original image; "rois": int32 [G,4], optional with masks (mask_rle.to_bbox derives them), needed for overlap="box"
        without masks; "iscrowd": optional [G], changes the mask IoU only (I / a_d)}.
        Returns {"AP": float64 [B,T], NaN for an image without ground truth; "mAP": float64 [T], the mean over the images that have
        ground truth; "thresholds"; "n_det", "n_gt": int32 [B]; "skipped": the images without ground truth; "pred_match": per image
        int32 [T,n_det] in rank order, "gt_match": per image int32 [T,n_gt], "order": per image int32 [n_det]
        (detection_eval.ap_from_overlaps)}.  The detections are those of detect(refine="device", postprocess="device") either way.
        backend="host": detect(mask_format="rle") as it stands, then mask_rle.iou or utils.compute_overlaps and
        detection_eval.ap_from_overlaps in NumPy.  backend="device": the same path up to ops.mask_rle per image, whose pack stays on
        the device; the ground truth (encodings, boxes, classes, thresholds) goes up in ONE packed upload; ops.rle_iou per image or
        ops.box_iou, then ops.detection_ap; ONE copy brings AP, matches, counts and status down, and nothing reads the device before
        it.  Only an image whose encodings outgrow ops.mask_rle's capacity costs a second launch, and the batch a second copy.  Both
        backends return the same dictionary, bit for bit.
        Not available: device_masks, a ground-truth mask of another size than its image, more than 1024 ground truths or detections an
        image (and, refused where the model is built, compute_dtype="bf16" and GPU_COUNT > 1).  Out of scope: COCO's 101-point
        interpolation, area ranges, maxDets and crowd regions as "ignore" in the matching."""
        from . import detection_eval
        if "device_masks" in other:
            raise ValueError("evaluate: device_masks is not available: the masks are scored as run-length encodings and never returned")
        if other:
            raise TypeError("evaluate() got an unexpected keyword argument %r" % sorted(other)[0])
        if overlap not in ("mask", "box"):
            raise ValueError("overlap must be 'mask' or 'box', got %r" % (overlap,))
        if backend not in ("host", "device"):
            raise ValueError("backend must be 'host' or 'device', got %r" % (backend,))
        cfg, B = self.config, len(images)
        M = int(cfg.DETECTION_MAX_INSTANCES)
        if M > ops.EVAL_MAX:
            raise ValueError("evaluate: DETECTION_MAX_INSTANCES = %d: more than %d detections in an image are not available" % (M, ops.EVAL_MAX))
        if len(ground_truth) != B:
            raise ValueError("evaluate: %d images but %d ground-truth entries" % (B, len(ground_truth)))
        thresholds = np.ascontiguousarray(detection_eval.DEFAULT_THRESHOLDS if iou_thresholds is None else iou_thresholds, np.float64).reshape(-1)
        T = len(thresholds)
        if not 1 <= T <= detection_eval.MAX_THRESHOLDS:
            raise ValueError("evaluate: 1 to %d IoU thresholds, got %d" % (detection_eval.MAX_THRESHOLDS, T))
        utils.check_mold(mold, cfg.IMAGE_PADDING)
        gts = [self._eval_ground_truth(b, images[b], ground_truth[b], overlap) for b in range(B)]
        n_gt = np.array([len(g[0]) for g in gts], np.int32)
        if backend == "host":
            found = self.detect(images, verbose=verbose, postprocess="device", mold=mold, refine="device", mask_format="rle")
            n_det = np.array([len(r["rois"]) for r in found], np.int32)
            ap, pred_match, gt_match, order = np.full((B, T), np.nan), [], [], []
            for b, (r, (gt_ids, rles, rois, crowd)) in enumerate(zip(found, gts)):
                if overlap == "mask":
                    ov = mask_rle.iou(r["masks"], rles, crowd)
                else:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        ov = utils.compute_overlaps(r["rois"].astype(np.int32).reshape(-1, 4), rois)
                ap[b], pm, gm, od = detection_eval.ap_from_overlaps(ov, gt_ids, r["class_ids"], r["scores"], thresholds)
                pred_match.append(pm)
                gt_match.append(gm)
                order.append(od.astype(np.int32))
        else:
            n_det, ap, pred_match, gt_match, order = self._evaluate_on_device(images, gts, n_gt, overlap, thresholds, mold, verbose)
        have = n_gt > 0
        return {"AP": ap, "mAP": ap[have].mean(axis=0) if have.any() else np.full(T, np.nan), "thresholds": thresholds.copy(), "n_det": n_det,
                "n_gt": n_gt, "skipped": int((~have).sum()), "pred_match": pred_match, "gt_match": gt_match, "order": order}

    def _evaluate_on_device(self, images, gts, n_gt, overlap, thresholds, mold, verbose):
        """evaluate(backend="device") behind the checks: (n_det [B], AP [B,T], pred_match, gt_match, order) on the host after ONE copy."""
        cfg, top, B, T = self.config, self.caption_model, len(images), len(thresholds)
        M, Gmax, masked = int(cfg.DETECTION_MAX_INSTANCES), int(n_gt.max()) if B else 0, overlap == "mask"
        if verbose:
            print("Evaluating %d images" % B)
        # ONE packed upload of int32 words: thresholds (float64 bits), boxes [B,Gmax,4] on a 16-byte boundary, n_gt [B], classes
        # [B,Gmax], then per image with ground truth its offsets [G+1], counts and crowd flags (bytes, padded to words)
        head = [np.zeros((2 * T + 3) // 4 * 4, np.int32), np.zeros((B, Gmax, 4), np.int32), n_gt, np.zeros((B, Gmax), np.int32)]
        head[0][:2 * T] = thresholds.view(np.int32)
        per_image, words = {}, []
        for b, (gt_ids, rles, rois, crowd) in enumerate(gts):
            G = len(gt_ids)
            head[1][b, :G], head[3][b, :G] = rois, gt_ids
            if masked and G:
                lengths = [len(r["counts"]) for r in rles]
                flags = np.zeros((G + 3) // 4 * 4, np.uint8)
                flags[:G] = crowd
                per_image[b] = (G, int(np.sum(lengths)))
                words += [np.cumsum([0] + lengths).astype(np.int32), np.concatenate([r["counts"] for r in rles]).astype(np.uint32).view(np.int32),
                          flags.view(np.int32)]
        parts = [a.reshape(-1) for a in head] + words
        up_host = np.concatenate(parts) if parts else np.zeros(0, np.int32)
        p, images, windows, consts, proposals, feats = self._proposal_features(images, mold, want_consts=True)
        up = torch.from_numpy(up_host).to(self.device)
        cuts = np.cumsum([0] + [a.size for a in parts])
        thr_d = up[:2 * T].view(torch.float64)
        gt_boxes, n_gt_d, gt_cls = up[cuts[1]:cuts[2]].view(B, Gmax, 4), up[cuts[2]:cuts[3]], up[cuts[3]:cuts[4]].view(B, Gmax)
        K = proposals.shape[1]
        z, d = top.heads(feats.view(B * K, cfg.POOL_SIZE, cfg.POOL_SIZE, 256))
        self.last_heads = (z, d)
        count, boxes, rois, norm, cls, sc, keep = self._refine_on_device(consts, proposals, z, d)
        # everything that comes down, in one int32 buffer: AP (float64 bits), pred_match, gt_match, order, counts, status
        sizes = [2 * B * T, B * T * M, B * T * Gmax, B * M, B, 4 * B]
        down = torch.zeros((int(np.sum(sizes)),), dtype=torch.int32, device=self.device)
        dcut = np.cumsum([0] + sizes)
        ap_d, pm_d, gm_d = down[:dcut[1]].view(torch.float64).view(B, T), down[dcut[1]:dcut[2]].view(B, T, M), down[dcut[2]:dcut[3]].view(B, T, Gmax)
        od_d, cnt_d, st_d = down[dcut[3]:dcut[4]].view(B, M), down[dcut[4]:dcut[5]], down[dcut[5]:].view(B, 4)
        overlaps = torch.empty((B, M, Gmax), dtype=torch.float64, device=self.device)
        runs = {}

        def mask_overlaps(b, at):
            G, n_words = per_image[b]
            offs_g, counts_g, crowd = up[at:at + G + 1], up[at + G + 1:at + G + 1 + n_words], up[at + G + 1 + n_words:at + G + 1 + n_words + (G + 3) // 4]
            ops.rle_iou(runs[b].offsets, runs[b].counts, offs_g, counts_g, *images[b].shape[:2], n_det=count[b:b + 1],
                        iscrowd=crowd.view(torch.uint8)[:G], out=overlaps[b, :, :G], status=st_d[b])

        def score():
            cnt_d.copy_(count)
            ops.detection_ap(overlaps, count, n_gt_d, cls, sc, gt_cls, thr_d, ap=ap_d, pred_match=pm_d, gt_match=gm_d, order=od_d)
            return down.cpu().numpy()                    # the ONE device-to-host copy

        where = {}
        if masked:
            masks = self._class_masks_fixed(p, norm, cls)
            at = int(cuts[4])
            for b in sorted(per_image):
                H0, W0 = images[b].shape[:2]
                runs[b] = ops.mask_rle(masks[b], rois[b], H0, W0, capacity=self.EVAL_RLE_CAPACITY)
                where[b] = at
                mask_overlaps(b, at)
                at += per_image[b][0] + 1 + per_image[b][1] + (per_image[b][0] + 3) // 4
        else:
            ops.box_iou(rois, gt_boxes, out=overlaps)
        host = score()
        status = host[dcut[5]:].reshape(B, 4)
        if status[:, 1:3].any():
            raise ops._lib.DcapError("evaluate: ops.rle_iou reports a ground-truth encoding it could not read (status %s)" % status.tolist())
        short = [b for b in range(B) if status[b, 0]]
        for b in short:                                  # the detections' encodings outgrew the capacity: once more with what they need
            runs[b].relaunch(int(status[b, 0]))
            mask_overlaps(b, where[b])
        if short:
            host = score()
            if host[dcut[5]:].reshape(B, 4)[:, :3].any():
                raise ops._lib.DcapError("evaluate: the second ops.mask_rle run still does not fit (status %s)" % host[dcut[5]:].reshape(B, 4).tolist())
        self.last_eval_relaunched = short
        n_det = host[dcut[4]:dcut[5]].copy()
        ap = host[:dcut[1]].view(np.float64).reshape(B, T).copy()
        pm, gm, od = host[dcut[1]:dcut[2]].reshape(B, T, M), host[dcut[2]:dcut[3]].reshape(B, T, Gmax), host[dcut[3]:dcut[4]].reshape(B, M)
        return (n_det, ap, [pm[b, :, :n_det[b]].copy() for b in range(B)], [gm[b, :, :n_gt[b]].copy() for b in range(B)],
                [od[b, :n_det[b]].copy() for b in range(B)])
