"""Float64 NumPy restatement of the RoI tag head's loss (roi_tag_classification/model.py:48-66 focal_loss, :877-887
roi_tag_classes_loss_graph, on Keras 2.1's K.binary_crossentropy over probabilities), operation for operation, with the gradient as
TensorFlow differentiates it -- and a float64 tag joint step composed from the oracle's pieces.  Shared by tests/test_roitag_ref.py
(CPU) and the GPU tests; nothing here imports the package."""
import numpy as np

LO = float(np.float32(1e-7))                 # Keras casts epsilon and 1 - epsilon to the tensor's dtype, float32
HI = float(np.float32(1.0 - 1e-7))
Z_LO = float(np.log(LO / (1.0 - LO)))        # the clip thresholds on the logit: -16.1181 and 15.9424
Z_HI = float(np.log(HI / (1.0 - HI)))
NO_SCORE = np.float32(-3.4e38)


def sigmoid(z):
    """p and 1 - p, each without cancellation."""
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    return np.where(z >= 0, big, small), np.where(z >= 0, small, big)


def _power(fw, gamma):
    """fw ** gamma and its derivative in fw as exact products, gamma in {0, 1, 2}."""
    if gamma == 0:
        return np.ones_like(fw), np.zeros_like(fw)
    if gamma == 1:
        return fw, np.ones_like(fw)
    if gamma == 2:
        return fw * fw, 2.0 * fw
    raise ValueError("gamma must be 0, 1 or 2, got %r" % (gamma,))


def focal_elements(z, t, alpha=0.25, gamma=2):
    """(L, dL/dz) per element, every row treated as live.  z float [..], t integer [..] of the same shape."""
    z = np.asarray(z, np.float64)
    one = np.asarray(t) == 1
    tf = np.asarray(t).astype(np.float64)
    p, omp = sigmoid(z)
    inside = (p >= LO) & (p <= HI)                                   # the clip passes gradient only here
    q = np.clip(p, LO, HI)
    x = np.log(q / (1.0 - q))
    bce = np.maximum(x, 0.0) - x * tf + np.log1p(np.exp(-np.abs(x)))     # tf.nn.sigmoid_cross_entropy_with_logits
    fw = np.where(one, omp, p)                                       # the UNCLIPPED p
    a = np.where(one, alpha, 1.0 - alpha)
    fwg, dfwg = _power(fw, gamma)
    L = a * fwg * bce
    dfw = np.where(one, -1.0, 1.0) * p * omp
    # d bce / dx = sigmoid(x) - t = q - t; dx/dq * dq/dp * dp/dz = [inside] p (1 - p) / (q (1 - q)) = [inside]
    dbce = np.where(inside, np.where(one, -omp, p - tf), 0.0)
    return L, a * (dfwg * dfw * bce + fwg * dbce)


def live_rows(t):
    return (np.asarray(t) == 1).any(axis=-1)


def tag_focal(z, t, alpha=0.25, gamma=2, grad_scale=1.0):
    """(loss_rows [M], dz [M,C]): dead rows are zeros whatever their logits hold (gather_nd removes them before any arithmetic)."""
    z = np.asarray(z, np.float64)
    live = live_rows(t)
    loss_rows, dz = np.zeros(z.shape[0]), np.zeros(z.shape)
    if live.any():
        L, g = focal_elements(z[live], np.asarray(t)[live], alpha, gamma)
        loss_rows[live] = L.sum(axis=1)
        dz[live] = g * grad_scale
    return loss_rows, dz


def plain_bce(z, t):
    """K.binary_crossentropy(t, sigmoid(z)) with Keras' clip, per element."""
    p, _ = sigmoid(z)
    q = np.clip(p, LO, HI)
    return -(np.asarray(t) * np.log(q) + (1.0 - np.asarray(t)) * np.log1p(-q))


def tag_scores(probs, min_confidence):
    """model.py:644-646 on float32 probabilities [M,C]: float32(sum of log(float64(p)) over p > min_confidence), or -3.4e38."""
    probs = np.asarray(probs, np.float32)
    thr = np.float32(min_confidence)
    out = np.empty(probs.shape[0], np.float32)
    for i, row in enumerate(probs):
        sel = row[row > thr]
        out[i] = np.float32(np.log(sel.astype(np.float64)).sum()) if sel.size else NO_SCORE
    return out


# ---- direct-test cases (tests/test_gpu_tag_focal.py; the CPU test checks what they promise) --------------------------------------
SHAPES = [(1, 1), (3, 5), (7, 64), (12, 257), (5, 1023), (2, 4100)]
PLANTED = [15.0, -15.0, 17.0, -17.0, 30.0, -30.0, 88.0, -88.0, 200.0, -200.0]


def focal_case(M, C, seed=0):
    """(z float32 [M,C], t int32 [M,C]): logits normal * 4 with the planted values scattered over them, every logit at least 0.05 away
    from both clip thresholds; rows: odd rows dead (when M > 2), the last live row all ones, the first row's only 1 in its last column,
    the other live rows random multi-hot."""
    rng = np.random.RandomState(1000 * M + C + seed)
    z = (rng.randn(M, C) * 4.0).astype(np.float32)
    flat = z.reshape(-1)
    where = rng.permutation(flat.size)
    for i, v in enumerate(PLANTED * 2):
        flat[where[i % flat.size]] = v
    for thr in (Z_LO, Z_HI):
        near = np.abs(flat - thr) < 0.05
        flat[near] = thr + 0.1
    t = (rng.rand(M, C) < 0.3).astype(np.int32)
    t[:, 0] = 1                                            # live unless made dead below
    if M > 2:
        t[1::2] = 0
    live = np.flatnonzero(t.any(axis=1))
    t[live[0]] = 0
    t[live[0], C - 1] = 1
    if len(live) > 1:
        t[live[-1]] = 1
    return z, t


def strided(a, ld):
    """The rows of a [M,C] inside a fresh [M,ld] array filled with a sentinel (the caller slices [:, :C])."""
    out = np.full((a.shape[0], ld), 77, a.dtype)
    out[:, :a.shape[1]] = a
    return out


# ---- the float64 tag joint step ---------------------------------------------------------------------------------------------------
TAG_TRAINABLE_PREFIXES = ('roitag_', 'rpn_', 'fpn_', 'mrcnn_')


def tag_trainable(Wt):
    """layers="no_backbone" of the tag model: roitag_*, rpn_*, fpn_*, mrcnn_*; BN moving statistics are not variables."""
    return [k for k in Wt if k.startswith(TAG_TRAINABLE_PREFIXES) and 'moving_' not in k]


def tag_joint_loss_and_grads(Wt, image_u8, rpn_match, rpn_bbox_target, cfg, targets, stage4_blocks=22, backbone_from=None, term_weights=None,
                             alpha=0.25, gamma=2):
    """One training step's losses and gradients of the tag model for ONE image: the body of oracle.np_models.joint_loss_and_grads with the
    caption decoder replaced by roi_head_forward / roi_head_backward + Dense(NUM_CLASSES) + the focal loss above.
    targets = (rois [R,4] normalised, classes [R,C]): the DetectionTargetLayer's sample (it carries no gradient; the tests hand in the
    one the device drew).  cfg, term_weights (roi_tag_classes_loss, rpn_class_loss, rpn_bbox_loss, reg_loss): as in the oracle.
    Returns (losses dict, grads dict over tag_trainable(Wt) [+ the trainable backbone], aux dict(proposals, loss_rows))."""
    from oracle import np_models as M
    from oracle import np_oracle as O
    F64 = np.float64
    x = O.mold_image(image_u8[None], cfg['mean_pixel'])
    _, H, W, _ = x.shape
    tw = dict(roi_tag_classes_loss=1.0, rpn_class_loss=1.0, rpn_bbox_loss=1.0, reg_loss=1.0)
    tw.update(term_weights or {})
    if backbone_from is None:
        _, C2, C3, C4, C5 = M.resnet_graph(x, Wt, stage4_blocks)
        Cs = {2: C2, 3: C3, 4: C4, 5: C5}
    else:
        Cs, trunk_caches = M.resnet_graph_cached(x, Wt, stage4_blocks)
    conv = lambda t, n, pad='valid': O.conv2d_nhwc(t, Wt[n + '/kernel'], Wt[n + '/bias'], 1, pad)
    pre = {5: conv(Cs[5], 'fpn_c5p5')}
    for k in (4, 3, 2):
        pre[k] = O.upsample2x(pre[k + 1]) + conv(Cs[k], 'fpn_c%dp%d' % (k, k))
    P = {k: conv(pre[k], 'fpn_p%d' % k, 'same') for k in (2, 3, 4, 5)}
    P[6] = O.subsample2(P[5])
    shared, cls, box = {}, {}, {}
    for k in (2, 3, 4, 5, 6):
        shared[k] = O.relu(conv(P[k], 'rpn_conv_shared', 'same'))
        cls[k] = conv(shared[k], 'rpn_class_raw')
        box[k] = conv(shared[k], 'rpn_bbox_pred')
    logits = np.concatenate([cls[k].reshape(1, -1, 2) for k in (2, 3, 4, 5, 6)], axis=1)[0]
    bbox = np.concatenate([box[k].reshape(1, -1, 4) for k in (2, 3, 4, 5, 6)], axis=1)[0]
    probs = O.softmax(logits)
    shapes = [[-(-H // s_), -(-W // s_)] for s_ in cfg['strides']]
    anchors = O.generate_pyramid_anchors(cfg['scales'], cfg['ratios'], shapes, cfg['strides'], 1)
    proposals, _, _ = O.proposal_layer(probs[:, 1], bbox, anchors, (H, W), cfg['proposal_count'], cfg['nms'])
    rois, classes = np.asarray(targets[0], np.float32), np.asarray(targets[1])
    maps = [P[2], P[3], P[4], P[5]]
    feats = O.pyramid_roi_align(rois[None], maps, (H, W, 3), 7)[0]
    # ---- the tag top
    h, cache = M.roi_head_forward(feats, Wt)
    Wk, bk = np.asarray(Wt['roitag_class_logits/kernel'], F64), np.asarray(Wt['roitag_class_logits/bias'], F64)
    loss_rows, dz = tag_focal(h @ Wk + bk, classes, alpha, gamma, grad_scale=tw['roi_tag_classes_loss'])
    losses = {'roi_tag_classes_loss': tw['roi_tag_classes_loss'] * float(loss_rows.sum())}
    l_cls, dlogits = O.rpn_class_loss(rpn_match, logits)
    l_box, dbbox = O.rpn_bbox_loss(rpn_bbox_target, rpn_match, bbox)
    losses['rpn_class_loss'], losses['rpn_bbox_loss'] = tw['rpn_class_loss'] * l_cls, tw['rpn_bbox_loss'] * l_box
    dlogits, dbbox = dlogits * tw['rpn_class_loss'], dbbox * tw['rpn_bbox_loss']
    train = tag_trainable(Wt) + (M.backbone_trainable(Wt, backbone_from, stage4_blocks) if backbone_from is not None else [])
    reg_keys = [k for k in train if 'gamma' not in k and 'beta' not in k]
    losses['reg_loss'] = tw['reg_loss'] * float(sum(cfg['weight_decay'] * (np.asarray(Wt[k], F64) ** 2).sum() / np.asarray(Wt[k]).size for k in reg_keys))
    losses['loss'] = sum(losses[k] for k in ('roi_tag_classes_loss', 'rpn_class_loss', 'rpn_bbox_loss', 'reg_loss'))
    # ---- backward
    G = M.roi_head_backward(dz @ Wk.T, cache)
    G['roitag_class_logits/kernel'], G['roitag_class_logits/bias'] = h.T @ dz, dz.sum(axis=0)
    dfeat = G.pop('_dx').reshape(feats.shape)
    dP = O.pyramid_roi_align_backward(rois[None], [m.shape for m in maps], (H, W, 3), dfeat[None])
    dP = {k: dP[i] for i, k in enumerate((2, 3, 4, 5))}
    dP[6] = np.zeros_like(P[6])
    off = 0
    acc = lambda name, val: G.__setitem__(name, G.get(name, 0.0) + val)
    for k in (2, 3, 4, 5, 6):
        n = cls[k].shape[1] * cls[k].shape[2] * len(cfg['ratios'])
        dcls = dlogits[off:off + n].reshape(cls[k].shape)
        dbox = dbbox[off:off + n].reshape(box[k].shape)
        off += n
        ds1, dw, db = O.conv2d_nhwc_backward(shared[k], Wt['rpn_class_raw/kernel'], dcls)
        acc('rpn_class_raw/kernel', dw); acc('rpn_class_raw/bias', db)
        ds2, dw, db = O.conv2d_nhwc_backward(shared[k], Wt['rpn_bbox_pred/kernel'], dbox)
        acc('rpn_bbox_pred/kernel', dw); acc('rpn_bbox_pred/bias', db)
        dsh = (ds1 + ds2) * (shared[k] > 0)
        dpk, dw, db = O.conv2d_nhwc_backward(P[k], Wt['rpn_conv_shared/kernel'], dsh, 1, 'same')
        acc('rpn_conv_shared/kernel', dw); acc('rpn_conv_shared/bias', db)
        dP[k] = dP[k] + dpk
    dP[5][:, ::2, ::2, :] += dP[6]
    dpre = {}
    for k in (2, 3, 4, 5):
        dpre[k], dw, db = O.conv2d_nhwc_backward(pre[k], Wt['fpn_p%d/kernel' % k], dP[k], 1, 'same')
        G['fpn_p%d/kernel' % k], G['fpn_p%d/bias' % k] = dw, db
    for k in (2, 3, 4):
        g = dpre[k]
        N_, h_, w_, c_ = g.shape
        dpre[k + 1] = dpre[k + 1] + g.reshape(N_, h_ // 2, 2, w_ // 2, 2, c_).sum(axis=(2, 4))
    dC = {}
    for k in (2, 3, 4, 5):
        dC[k], dw, db = O.conv2d_nhwc_backward(Cs[k], Wt['fpn_c%dp%d/kernel' % (k, k)], dpre[k])
        G['fpn_c%dp%d/kernel' % (k, k)], G['fpn_c%dp%d/bias' % (k, k)] = dw, db
    if backbone_from is not None:
        G.update(M.resnet_backward(dC, trunk_caches, Wt, backbone_from))
    for k in reg_keys:
        G[k] = G[k] + tw['reg_loss'] * 2.0 * cfg['weight_decay'] * np.asarray(Wt[k], F64) / np.asarray(Wt[k]).size
    return losses, {k: G[k] for k in train}, dict(proposals=proposals, loss_rows=loss_rows)


def tag_joint_loss_and_grads_batch(Wt, images_u8, rpn_match, rpn_bbox_target, cfg, targets, stage4_blocks=22):
    """IMAGES_PER_GPU = B: the RPN losses are means over the whole batch's anchors (image b enters with its share of them, as in
    oracle.np_models.joint_loss_and_grads_batch); roi_tag_classes_loss is the plain SUM over all images' live rows; the regulariser
    is counted once.  targets = (rois [B,R,4], classes [B,R,C])."""
    B = len(images_u8)
    rpn_match = [np.asarray(m).reshape(-1) for m in rpn_match]
    n_sel = np.array([(m != 0).sum() for m in rpn_match], np.float64)
    n_pos = np.array([(m == 1).sum() for m in rpn_match], np.float64)
    share = lambda n: n / max(n.sum(), 1.0)
    w_cls, w_box = share(n_sel), share(n_pos)
    losses, grads, auxes = {}, {}, []
    for b in range(B):
        tw = dict(roi_tag_classes_loss=1.0, rpn_class_loss=w_cls[b], rpn_bbox_loss=w_box[b], reg_loss=1.0 if b == 0 else 0.0)
        l, g, aux = tag_joint_loss_and_grads(Wt, images_u8[b], rpn_match[b], rpn_bbox_target[b], cfg, (targets[0][b], targets[1][b]),
                                             stage4_blocks=stage4_blocks, term_weights=tw)
        for k, v in l.items():
            losses[k] = losses.get(k, 0.0) + v
        for k, v in g.items():
            grads[k] = grads.get(k, 0.0) + v
        auxes.append(aux)
    return losses, grads, auxes
