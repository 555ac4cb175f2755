"""Float64 references for the Mask R-CNN inference path, shared by tests/test_maskrcnn_ref.py (CPU) and the GPU tests; nothing here
imports the package.

  unmold_mask      utils.unmold_mask restated a second time, independently of mask_rcnn_model's: the bytescale step in float64 with
                   every result rounded to float32 explicitly (float64 carries more than twice float32's bits, so a float64 operation
                   rounded once more to float32 IS the float32 operation), the resize by tests/_resize_ref.py's integer restatement
                   of PIL's resample (pinned to PIL by tests/test_resize_geometry.py), the threshold on byte / 255 in float64.
  class_select     argmax of the logits (lowest index), 1 / sum exp(z - max), the winner's deltas.
  mask_tail        Conv2DTranspose(2x2, stride 2) + ReLU + 1x1 + sigmoid for each RoI's own class, with the running forward bound A.
  detection_heads / mask_head   the float64 heads on the oracle's maps (oracle functions imported, not edited)."""
import numpy as np

import _resize_ref as RS

F32, F64 = np.float32, np.float64
U = 2.0 ** -24


def _r(x):
    """Round a float64 result to float32 and carry on in float64."""
    return np.asarray(x, F64).astype(F32).astype(F64)


def bytescale(mask):
    m = np.asarray(mask, F32).astype(F64)
    cmin, cmax = m.min(), m.max()
    rng = _r(cmax - cmin)
    if rng == 0.0:
        rng = 1.0
    scale = _r(255.0 / rng)
    v = _r(_r(m - cmin) * scale)
    v = _r(np.minimum(np.maximum(v, 0.0), 255.0) + 0.5)
    return np.floor(v).astype(np.uint8)


def unmold_mask(mask, bbox, image_shape):
    y1, x1, y2, x2 = (int(v) for v in bbox)
    H, W = int(image_shape[0]), int(image_shape[1])
    full = np.zeros((H, W), np.uint8)
    if y2 <= y1 or x2 <= x1 or y1 < 0 or x1 < 0 or y2 > H or x2 > W:
        return full
    small = RS.resize_bilinear(bytescale(mask)[:, :, None], y2 - y1, x2 - x1)[:, :, 0]
    full[y1:y2, x1:x2] = (small.astype(F64) / 255.0 >= 0.5)
    return full


def class_select(logits, deltas):
    """(ids, scores float64, winner's deltas, d_max): d_max = the largest gap max - z_j of the case."""
    z = np.asarray(logits, F64)
    ids = z.argmax(axis=1)
    gap = z.max(axis=1, keepdims=True) - z
    scores = 1.0 / np.exp(-gap).sum(axis=1)
    d = np.asarray(deltas).reshape(z.shape[0], z.shape[1], 4)
    return ids, scores, d[np.arange(z.shape[0]), ids], float(gap.max())


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def mask_tail(x, wd, bd, wm, bm, class_ids):
    """x [N,P,P,Cin], wd [2,2,Cmid,Cin] (Keras' Conv2DTranspose kernel), bd [Cmid], wm [Cmid,C], bm [C], class_ids [N] ->
    (out [N,2P,2P] float64, z the pre-sigmoid values, A [N,2P,2P] = sum_c' (sum_c |x||wd| + |bd|) |wm| + |bm|).  An id outside [0,C)
    gives zeros (and A = 0)."""
    x, wd, bd, wm, bm = (np.asarray(a, F64) for a in (x, wd, bd, wm, bm))
    N, P = x.shape[0], x.shape[1]
    C = wm.shape[1]
    out, zs, A = np.zeros((N, 2 * P, 2 * P)), np.zeros((N, 2 * P, 2 * P)), np.zeros((N, 2 * P, 2 * P))
    for n in range(N):
        k = int(class_ids[n])
        if not 0 <= k < C:
            continue
        for dy in range(2):
            for dx in range(2):
                y = x[n] @ wd[dy, dx].T + bd                                   # [P,P,Cmid]
                ya = np.abs(x[n]) @ np.abs(wd[dy, dx]).T + np.abs(bd)
                z = np.maximum(y, 0.0) @ wm[:, k] + bm[k]
                zs[n, dy::2, dx::2] = z
                out[n, dy::2, dx::2] = sigmoid(z)
                A[n, dy::2, dx::2] = ya @ np.abs(wm[:, k]) + abs(bm[k])
    return out, zs, A


def mask_tail_tol(A, Cin, Cmid):
    """The running forward bound of the fp32 tail against float64: gamma A / 4 + 4 u with gamma = (Cin + Cmid + 4) u -- the two dot
    products' accumulated roundings on the magnitudes A, through the 1/4-Lipschitz sigmoid, plus the sigmoid's own few ulps."""
    return (Cin + Cmid + 4) * U * A / 4.0 + 4.0 * U


CONV_TOL = 2e-5          # tests/test_gpu_kernels.py::test_conv2d_matches_oracle: every fp32 convolution within 2e-5 of max(1, |y|max)
ROI_TOL = 1e-5           # tests/test_gpu_kernels.py::test_roi_align_pyramid, scaled the same way


def scale_mask_weights(Wt, conv1=0.02, mask=4.0):
    """The synthetic mask head at scales that can be tested: RoIAlign of the random encoder's maps averages 20 (up to 100), so the first
    convolution's glorot kernel is damped to bring the activations to O(1) -- where a BatchNorm beta (0.1) or a bias (0.01) is a visible
    share of every value -- and mrcnn_mask is widened so that the class masks spread over (0.2, 0.8) without saturating."""
    W = dict(Wt)
    W['mrcnn_mask_conv1/kernel'] = np.asarray(Wt['mrcnn_mask_conv1/kernel']) * F32(conv1)
    W['mrcnn_mask/kernel'] = np.asarray(Wt['mrcnn_mask/kernel']) * F32(mask)
    return W


def layer_tol(want, tol=CONV_TOL):
    return tol * max(1.0, float(np.abs(want).max()))


# ---- the float64 heads on the oracle's maps ---------------------------------------------------------------------------------------
def encoder_maps(Wt, image_u8, mean_pixel, stage4_blocks):
    from oracle import np_models as M
    from oracle import np_oracle as O
    x = O.mold_image(image_u8[None], mean_pixel)
    _, C2, C3, C4, C5 = M.resnet_graph(x, Wt, stage4_blocks)
    P2, P3, P4, P5, _ = M.fpn_graph(C2, C3, C4, C5, Wt)
    return [P2, P3, P4, P5], x.shape[1:3]


def detection_heads(Wt, maps, hw, proposals):
    """proposals [R,4] normalised -> (logits [R,C], deltas [R,4C]) in float64."""
    from oracle import np_models as M
    from oracle import np_oracle as O
    feats = O.pyramid_roi_align(np.asarray(proposals, F32)[None], maps, (hw[0], hw[1], 3), 7)[0]
    f, _ = M.roi_head_forward(feats, Wt)
    z = f @ np.asarray(Wt['mrcnn_class_logits/kernel'], F64) + np.asarray(Wt['mrcnn_class_logits/bias'], F64)
    d = f @ np.asarray(Wt['mrcnn_bbox_fc/kernel'], F64) + np.asarray(Wt['mrcnn_bbox_fc/bias'], F64)
    return z, d


def mask_layer(Wt, i, x):
    """mrcnn_mask_conv<i> + mrcnn_mask_bn<i> (inference statistics) + ReLU in float64, i = 1..4."""
    from oracle import np_oracle as O
    c, b = "mrcnn_mask_conv%d" % i, "mrcnn_mask_bn%d" % i
    y = O.conv2d_nhwc(np.asarray(x, F64), np.asarray(Wt[c + '/kernel'], F64), np.asarray(Wt[c + '/bias'], F64), 1, 'same')
    return O.relu(O.batchnorm_inference(y, *(np.asarray(Wt[b + '/' + n], F64) for n in ('gamma', 'beta', 'moving_mean', 'moving_variance'))))


def mask_tail_of(Wt, x4, class_ids):
    """mask_tail with the model's weights (Keras shapes): (out, z, A)."""
    wm = np.asarray(Wt['mrcnn_mask/kernel'], F64)
    return mask_tail(x4, Wt['mrcnn_mask_deconv/kernel'], Wt['mrcnn_mask_deconv/bias'], wm.reshape(wm.shape[-2], wm.shape[-1]), Wt['mrcnn_mask/bias'],
                     class_ids)


def tail_gain(Wt, class_ids):
    """[M,2,2]: sum_c' (sum_c |wd[dy,dx,c',c]|) |wm[c',k]| per detection and quadrant -- what a uniform error of the tail's input is
    multiplied by, at most, on its way to z."""
    wd, wm = np.abs(np.asarray(Wt['mrcnn_mask_deconv/kernel'], F64)), np.abs(np.asarray(Wt['mrcnn_mask/kernel'], F64))
    wm = wm.reshape(wm.shape[-2], wm.shape[-1])
    return np.stack([np.einsum('yxoc,o->yx', wd, wm[:, int(k)]) for k in class_ids])


def mask_head(Wt, maps, hw, boxes_norm, class_ids, pool=14):
    """build_fpn_mask_graph in float64 for each box's own class: (masks [M,2 pool,2 pool], the RoIAlign output and the four layers'
    outputs)."""
    from oracle import np_oracle as O
    xs = [O.pyramid_roi_align(np.asarray(boxes_norm, F32)[None], maps, (hw[0], hw[1], 3), pool)[0]]
    for i in (1, 2, 3, 4):
        xs.append(mask_layer(Wt, i, xs[-1]))
    return mask_tail_of(Wt, xs[-1], class_ids)[0], xs
