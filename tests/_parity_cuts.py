"""Cuts at the discrete decisions of a train step, for the model parity tests (NumPy only; importable without a GPU).

A model-level comparison with the float64 oracle is only as sharp as its treatment of the step's discontinuities: the sign of a ReLU
pre-activation in the RoI head, the top-k / NMS order of the proposals, the RoI sample.  The rule the checkers below implement:

  1. the device's INPUT to a decision is compared with the oracle's at a tolerance (check_rpn_heads, check_head_decisions' acc);
  2. the decision ITSELF is checked exactly, from the device's own input (check_proposals_from_device_scores, check_sample; for the
     ReLU: equal to the oracle's sign wherever the oracle's pre-activation is farther from zero than the device's rounding reaches);
  3. the decision is handed to the oracle for everything downstream (targets_override=, head_masks=);
  4. nothing is excluded from the comparison that follows.

tests/test_parity_cuts.py shows every checker failing on a planted error."""
import numpy as np

from oracle import np_oracle as O

U32 = 2.0 ** -24
F64 = np.float64
HEAD = (("mrcnn_class_conv1", "mrcnn_class_bn1"), ("mrcnn_class_conv2", "mrcnn_class_bn2"))
HEAD_K = (12544, 1024)                  # the head GEMMs' reduction lengths: K u is the worst-case bound of a fp32 sum of K terms
CLOSE_SET_CAP = 64                      # |C| per head layer (a condition on the INPUTS: computed from the oracle alone)
RPN_HEAD_TOL = 2e-4                     # rel_err of the RPN head outputs per level and image: what the full-size encoder test holds P2..P5 to

# c_acc: the device's head GEMM output against the oracle's, in units of u * (|x| @ |K|) (the reference's magnitude sum), per head layer.
# MEASURED on the MI355X, max |acc_dev - acc64| / (u * mag) over the whole [B*R, 1024] tensor:
#     two images x 200 RoIs (512 px, 2 blocks):   layer 1  0.882   layer 2  4.628
#     one image x 200 RoIs (512 px, 22 blocks):   layer 1  0.838   layer 2  4.285
# (layer 2's figure contains layer 1's error carried through a1).  The constant is 4 x the larger figure of each layer, rounded up
# to a power of two -- the margin is for another tile or split-K choice, which reorders a 12 544-term sum.  A value above K (HEAD_K)
# would mean the GEMM is wrong, not that the bound is tight.  4 x 0.882 = 3.5 -> 4;  4 x 4.628 = 18.5 -> 32.
C_ACC = (4.0, 32.0)
assert all(c <= k for c, k in zip(C_ACC, HEAD_K))


def rel_err(got, want):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    return float(np.abs(got - want).max()) / max(1e-30, float(np.abs(want).max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# RoI head: the two ReLU decisions
# ---------------------------------------------------------------------------------------------------------------------------------

def head_kinks(z64, mag, gamma, sd, extra, c_acc):
    """The close set C = {|z64| <= t}: the entries whose float64 pre-activation lies within the device's rounding reach of zero, so that
    the device's sign may differ.  t = c_acc u mag |gamma| / sd  (the GEMM's error bound carried through the BN scale)
                                     + 8 u extra               (bn_preact's own six roundings on the magnitudes it is computed from, the
                                                                bound tests/test_gpu_kernel_edges.py::test_bn_relu_fwd_bwd_against_float64
                                                                holds y to).
    Returns (C boolean like z64, t)."""
    t = c_acc * U32 * np.asarray(mag, F64) * np.abs(gamma) / sd + 8 * U32 * np.asarray(extra, F64)
    return np.abs(np.asarray(z64, F64)) <= t, t


def oracle_head_cache(auxes):
    """The oracle's head record of a batch in the device's row order (image b = rows [b*R, (b+1)*R)) from the aux dicts of
    M.joint_loss_and_grads (one) / M.joint_loss_and_grads_batch (a list)."""
    auxes = [auxes] if isinstance(auxes, dict) else list(auxes)
    cat = lambda key, i: np.concatenate([np.asarray(a[key][i], F64) for a in auxes], axis=0)
    return dict(z=(cat('head_z', 0), cat('head_z', 1)), mag=(cat('head_mag', 0), cat('head_mag', 1)), acc=(cat('head_acc', 0), cat('head_acc', 1)))


def device_head_masks(dev_hact):
    """The device's two ReLU decisions (its backward masks by y > 0, TF's ReluGrad) from its forward outputs hact0, hact1."""
    return tuple(np.asarray(h) > 0 for h in dev_hact)


def check_head_decisions(dev_acc, dev_hact, oracle_cache, weights, c_acc=C_ACC, cap=CLOSE_SET_CAP):
    """Per head layer li, over the whole [B*R, 1024] tensor:
      1. the device's GEMM output acc (no bias) equals the oracle's y - bias within c_acc[li] u mag, elementwise;
      2. the device's mask hact > 0 equals the oracle's z64 > 0 everywhere outside the close set C (head_kinks);
      3. |C| <= cap -- a condition on the inputs (oracle quantities only): a sample that exceeds it needs another image seed, not a larger cap.
    dev_acc = (acc0, acc1), dev_hact = (hact0, hact1): the device's buffers as arrays; oracle_cache: oracle_head_cache(aux);
    weights: the model's weight dict.  Returns (masks to hand to the oracle, report)."""
    masks, report = [], {}
    for li, (conv, bn) in enumerate(HEAD):
        acc_d, hact = np.asarray(dev_acc[li], F64), np.asarray(dev_hact[li])
        z64, mag, acc64 = (np.asarray(oracle_cache[k][li], F64) for k in ('z', 'mag', 'acc'))
        assert acc_d.shape == z64.shape == hact.shape == mag.shape, (li, acc_d.shape, z64.shape, hact.shape, mag.shape)
        w = {k: np.asarray(weights[n], F64) for k, n in (('bias', conv + '/bias'), ('gamma', bn + '/gamma'), ('beta', bn + '/beta'),
                                                         ('mean', bn + '/moving_mean'), ('var', bn + '/moving_variance'))}
        sd = np.sqrt(w['var'] + O.BN_EPS)
        ratio = np.abs(acc_d - acc64) / (U32 * np.maximum(mag, 1e-300))
        worst = tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), ratio.shape))
        measured = float(ratio[worst])
        print("head layer %d: max |acc_dev - acc64| / (u mag) = %.3f at %s (c_acc %g)" % (li + 1, measured, worst, c_acc[li]))
        assert measured <= c_acc[li], "head layer %d: acc at %s is %.9g, the oracle's %.9g: %.3f u mag, above c_acc = %g" % (
            li + 1, worst, acc_d[worst], acc64[worst], measured, c_acc[li])
        extra = np.abs(w['gamma']) * (np.abs(acc64) + np.abs(w['bias']) + np.abs(w['mean'])) / sd + np.abs(w['beta'])
        C, t = head_kinks(z64, mag, w['gamma'], sd, extra, c_acc[li])
        n_close = int(C.sum())
        print("head layer %d: |C| = %d (cap %d), largest t = %.3g" % (li + 1, n_close, cap, float(t.max())))
        assert n_close <= cap, "head layer %d: %d pre-activations within rounding of zero (cap %d): choose another image seed" % (li + 1, n_close, cap)
        m_dev = hact > 0
        differ = m_dev != (z64 > 0)
        outside = differ & ~C
        if outside.any():
            r, c = (int(v) for v in np.argwhere(outside)[0])
            z_dev = w['gamma'][c] * (acc_d[r, c] + w['bias'][c] - w['mean'][c]) / sd[c] + w['beta'][c]
            raise AssertionError("head layer %d: %d ReLU decision(s) differ outside the close set; first at (row %d, channel %d): oracle z = %.9g, "
                                 "device z (from its acc) = %.9g, device y = %.9g, t = %.3g" % (li + 1, int(outside.sum()), r, c, z64[r, c], z_dev,
                                                                                              float(hact[r, c]), t[r, c]))
        report["layer%d" % (li + 1)] = dict(close_set=n_close, acc_ratio=measured, c_acc=float(c_acc[li]), largest_t=float(t.max()),
                                            disagreements=[dict(row=int(r), channel=int(c), z64=float(z64[r, c]), t=float(t[r, c]))
                                                           for r, c in np.argwhere(differ)])
        masks.append(m_dev)
    return tuple(masks), report


# ---------------------------------------------------------------------------------------------------------------------------------
# RPN heads, proposals, RoI sample
# ---------------------------------------------------------------------------------------------------------------------------------

def _host(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def check_rpn_heads(plan, aux, A, tol=RPN_HEAD_TOL):
    """The device's fused RPN head outputs plan.rpn_heads (per level [B,h,w,head_channels]: 2A class logits, then 4A box deltas, then
    padding, which is ignored) against the oracle's aux['rpn_cls'] / aux['rpn_box'] ({level: [1,h,w,2A] / [1,h,w,4A]}), per level and
    per image (aux: one dict or a list per image).  Returns {(image, level, what): rel_err}."""
    auxes = [aux] if isinstance(aux, dict) else list(aux)
    errs = {}
    for i, hd in enumerate(plan.rpn_heads):
        hd = _host(hd)
        assert hd.shape[0] == len(auxes) and hd.shape[-1] >= 6 * A, (hd.shape, len(auxes), A)
        for b, a in enumerate(auxes):
            level = 2 + i
            for what, got, want in (("cls", hd[b, ..., :2 * A], a['rpn_cls'][level][0]), ("box", hd[b, ..., 2 * A:6 * A], a['rpn_box'][level][0])):
                assert got.shape == want.shape, (b, level, what, got.shape, want.shape)
                errs[(b, level, what)] = e = rel_err(got, want)
                assert e < tol, "RPN head of image %d, P%d, %s: rel_err %.3g (tolerance %g)" % (b, level, what, e, tol)
    return errs


def compare_proposals(props, order, keep, want_props, want_order, want_keep):
    """One image's ProposalLayer result (device arrays) against the float32 oracle's on the same scores and deltas, as
    tests/test_gpu_kernels.py::test_rpn_proposals_bit_exact_given_scores compares them: top-k order and NMS survivors exactly, box
    coordinates to the last bit of expf, zero padding behind the survivors."""
    np.testing.assert_array_equal(order, want_order)
    n = len(want_keep)
    np.testing.assert_array_equal(keep[:n], want_keep)
    assert np.all(keep[n:] == -1), "survivors beyond the oracle's %d" % n
    np.testing.assert_allclose(props, want_props, rtol=3e-7, atol=1e-7)
    assert np.all(props[n:] == 0), "proposals are not zero padded behind the %d survivors" % n


def check_proposals_from_device_scores(plan, anchors, cfg, B):
    """plan.proposals(debug=True) of the last forward: per image, O.proposal_layer on the device's OWN fp32 scores and head deltas must
    reproduce the device's order, survivors and boxes (compare_proposals).  anchors [A_total,4] pixels; cfg: dict with proposal_count
    (or count) and nms.  Returns the device's proposals [B,count,4].
    (Nothing in a train step writes the plan's head buffers -- the RPN backward reads them and writes gradient buffers of its own -- so
    this runs directly after forward_backward on that step's heads.)"""
    count = int(cfg.get('proposal_count', cfg.get('count')))
    props, (scores, order, keep) = plan.proposals(debug=True)
    props, scores, order, keep = (_host(t) for t in (props, scores, order, keep))
    heads = [_host(h) for h in plan.rpn_heads]
    A = len(plan.rpn["ratios"])
    assert props.shape == (B, count, 4) and scores.shape[0] == B
    box = np.concatenate([h[..., 2 * A:6 * A].reshape(B, -1, 4) for h in heads], axis=1)
    cls = np.concatenate([h[..., :2 * A].reshape(B, -1, 2) for h in heads], axis=1)
    assert np.abs(scores - O.softmax(cls)[:, :, 1]).max() < 1e-6
    anchors = np.asarray(anchors, np.float32)
    for b in range(B):
        want, ix, kp = O.proposal_layer(scores[b], box[b], anchors, (plan.H, plan.W), count, cfg['nms'])
        compare_proposals(props[b], order[b], keep[b], want, ix, kp)
    return props


def check_sample(tg, device_props, gt_caps, gt_boxes_px, H, W, cfg):
    """The step's RoI sample tg (model.last_targets) must be what DetectionTargetLayer selects from the device's own proposals and THIS
    image's ground truth: per image b, O.detection_targets(device_props[b], gt_caps[b], gt_norm[b], TRAIN_ROIS_PER_IMAGE,
    ROI_POSITIVE_RATIO, None) equals tg's rois, caps, npos, nneg exactly (the RoIs are copies of proposals; shuffle=None keeps proposal
    order).  gt_norm is computed in float32 as the model and the oracle do.  gt_caps [B,G,T], gt_boxes_px [B,G,4]."""
    device_props = np.asarray(device_props)
    B = device_props.shape[0]
    rois, caps = np.asarray(tg['rois']), np.asarray(tg['caps'])
    if rois.ndim == 2:
        rois, caps = rois[None], caps[None]
    npos, nneg = np.atleast_1d(tg['npos']), np.atleast_1d(tg['nneg'])
    gt_caps = np.asarray(gt_caps).reshape(B, -1, np.asarray(gt_caps).shape[-1])
    gt_norm = (np.asarray(gt_boxes_px, np.float32).reshape(B, -1, 4) / np.array([H, W, H, W], np.float32)).astype(np.float32)
    assert rois.shape[0] == B and len(npos) == B and len(nneg) == B
    for b in range(B):
        w_rois, w_caps, w_pos, w_neg = O.detection_targets(device_props[b], gt_caps[b], gt_norm[b], cfg.TRAIN_ROIS_PER_IMAGE, cfg.ROI_POSITIVE_RATIO, None)
        assert (int(npos[b]), int(nneg[b])) == (w_pos, w_neg), "image %d: the device sampled %d positive / %d negative RoIs, DetectionTargetLayer %d / %d" % (
            b, npos[b], nneg[b], w_pos, w_neg)
        if not np.array_equal(rois[b], w_rois):
            bad = np.nonzero((rois[b] != w_rois).any(axis=1))[0]
            raise AssertionError("image %d: %d sampled RoI row(s) differ from DetectionTargetLayer's on the device's proposals; first row %d: %s, want %s"
                                 % (b, len(bad), bad[0], rois[b][bad[0]], w_rois[bad[0]]))
        if not np.array_equal(caps[b], w_caps):
            bad = np.nonzero((caps[b] != w_caps).any(axis=1))[0]
            raise AssertionError("image %d: %d sampled target row(s) differ from the GT rows DetectionTargetLayer assigns; first row %d: %s, want %s"
                                 % (b, len(bad), bad[0], caps[b][bad[0]], w_caps[bad[0]]))


def assert_rois_are_proposals(rois, n, props):
    """Every one of the first n sampled RoIs is bit-equal to one of the proposals."""
    have = {r.tobytes() for r in np.ascontiguousarray(props, np.float32)}
    for i, r in enumerate(np.ascontiguousarray(rois, np.float32)[:n]):
        assert r.tobytes() in have, "sampled RoI %d %s is none of the device's proposals" % (i, r)


def device_head_buffers(top):
    """(acc0, acc1), (hact0, hact1) of a RoiHead top's last forward (model.caption_model), as host arrays."""
    bf = top._bufs
    return tuple(_host(bf['acc%d' % i]) for i in (0, 1)), tuple(_host(bf['hact%d' % i]) for i in (0, 1))


def check_step_decisions(model, tg, aux, oracle_cfg, gt_rows, gt_boxes_px):
    """The three cuts in front of the RoI head after a forward_backward of `model` (a joint or tag model): the RPN heads against the
    oracle's (aux: one dict, or a list per image), the proposals exactly from the device's own scores, and the sample tg exactly from
    those proposals and the step's own ground truth (gt_rows [B,G,*]: captions or tag rows).  Returns (device proposals, head errors)."""
    auxes = [aux] if isinstance(aux, dict) else list(aux)
    plan = model.plan()
    errs = check_rpn_heads(plan, auxes, len(oracle_cfg['ratios']))
    props = check_proposals_from_device_scores(plan, auxes[0]['anchors'], oracle_cfg, len(auxes))
    check_sample(tg, props, gt_rows, gt_boxes_px, plan.H, plan.W, model.config)
    return props, errs
