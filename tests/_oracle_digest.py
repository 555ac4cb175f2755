"""Digests of the float64 oracle's results on the small joint step, for the test that holds its default path (no rounding hook) to the
values it had before the hook existed (tests/golden/oracle_default_path_digests.json).  Per result array: its sum and the sum of its
absolute values (float64; compared at 1e-12, the room another BLAS's summation order needs)."""
import numpy as np

S, V, T, R, BLOCKS = 128, 24, 8, 16, 1


def _put(out, name, a):
    a = np.asarray(a, np.float64)
    out[name] = [float(a.sum()), float(np.abs(a).sum())]


def digests(M):
    """M: an oracle.np_models module.  joint step (stages 4+ trainable: every hooked function runs), the two-image batch step, v1 step."""
    from _joint_cases import joint_config, joint_inputs, joint_weights, oracle_cfg
    cfg, Wt, (img, _, match, tdelta, gt_caps, gt_boxes) = joint_config(S, V, T, R), joint_weights(V, BLOCKS), joint_inputs(S, V, T)
    out = {}
    losses, G, aux = M.joint_loss_and_grads(Wt, img[0], match[0, :, 0], tdelta[0], gt_caps[0], gt_boxes[0], oracle_cfg(cfg), stage4_blocks=BLOCKS,
                                            backbone_from=4)
    for k, v in losses.items():
        _put(out, "joint/loss/" + k, v)
    for k, v in G.items():
        _put(out, "joint/grad/" + k, v)
    _put(out, "joint/cap_probs", aux['cap_probs'])
    tg = ([aux['rois']] * 2, [aux['caps']] * 2)
    img2 = img[0][::-1].copy()
    losses, G, _ = M.joint_loss_and_grads_batch(Wt, [img[0], img2], [match[0]] * 2, [tdelta[0]] * 2, [gt_caps[0]] * 2, [gt_boxes[0]] * 2, oracle_cfg(cfg), tg,
                                                stage4_blocks=BLOCKS)
    for k, v in losses.items():
        _put(out, "batch/loss/" + k, v)
    for k, v in G.items():
        _put(out, "batch/grad/" + k, v)
    rng = np.random.default_rng(0)
    feat = rng.standard_normal((3, 7, 7, 256))
    caps = np.array([[1, 3, 4, 0, 0, 0, 0, 0], [1, 5, 6, 7, 8, 9, 2, 3], [0] * 8], float)
    loss, G, probs = M.v1_loss_and_grads(Wt, feat, caps)
    _put(out, "v1/loss", loss)
    _put(out, "v1/probs", probs)
    for k, v in G.items():
        _put(out, "v1/grad/" + k, v)
    return out
