"""The instrument of the bf16 step parity tests shown working, without a GPU (tests/_bf16_sites.py; the oracle's `quant` hook).

The device is stood in for by the rounding oracle itself evaluated with float32 products (BS.Float32StandIn) at the GPU tests' size
(128 px, one stage-4 block, V = 24, T = 8, 16 RoIs, compute_dtype='bf16').  Against the float64 rounding oracle, given the stand-in's
RoI sample, ReLU masks and operand roundings exactly as the GPU tests hand over the device's, that is the FLOOR of the comparison:
fp32 accumulation order.  The same for the step with bf16 storage and trainable stages, and for the inference forward behind its cut.  Then six errors are planted in
the stand-in, one at a time: each must fail the new comparison at the GPU test's own tolerances (BS.TOL_STEP) -- and pass the old one
(losses 1e-2, gradients 5e-2 against the oracle that never rounds), which is the gap this file writes down.  DESIGN.md section 3d
holds the figures."""
import types

import numpy as np
import pytest

from oracle import np_models as M

import _bf16_sites as BS
from _joint_cases import joint_config, joint_inputs, joint_weights, oracle_cfg

S, V, T, R, BLOCKS = 128, 24, 8, 16, 1
OLD_TOL = dict(losses=1e-2, grads=5e-2)              # test_joint_model_bf16_step_tracks_the_fp32_oracle's comparison with the unrounded oracle
OLD_TOL_STORAGE = dict(losses=1e-2, grads=1.5e-1)    # test_joint_model_trains_resnet_stages_in_bf16's


def make_case(T=T, long_captions=False, backbone_from=None, conv_bf16=False):
    """The GPU tests' step in one of their modes; long_captions (with T = 24): every ground-truth caption fills its positions (the sample
    then carries 69 live tokens instead of six, so that one token more or less is a 1.4 % error -- one the old comparison lets through)."""
    cfg, Wt, inputs = joint_config(S, V, T, R), joint_weights(V, BLOCKS), joint_inputs(S, V, T)
    img, _, match, tdelta, gt_caps, gt_boxes = inputs
    if long_captions:
        from image_captioning_amd import synth
        gt_caps = gt_caps.copy()
        gt_caps[0, :3] = synth.captions_v1(9, 3, T, V, lmin=T - 2, lmax=T - 2)
    d = BS.dims(S, V, T, R, BLOCKS, backbone_from=backbone_from, conv_bf16=conv_bf16)
    sites = BS.planned_sites(d)
    caches = {}                                       # the frozen trunk once per arithmetic (float64 / float32 products): it is the same in every run

    def step(quant, tg=None, masks=None):
        kind = None if quant is None else type(quant).__name__
        return M.joint_loss_and_grads(Wt, img[0], match[0, :, 0], tdelta[0], gt_caps[0], gt_boxes[0], oracle_cfg(cfg), stage4_blocks=BLOCKS,
                                      targets_override=tg, head_masks=masks, quant=quant, backbone_from=backbone_from,
                                      trunk_cache=caches.setdefault(kind, {}))
    plain = step(None)
    c = types.SimpleNamespace(Wt=Wt, cfg=cfg, d=d, sites=sites, step=step, plain=plain, tg=(plain[2]['rois'], plain[2]['caps']), caches=caches,
                              tol=BS.TOL_TRUNK_STEP if conv_bf16 else BS.TOL_STEP, old=OLD_TOL_STORAGE if conv_bf16 else OLD_TOL)
    return c


@pytest.fixture(scope="module")
def case():
    c = make_case()
    c.clean = evaluate(c)
    return c


def evaluate(c, post=None, materialise=False, **planted):
    """One stand-in step (with the planted error) and the float64 rounding oracle of it, given what the GPU tests hand over.
    post(losses, G): a planted error applied to the stand-in's results.  Returns the new comparison's figures, the hand-over
    violations and the old comparison's figures."""
    on = BS.bf16_set(c.sites) - set(planted.pop("off_pipe", ()))
    unrounded = set(planted.pop("unrounded", ())) | {(s, r) for s in BS.bf16_set(c.sites) - on for r in ("x", "w", "dy")}
    standin = BS.Float32StandIn(BS.bf16_set(c.sites), known=c.sites, materialise=materialise, unrounded=unrounded, **planted)
    losses, G, aux = c.step(standin, c.tg)
    losses, G = dict(losses), dict(G)
    if post is not None:
        post(losses, G)
    policy = BS.Bf16Policy(BS.bf16_set(c.sites), known=c.sites, materialise=materialise, given=standin.made)       # every operand copy, by name
    want, Gq, _ = c.step(policy, c.tg, tuple(z > 0 for z in aux['head_z']))
    return _figures(c, losses, G, want, Gq, policy)


def _figures(c, losses, G, want, Gq, policy):
    return types.SimpleNamespace(errs=BS.compare(G, Gq), lerrs=BS.loss_errs(losses, want), violations=policy.handed_violations(), policy=policy,
                                 old=BS.compare(G, c.plain[1]), old_l=BS.loss_errs(losses, c.plain[0]), losses=losses, G=G, want=want, Gq=Gq, c=c)


def replant(r, post):
    """A planted error that touches the stand-in's RESULTS only: the clean run's figures again, with post(losses, G) applied."""
    losses, G = dict(r.losses), dict(r.G)
    post(losses, G)
    return _figures(r.c, losses, G, r.want, r.Gq, r.policy)


def new_comparison_fails(r):
    return bool(r.violations) or bool(BS.failures(r.errs, r.c.tol)) or max(r.lerrs.values()) >= r.c.tol['losses']


def old_comparison_passes(r):
    return max(r.old.values()) < r.c.old['grads'] and max(r.old_l.values()) < r.c.old['losses']


def test_site_set_at_the_test_size_is_the_set_at_configs4_size(case):
    """No site of the reduced step falls back to the fp32 pipe that configs[4]'s own size puts on the bf16 pipe, in the three modes the GPU
    tests run: head / decoder / vocabulary alone, + bf16 storage with stages 4+ trainable, + everything trainable."""
    for kw in (dict(), dict(backbone_from=4, conv_bf16=True), dict(backbone_from=1, conv_bf16=True)):
        d = BS.dims(S, V, T, R, BLOCKS, **kw)
        small, full = BS.planned_sites(d), BS.planned_sites(BS.configs4_dims(d))
        assert set(small) == set(full) and BS.bf16_set(small) == BS.bf16_set(full), kw
    on = BS.bf16_set(case.sites)
    assert len(on) == 38 and sum(1 for s in on if case.sites[s].kind == "gemm") == 24 and "imgcap_lstm_d2:fwd" in on
    # ... and a size that does not fit is seen: an odd RoI count takes the per-RoI products of the decoder off the bf16 pipe
    odd = BS.bf16_set(BS.planned_sites(BS.dims(S, V, T, 15, BLOCKS)))
    assert {"imgcap_lstm1.feat:wgrad", "imgcap_lstm_d1.feat:wgrad", "mrcnn_class_conv1:wgrad"} <= on - odd


def test_default_path_gives_what_it_gave_before_the_hook():
    """quant=None: the joint step (stages 4+ trainable, so every hooked function runs), the two-image batch step and the v1 step give
    what the code before the hook gave -- tests/golden/oracle_default_path_digests.json was written by that code (tests/_oracle_digest.py:
    sum and sum of magnitudes of every loss, gradient and probability tensor).  Compared at 1e-12 of the tensor's magnitude sum: with
    the BLAS thread count held equal the results are equal byte for byte, another thread count reorders sums by 4e-16."""
    import json
    import os
    import _oracle_digest
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_default_path_digests.json")))
    got = _oracle_digest.digests(M)
    assert set(got) == set(want)
    for k, (s_, m_) in want.items():
        assert abs(got[k][0] - s_) <= 1e-12 * max(m_, 1e-300) and abs(got[k][1] - m_) <= 1e-12 * max(m_, 1e-300), (k, got[k], want[k])


def test_identity_hook_is_the_same_function(case):
    """An identity hook takes the single-pass decoder and the hooked convolutions: the same function to float64 rounding."""
    ident = case.step(lambda site, role, arr: arr)
    for k, v in case.plain[1].items():
        assert np.abs(ident[1][k] - v).max() <= 1e-11 * np.abs(v).max(), k
    rng = np.random.default_rng(0)
    feat = rng.standard_normal((3, 7, 7, 256))
    caps = np.array([[1, 3, 4, 0, 0, 0, 0, 0], [1, 5, 6, 7, 8, 9, 2, 3], [0] * 8], float)
    p0, c0 = M.v1_training_forward(case.Wt, feat, caps)
    p1, c1 = M.v1_training_forward(case.Wt, feat, caps, quant=lambda site, role, arr: arr)
    assert np.abs(p0 - p1).max() < 1e-13
    dlog = rng.standard_normal(p0.shape) / 24
    g0, g1 = M.v1_backward_from_dlogits(case.Wt, c0, dlog), M.v1_backward_from_dlogits(case.Wt, c1, dlog)
    assert set(g0) == set(g1)
    for k in g0:
        assert np.abs(g0[k] - g1[k]).max() <= 1e-11 * max(1e-300, np.abs(g0[k]).max()), k


def test_policy_counts_the_rounded_products_and_refuses_unknown_sites(case):
    p = case.clean.policy
    assert sorted(p.rounded_products()) == sorted(BS.bf16_set(case.sites)) and p.seen == set(case.sites)
    with pytest.raises(KeyError):
        p("imgcap_lstm3:fwd", "x", np.zeros(3))
    q = BS.Bf16Policy({"a:fwd"})
    x = np.array([1.0 + 2.0 ** -9, 3.0])
    assert q("a:fwd", "x", x)[0] in (1.0, 1.0 + 2.0 ** -7) and q("b:fwd", "x", x) is x and q.rounded_products() == []
    q("a:fwd", "w", x)
    assert q.rounded_products() == ["a:fwd"]


def test_floor_of_the_comparison(case):
    """The clean stand-in against the rounding oracle: the floor, per tensor group, far below the tolerances; nothing handed over is
    refused, and only a handful of entries were rounded to the other neighbour."""
    r = case.clean
    floor = BS.worst_per_group(r.errs)
    print("floor per group:", {g: "%.3g" % v for g, v in floor.items()}, "losses %.3g" % max(r.lerrs.values()))
    assert not r.violations
    flips = sum(h["flips"] for h in r.policy.handed.values())
    assert 0 < flips < 1e-3 * sum(h["size"] for h in r.policy.handed.values())
    assert not new_comparison_fails(r) and old_comparison_passes(r)
    for g, v in floor.items():
        assert v < 0.5 * BS.TOL_STEP[g], (g, v)
    assert max(r.lerrs.values()) < 0.5 * BS.TOL_STEP['losses']
    # without the hand-over the same comparison sits at the size of the rounding step: the flips feed on themselves
    bare = BS.Bf16Policy(BS.bf16_set(case.sites), known=case.sites)
    bare_G = case.step(bare, case.tg)[1]
    drift = BS.worst_per_group(BS.compare(r.G, bare_G))
    print("without the hand-over:", {g: "%.3g" % v for g, v in drift.items()})
    assert min(drift.values()) > 100 * max(floor["head"], floor["decoder"])


def _scaled(key, factor):
    def post(losses, G):
        G[key] = G[key] * factor
    return post


def _no_l2(c, key):
    def post(losses, G):
        G[key] = G[key] - 2.0 * c.cfg.WEIGHT_DECAY * np.asarray(c.Wt[key], np.float64) / np.asarray(c.Wt[key]).size
    return post


@pytest.mark.parametrize("name", ["a_scaled_gradient", "b_dropped_l2", "c_head_site_on_fp32_pipe", "c_fpn_site_on_fp32_pipe", "d_wgrad_reads_unrounded_x",
                                  "e_loss_from_unrounded_logits", "f_token_count_off_by_one"])
def test_planted_error_fails_the_new_comparison_and_passes_the_old(case, name):
    c = make_case(T=24, long_captions=True) if name.startswith("f_") else case
    cnt = float((M.v1_targets(c.tg[1]) > 0).sum())
    if name == "a_scaled_gradient":                     # one gradient tensor x 1.02 (a wrong grad_scale, a 1 / count off by a token in fifty)
        r, touched = replant(c.clean, _scaled('imgcap_lstm2/kernel', 1.02)), ['imgcap_lstm2/kernel']
    elif name == "b_dropped_l2":                        # (a bias: WEIGHT_DECAY w / size(w) is 6e-5 of this gradient; of a kernel's it is 1e-10, below fp32)
        r, touched = replant(c.clean, _no_l2(c, 'imgcap_lstm1/bias')), ['imgcap_lstm1/bias']
    elif name == "c_head_site_on_fp32_pipe":            # a silent fallback: fp32 product where the plan says bf16
        r, touched = evaluate(c, off_pipe=['mrcnn_class_conv2:fwd']), ['mrcnn_class_conv2/kernel']
    elif name == "c_fpn_site_on_fp32_pipe":
        r, touched = evaluate(c, off_pipe=['fpn_p3:wgrad']), ['fpn_p3/kernel']
    elif name == "d_wgrad_reads_unrounded_x":           # the weight gradient reads the activation before its rounding, the gradient after
        r, touched = evaluate(c, unrounded=[('imgcap_lstm2:wgrad', 'x')]), ['imgcap_lstm2/kernel']
    elif name == "e_loss_from_unrounded_logits":        # materialised logits: the gradient comes from the rounded ones, the loss does not
        clean_losses = dict(c.clean.losses)

        def post(losses, G):
            losses.update(clean_losses)
        r, touched = evaluate(c, post=post, materialise=True), []
    else:                                               # the caption loss's mean runs over one token too many
        assert cnt >= 60, cnt
        f = cnt / (cnt + 1.0)
        r, touched = evaluate(c, scale_dy={'imgcap_lstm_d2:wgrad': f, 'imgcap_lstm_d2:dgrad': f}), ['imgcap_lstm_d2/kernel', 'imgcap_lstm1/kernel']
    figures = {k: r.errs[k] for k in touched}
    if name.startswith("e_"):
        figures = {'imgcap_loss': r.lerrs['imgcap_loss']}
    print("planted", name, {k: "%.3g" % v for k, v in figures.items()}, "hand-over violations: %d" % len(r.violations),
          "old: grads %.3g losses %.3g" % (max(r.old.values()), max(r.old_l.values())))
    assert new_comparison_fails(r), name
    assert old_comparison_passes(r), name
    # Condition on the tolerances: below half of what the planted error does to the tensor it touches
    for k, v in figures.items():
        tol = BS.TOL_STEP['losses'] if k.endswith('_loss') else BS.TOL_STEP[BS.group_of(k)]
        assert tol < 0.5 * v, (name, k, v, tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16 storage between the convolutions, every stage trainable (the mode of test_joint_model_trains_resnet_stages_in_bf16[all])
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def storage_case():
    c = make_case(backbone_from=1, conv_bf16=True)
    c.clean = evaluate(c)
    return c


def test_floor_with_bf16_storage_and_trainable_stages(storage_case):
    r = storage_case.clean
    floor = BS.worst_per_group(r.errs)
    print("floor per group, bf16 storage:", {g: "%.3g" % v for g, v in floor.items()}, "losses %.3g" % max(r.lerrs.values()))
    assert not r.violations and not new_comparison_fails(r) and old_comparison_passes(r)
    assert set(floor) == set(BS.GROUPS) and all(v < 0.5 * BS.TOL_TRUNK_STEP[g] for g, v in floor.items()), floor


@pytest.mark.parametrize("name", ["a_scaled_trunk_gradient", "c_trunk_forward_site_on_fp32_pipe", "c_trunk_dgrad_site_on_fp32_pipe"])
def test_planted_error_in_the_trunk_fails_the_new_comparison_and_passes_the_old(storage_case, name):
    c = storage_case
    if name == "a_scaled_trunk_gradient":
        r, touched = replant(c.clean, _scaled('res4b_branch2b/kernel', 1.02)), ['res4b_branch2b/kernel']
    elif name == "c_trunk_forward_site_on_fp32_pipe":
        r, touched = evaluate(c, off_pipe=['res5b_branch2b:fwd']), ['res5b_branch2b/kernel']
    else:
        r, touched = evaluate(c, off_pipe=['res5b_branch2b:dgrad']), ['res5b_branch2a/kernel']
    figures = {k: r.errs[k] for k in touched}
    print("planted", name, {k: "%.3g" % v for k, v in figures.items()}, "hand-over violations: %d" % len(r.violations),
          "old: grads %.3g losses %.3g" % (max(r.old.values()), max(r.old_l.values())))
    assert new_comparison_fails(r) and old_comparison_passes(r), name
    for k, v in figures.items():
        assert BS.TOL_TRUNK_STEP[BS.group_of(k)] < 0.5 * v, (name, k, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# the inference forward behind the cut at the pyramid (test_joint_model_inference_in_bf16): head + teacher-forced decoder
# ---------------------------------------------------------------------------------------------------------------------------------

def _forward(case, policy, feats, caps):
    f, _ = M.roi_head_forward(feats, case.Wt, quant=policy)
    return M.v1_single_pass_forward(case.Wt, f, caps, policy)[0]


@pytest.mark.parametrize("planted", [None, ("imgcap_lstm2:fwd", "x"), ("mrcnn_class_conv2:fwd", "w")])
def test_inference_forward_bound_sees_an_unrounded_operand(case, planted):
    """Log-probabilities of head + decoder on given features: the float32 stand-in against the float64 rounding oracle with the
    stand-in's operand roundings handed over.  Clean: far below BS.TOL_INFERENCE['logprobs'].  One operand of one product read
    unrounded: at least twice the bound (a handed-over copy that is no rounding is refused besides)."""
    sites = BS.inference_sites(BS.dims(S, V, 5, 40, BLOCKS, conv_bf16=True))
    rng = np.random.default_rng(5)
    feats = 3.0 * np.abs(rng.standard_normal((40, 7, 7, 256)))
    caps = np.concatenate([np.ones((40, 1)), rng.integers(3, V, (40, 4)).astype(np.float64)], axis=1)
    standin = BS.Float32StandIn(BS.bf16_set(sites), known=sites, unrounded=[planted] if planted else ())
    got = _forward(case, standin, feats, caps)
    policy = BS.Bf16Policy(BS.bf16_set(sites), known=sites, given=standin.made)
    want = _forward(case, policy, feats, caps)
    err = float(np.abs(np.log(np.maximum(got.astype(np.float64), 1e-30)) - np.log(np.maximum(want, 1e-30))).max())
    print("inference forward, planted %s: log-probabilities %.3g, refused copies %d" % (planted, err, len(policy.handed_violations())))
    if planted is None:
        assert not policy.handed_violations() and err < 0.5 * BS.TOL_INFERENCE['logprobs'], err
    else:
        assert err > 2 * BS.TOL_INFERENCE['logprobs'], err
