"""Every cached form of a weight must follow a weight change (-m gpu).

One rule over a matrix of models, histories and events (tests/_coherence_cases.py): a model that has lived through a HISTORY -- which
creates the derived copies: encoder plans with their Winograd / chained-pointwise packs, folded BatchNorm operands and bf16 casts, the
bf16 shadow of the parameter bucket, folded heads, packed recurrent kernels, captured step graphs -- and then sees a weight-change
EVENT must give, bit for bit (torch.equal / np.array_equal, no tolerance), the OBSERVABLES of a fresh model of the same class that was
built on the resulting weights and never ran the history.  Both run the same kernels at the same shapes in the same order; call to
call, captured against eager and piped against serial the project already holds itself to bit equality.  The fresh model is the
reference: its own parity with the float64 oracle is the business of the model test files.

Events: e1 set_weights of a full dictionary drawn from other seeds; e2 set_weights of ONE tensor aimed at one derived form (x 1.5; a
bias, beta or moving mean + 0.5); e3 save_weights of a donor model and load_weights(path, by_name=True), once with exclude=; e4 three
optimizer steps, the fresh model given get_weights_dict() -- which also pins get_weights_dict -> set_weights as bit-exact on every
packed layout; e5 the stores rewritten in place and _weights_changed(), what ParallelModel.broadcast_weights does on every rank but
the first (a world of one broadcasts nothing, so the two calls are made directly).

The guard against a vacuous case: for every case a fresh model on the OLD weights gives float observables more than 1e-3 of their
largest magnitude away from the new ones (three orders above the fp32 rounding the parity tests allow); an observable upstream of
the changed tensor must not move at all.  Ids are compared between the aged and the fresh model, not guarded.

Training models take one FURTHER optimizer step in the comparison.  set_weights does not reset the optimizer (as in Keras) and the
detection-target stream goes on, so the fresh model starts that step from the aged model's optimizer state and stream positions
(_coherence_cases.adopt_training_state): what is compared is what the weights' copies contribute."""
import numpy as np
import pytest
import torch

import _coherence_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def donors(tmp_path_factory):
    """save_weights of a donor model on the other seeds' weights, once per kind: kind -> path."""
    root, made = tmp_path_factory.mktemp("donors"), {}

    def path(kind, make):
        if kind not in made:
            made[kind] = str(root / (kind + ".npz"))
            make().save_weights(made[kind])
        return made[kind]
    return path


def _loaded(path, W_old, exclude=()):
    """What load_weights(path, by_name=True, exclude=) leaves the model with: the file's arrays, the excluded layers' old ones."""
    from image_captioning_amd.modified_dense_model import load_weight_file
    W = dict(W_old)
    W.update({k: v for k, v in load_weight_file(path).items() if k in W_old and k.split("/")[0] not in exclude})
    return W


# ------------------------------------------------------------------------------------------------------------------------------------
# the joint model in training mode
# ------------------------------------------------------------------------------------------------------------------------------------
BN_GAMMA = "bn3a_branch2a/gamma"          # a frozen backbone BatchNorm: folded into the plan's epilogue vectors when the plan is built
LATERAL = "fpn_c4p4/kernel"               # a trainable kernel the plan reads in place from the bucket (bf16 model: re-cast inside every forward)


def _plan_tensor(model, which):
    """The single tensor(s) of an e2 event aimed at one of the plan's packs, read off the plan the history built."""
    p = model.plan()
    frozen = lambda n: n + "/kernel" in model._backbone
    if which == "wino":                    # a backbone 3x3 kernel with Cin, Cout % 32 == 0: it runs in the Winograd form
        names = [n for n in p._wwino if frozen(n)]
        assert names, "no frozen layer runs the Winograd kernel"
        return [names[0] + "/kernel"]
    if which == "chain":                   # a 2c kernel and the next block's 2a, one chained launch (at S = 128 the stage-2 seam; the
        names = list(p._wchain)            # stage-3 / 4 tile form needs 6144 pixels -- the same cache, dropped with the same plan)
        assert len(names) >= 2 and names[0].endswith("2c") and names[1].endswith("2a") and all(frozen(n) for n in names[:2]), names
        return [names[0] + "/kernel", names[1] + "/kernel"]
    names = [n for n in p._wb if frozen(n) and p._specs[n].k == 1]      # "cast": a backbone 1x1 kernel the bf16 plan rounded once
    assert names, "no frozen pointwise layer has a per-plan bf16 cast"
    return [names[0] + "/kernel"]


def _joint_event(event, aged, W_old, inputs, donors, dtype):
    """Runs the event on the aged model -> (the weights a fresh model is given, did a backbone tensor change)."""
    if event == "e1_full":
        W = K.joint_weights(1)
        aged.set_weights(W)
        return W, True
    if event.startswith("e2_"):
        keys = {"bn_gamma": [BN_GAMMA], "lateral": [LATERAL]}.get(event[3:]) or _plan_tensor(aged, event[3:])
        change = {k: K.bumped(k, W_old[k]) for k in keys}
        aged.set_weights(change)
        return dict(W_old, **change), all(k in aged._backbone for k in keys)
    if event.startswith("e3_"):
        path = donors("joint", lambda: K.joint_model(K.joint_weights(1)))      # (the file is the same whatever the donor computes in)
        exclude = ["fpn_c4p4", "imgcap_lstm1", "res3a_branch2a"] if event == "e3_load_exclude" else None
        aged.load_weights(path, by_name=True, exclude=exclude)
        return _loaded(path, W_old, exclude or ()), True
    if event == "e4_steps":
        for _ in range(3):
            aged.train_on_batch(inputs)
    else:
        assert event == "e5_in_place"
        aged.store.flat.mul_(1.25)
        aged.store.w["mrcnn_class_bn1/moving_variance"].mul_(1.5)             # (a frozen entry: broadcast one by one)
        aged._weights_changed()
    return aged.get_weights_dict(), False


# (the Winograd and chained-pointwise packs exist in f32 plans, the per-plan cast of a frozen kernel in bf16 plans)
JOINT_CASES = [("f32", e) for e in ("e1_full", "e2_bn_gamma", "e2_wino", "e2_chain", "e2_lateral", "e3_load", "e3_load_exclude", "e4_steps", "e5_in_place")]
JOINT_CASES += [("bf16", e) for e in ("e1_full", "e2_bn_gamma", "e2_cast", "e2_lateral", "e3_load", "e4_steps", "e5_in_place")]


def _joint_case(dtype, event, donors, layers=None, single=None):
    inputs = K.train_inputs()
    sample = K.fixed_sample(inputs)
    where = "joint %s %s%s" % (dtype, event, "" if layers is None else " " + layers)
    aged = K.joint_model(K.joint_weights(0), dtype=dtype, layers=layers)
    K.train_history(aged, inputs)
    plan, graphs = aged._plan, dict(aged._graphs)
    W_old = aged.get_weights_dict()
    if single is not None:                                        # (the trainable-stage case: one tensor of the bucket)
        change = {single: K.bumped(single, W_old[single])}
        aged.set_weights(change)
        W_new, backbone = dict(W_old, **change), False
    else:
        W_new, backbone = _joint_event(event, aged, W_old, inputs, donors, dtype)
    if backbone:                                                  # the plans pack the backbone and the step graph bakes the plan's buffers: both go
        assert aged._plan is None and aged._plans == [] and not aged._graphs, where
    else:                                                         # the bucket was written in place: the plan and the captured step stay
        assert aged._plan is plan and aged._graphs.keys() == graphs.keys() and all(aged._graphs[k] is g for k, g in graphs.items()), where
    if dtype == "bf16":
        assert not K.stale_shadow(aged.store), (where, K.stale_shadow(aged.store))
    fresh = K.joint_model(W_new, dtype=dtype, layers=layers)
    want = K.step_observables(fresh, inputs, sample)
    K.same(K.step_observables(aged, inputs, sample), want, where)
    # one further optimizer step: a replay of the surviving graph, or the first eager step behind a dropped one
    K.adopt_training_state(fresh, aged, lambda m: (m.compile(K.LR), setattr(m, "use_step_graph", True)))
    la, lf = aged.train_on_batch_device(inputs).clone(), fresh.train_on_batch_device(inputs).clone()
    if not backbone:
        assert [c.last for k, c in aged._steps.items() if k[0] == "train"] == ["replay"], where
    K.same(dict(step_losses=la, flat_after_step=aged.store.flat), dict(step_losses=lf, flat_after_step=fresh.store.flat), where + " further step")
    if dtype == "bf16":
        assert not K.stale_shadow(aged.store) and not K.stale_shadow(fresh.store), where
    old = K.old_observables(("joint", dtype, layers), lambda: K.step_observables(K.joint_model(W_old, dtype=dtype, layers=layers), inputs, sample))
    K.moved(old, want, ("losses", "flat_grad"), where)
    return aged, fresh


@pytest.mark.parametrize("dtype,event", JOINT_CASES, ids=["%s-%s" % c for c in JOINT_CASES])
def test_joint_training_follows_a_weight_event(gpu, donors, dtype, event):
    """History h2 (four train_on_batch calls: the step is captured on the third and replayed) on the joint model, f32 and bf16, then
    each event.  Observables: the loss terms and store.flat_grad of forward_backward on a fixed sample, the losses and store.flat
    after one further train step; bf16: the shadow equals torch's cast of the master weights after the event and after the step.
    The e2 tensors: a backbone bn gamma (plan-owned folded BN), a backbone 3x3 kernel (Winograd pack; f32 plans), a 2c / 2a pair
    (chained-pointwise pack; f32 plans), a backbone 1x1 kernel (per-plan bf16 cast; bf16 plans), fpn_c4p4/kernel (read in place).
    A backbone event drops the plans and the captured step; every other event keeps both and the further step is a replay."""
    _joint_case(dtype, event, donors)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_joint_trainable_stage_follows_a_weight_event(gpu, donors, dtype):
    """set_trainable("4+"): stages 4 and 5 live in the bucket, their BatchNorm is folded inside every forward and their kernels are
    read in place (bf16: re-cast inside every forward).  bn4b_branch2c/beta + 0.5 (the stage's last BatchNorm: all of C4 moves) is a write into the bucket: plan and captured step
    stay, and the fold, the backward through the stage and the further step follow the new value."""
    _joint_case(dtype, "e2_stage4_beta", donors, layers="4+", single="bn4b_branch2c/beta")


# ------------------------------------------------------------------------------------------------------------------------------------
# the joint model in inference mode
# ------------------------------------------------------------------------------------------------------------------------------------
def _infer_observables(model, img):
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    _, _, _, _, proposals, feats = DenseImageCapRCNN._proposal_features(model, [img], "host", False)
    out = dict(proposals=proposals.clone(), features=feats.clone())
    feat, cm = out["features"][0], model.caption_model
    probs, ids, scores = cm.generate(feat, return_probabilities=True)
    _, inc_ids, inc_scores = cm.generate(feat, return_probabilities=False, decoder="incremental")
    _, beam_ids, beam_scores = cm.generate(feat, return_probabilities=False, decoder="beam", beam_size=3, score="prob")     # (see K.v1_observables)
    out.update(probs=probs, ids=ids, word_scores=scores, greedy_ids=inc_ids, greedy_scores=inc_scores, beam_ids=beam_ids, beam_scores=beam_scores)
    return out


@pytest.mark.parametrize("event", ["e1_full", "e2_bn_gamma", "e2_wino", "e2_chain", "e2_recurrent", "e3_load"])
def test_joint_inference_follows_a_weight_event(gpu, donors, event):
    """Histories h1 and h3 (generate_captions twice, then the incremental and the beam decoder) on the inference plan, then the event.
    Observables: proposals, pooled features, the prefix decoder's word probabilities and ids, greedy and beam ids and scores.
    e2_recurrent -- imgcap_lstm1/recurrent_kernel, the decoders' packed recurrent kernel -- leaves the plan in place, and proposals
    and features must not move."""
    from image_captioning_amd import synth
    img = synth.images(7, 1, K.S, K.S)[0]
    where = "joint inference " + event
    aged = K.joint_model(K.joint_weights(0), mode="inference")
    for kw in ({}, {}, dict(return_probabilities=False, decoder="incremental"), dict(return_probabilities=False, decoder="beam", beam_size=3)):
        aged.generate_captions([img], **kw)
    plan = aged._plan
    assert plan is not None and plan._wwino and plan._wchain and "dec_upk1" in aged.caption_model._bufs
    W_old = aged.get_weights_dict()
    if event == "e2_recurrent":
        key = "imgcap_lstm1/recurrent_kernel"
        change = {key: K.bumped(key, W_old[key])}
        aged.set_weights(change)
        W_new, backbone = dict(W_old, **change), False
    else:
        W_new, backbone = _joint_event(event, aged, W_old, None, donors, "f32")
    assert (aged._plan is None and aged._plans == []) if backbone else aged._plan is plan, where
    want = _infer_observables(K.joint_model(W_new, mode="inference"), img)
    K.same(_infer_observables(aged, img), want, where)
    old = K.old_observables("joint inference", lambda: _infer_observables(K.joint_model(W_old, mode="inference"), img))
    floats = ("proposals", "features", "probs", "word_scores", "greedy_scores", "beam_scores")
    K.moved(old, want, floats[2:] if event == "e2_recurrent" else floats, where)


# ------------------------------------------------------------------------------------------------------------------------------------
# pipeline.JointTrainPipeline: the two alternating plans
# ------------------------------------------------------------------------------------------------------------------------------------
PIPE_KERNEL = "res2a_branch2b/kernel"


def _pipe_batches(n):
    from image_captioning_amd import synth
    from _joint_cases import joint_inputs
    batches = []
    for s in range(n):
        inp = joint_inputs(K.S, K.V, K.T, seed=8 + s)
        if s & 1:
            inp[0] = synth.images(20 + s, 1, K.S, K.S)
        batches.append(inp)
    return batches


def _piped_model():
    from image_captioning_amd.pipeline import JointTrainPipeline
    model = K.joint_model(K.joint_weights(0))
    model.compile(1e-5)
    return model, JointTrainPipeline(model)


def _piped(pipe, batches):
    """step() per batch and flush(): the batches' loss terms (each is copied at once: the next step reuses its buffer)."""
    losses = []
    for b in batches:
        l = pipe.step(b)
        if l is not None:
            losses.append(l.clone())
    return losses + [pipe.flush().clone()]


def test_pipeline_fetches_new_plans_after_a_backbone_change_between_batches(gpu):
    """History h4 (three piped steps and flush()), e2 on a backbone kernel, three more piped steps: the pipeline must run the new
    plans -- every loss term and every weight equals, bit for bit, a fresh model taken through the same six steps and the same
    set_weights serially.  Guard: without the change the last three batches' losses lie more than 1e-3 elsewhere."""
    batches = _pipe_batches(6)
    model, pipe = _piped_model()
    losses = _piped(pipe, batches[:3])
    assert len(model._plans) == 2 and pipe.pending is None
    before = list(model._plans)
    new = K.bumped(PIPE_KERNEL, model.get_weights_dict()[PIPE_KERNEL])
    model.set_weights({PIPE_KERNEL: new})
    losses += _piped(pipe, batches[3:])
    torch.cuda.synchronize()
    assert len(model._plans) == 2 and pipe.plans is model._plans and not any(p is q for p in model._plans for q in before)
    runs = {}
    for changed in (True, False):
        ref = K.joint_model(K.joint_weights(0))
        ref.compile(1e-5)
        ref.use_step_graph = False
        out = [ref.train_on_batch_device(b).clone() for b in batches[:3]]
        if changed:
            ref.set_weights({PIPE_KERNEL: new})
        out += [ref.train_on_batch_device(b).clone() for b in batches[3:]]
        runs[changed] = (torch.stack(out), ref.store.flat.clone())
    K.same(dict(losses=torch.stack(losses), flat=model.store.flat), dict(losses=runs[True][0], flat=runs[True][1]), "pipeline refresh")
    d = K.distance(runs[False][0][3:], runs[True][0][3:])
    print("  guard pipeline refresh: the last three batches' losses without the change: %.3e of the largest" % d)
    assert d > K.GUARD


def test_pipeline_refuses_a_backbone_change_while_a_batch_is_pending(gpu):
    """The pending batch's backbone pass ran on the old weights and the plan that holds its C2..C5 is gone from the model: step()
    and flush() raise a RuntimeError that says to flush() first; a change of non-backbone weights in the same place is fine."""
    batches = _pipe_batches(3)
    model, pipe = _piped_model()
    pipe.step(batches[0])
    model.set_weights({LATERAL: K.bumped(LATERAL, model.get_weights_dict()[LATERAL])})
    assert pipe.step(batches[1]) is not None and pipe.pending is not None
    model.set_weights({PIPE_KERNEL: K.bumped(PIPE_KERNEL, model.get_weights_dict()[PIPE_KERNEL])})
    for call in (lambda: pipe.step(batches[2]), pipe.flush):
        with pytest.raises(RuntimeError, match=r"flush\(\) before changing backbone weights"):
            call()
    torch.cuda.synchronize()


def test_pipeline_close_gives_the_model_back_its_step_graph(gpu):
    """The constructor pins use_step_graph off for the pipeline's alternating plans; close() restores what it found -- the automatic
    choice of an unpinned model, the pinned graph of another -- and the first plan.  After close() four train_on_batch calls capture
    and replay a graph again, and the weights equal, bit for bit, those of a model that never had a pipeline."""
    from image_captioning_amd.pipeline import JointTrainPipeline
    batches, base = _pipe_batches(3), K.train_inputs()
    model = K.joint_model(K.joint_weights(0))
    model.compile(1e-5)
    found = (model._path.use_graph, model._path.auto)
    pipe = JointTrainPipeline(model)
    assert not model.use_step_graph and not model._path.auto
    pipe.close()
    assert (model._path.use_graph, model._path.auto) == found
    model.use_step_graph = True
    pipe = JointTrainPipeline(model)
    for b in batches:
        pipe.step(b)
    assert pipe.pending is not None
    last = pipe.close()                                            # (flushes the pending batch first)
    assert last is not None and pipe.pending is None and model.use_step_graph and model._plan is model._plans[0]
    ref = K.joint_model(K.joint_weights(0))
    ref.compile(1e-5)
    ref.use_step_graph = False
    for b in batches:
        ref.train_on_batch_device(b)
    ref.use_step_graph = True
    for m in (model, ref):
        for _ in range(4):
            m.train_on_batch(base)
        assert [c.last for k, c in m._steps.items() if k[0] == "train"] == ["replay"]
    assert model.optimizer.iterations == ref.optimizer.iterations == 7
    K.same(dict(flat=model.store.flat), dict(flat=ref.store.flat), "after close()")


# ------------------------------------------------------------------------------------------------------------------------------------
# Mask R-CNN and the RoI tag model: what their tops derive
# ------------------------------------------------------------------------------------------------------------------------------------
MASK_BETA = "mrcnn_mask_bn2/beta"
DETECT_FLOATS = ("scores", "logits", "deltas", "class_masks")


def _detect_case(event, donors):
    from image_captioning_amd import synth
    img = synth.images(7, 1, 96, K.S)[0]
    where = "maskrcnn " + event
    aged = K.detect_model(K.detect_weights(0))
    for _ in range(2):
        assert len(aged.detect([img])[0]["class_ids"]) > 0, "no detection: the mask head did not run"
    top = aged.caption_model
    assert top._folded is not None and aged._plan is not None
    W_old = aged.get_weights_dict()
    new = K.bumped(MASK_BETA, W_old[MASK_BETA])
    moves = ("class_masks",)
    if event == "model_set_weights":
        aged.set_weights({MASK_BETA: new})
    elif event == "top_load_weights":
        top.load_weights({MASK_BETA: new})
    elif event == "weights_changed_in_place":
        top.store.w[MASK_BETA].add_(0.5)
        aged._weights_changed()
    elif event == "e1_full":
        aged.set_weights(K.detect_weights(1))
        moves = DETECT_FLOATS
    else:
        assert event == "e3_load_exclude"
        path = donors("maskrcnn", lambda: K.detect_model(K.detect_weights(1)))
        aged.load_weights(path, by_name=True, exclude=["mrcnn_mask_bn1"])
        moves = DETECT_FLOATS
    W_new = aged.get_weights_dict()
    if event in ("model_set_weights", "top_load_weights", "weights_changed_in_place"):
        assert np.array_equal(W_new[MASK_BETA], new) and all(np.array_equal(W_new[k], W_old[k]) for k in W_old if k != MASK_BETA)
    elif event == "e3_load_exclude":
        assert np.array_equal(W_new["mrcnn_mask_bn1/beta"], W_old["mrcnn_mask_bn1/beta"]) and not np.array_equal(W_new[MASK_BETA], W_old[MASK_BETA])
    want = K.detect_observables(K.detect_model(W_new), img)
    K.same(K.detect_observables(aged, img), want, where)
    old = K.old_observables("maskrcnn", lambda: K.detect_observables(K.detect_model(W_old), img))
    K.moved(old, want, moves, where)


@pytest.mark.parametrize("event", ["model_set_weights", "top_load_weights", "weights_changed_in_place", "e1_full", "e3_load_exclude"])
def test_maskrcnn_folded_mask_head_follows_every_way_its_weights_change(gpu, donors, event):
    """DetectTop folds the four mask BatchNorms once per set of weights (_folded).  History h1 (detect() twice, with detections),
    then mrcnn_mask_bn2/beta + 0.5 through the model's set_weights, through load_weights on the top, and written in place followed by
    the model's _weights_changed() (a broadcast) -- and e1 / e3 through the model.  Observables: detect()'s rois, class ids, scores
    and masks, the head's logits and deltas and the class masks as floats; the single tensor moves the class masks alone."""
    _detect_case(event, donors)


@pytest.mark.parametrize("event", ["e1_full", "e2_head_variance", "e4_steps"])
def test_roitag_model_follows_a_weight_event(gpu, event):
    """ROITagRCNN's top derives nothing of its own (its head reads BatchNorm's four vectors in the kernel), its plan what the joint
    model's does.  History: two eager train steps; e2: mrcnn_class_bn2/moving_variance, a frozen entry of the top's store."""
    inputs = K.tag_inputs()
    sample = K.fixed_sample(inputs, caps=inputs[4][0, :3])
    where = "roitag " + event
    aged = K.tag_model(K.tag_weights(0))
    K.train_history(aged, inputs, steps=2, graph=False)
    W_old = aged.get_weights_dict()
    if event == "e1_full":
        aged.set_weights(K.tag_weights(1))
    elif event == "e2_head_variance":
        key = "mrcnn_class_bn2/moving_variance"
        aged.set_weights({key: K.bumped(key, W_old[key])})
    else:
        for _ in range(3):
            aged.train_on_batch(inputs)
    W_new = aged.get_weights_dict()
    assert (aged._plan is None) == (event == "e1_full")
    fresh = K.tag_model(W_new)
    want = K.step_observables(fresh, inputs, sample)
    K.same(K.step_observables(aged, inputs, sample), want, where)
    K.adopt_training_state(fresh, aged, lambda m: m.compile(K.LR))
    la, lf = aged.train_on_batch_device(inputs).clone(), fresh.train_on_batch_device(inputs).clone()
    K.same(dict(step_losses=la, flat_after_step=aged.store.flat), dict(step_losses=lf, flat_after_step=fresh.store.flat), where + " further step")
    old = K.old_observables("roitag", lambda: K.step_observables(K.tag_model(W_old), inputs, sample))
    K.moved(old, want, ("losses", "flat_grad"), where)


# ------------------------------------------------------------------------------------------------------------------------------------
# the feature extractor: plans keyed by shape
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("event", ["e1_full", "e2_stem", "e3_load_exclude"])
def test_feature_extractor_rebuilds_the_plans_of_both_shapes(gpu, tmp_path, event):
    """modified_dense_model.DenseImageCapRCNN keeps one plan per (batch, h, w).  History h1: extract_features at two shapes, twice;
    the event must drop both plans (e2: conv1/kernel, the stem's own packed layout)."""
    from image_captioning_amd.modified_dense_model import save_weight_file
    where = "extractor " + event
    aged = K.extractor_model(K.extractor_weights(0))
    for _ in range(2):
        K.extractor_observables(aged)
    assert set(aged._plans) == set(K.EXTRACTOR_SHAPES)
    W_old = dict(aged._weights)
    if event == "e1_full":
        W_new = K.extractor_weights(1)
        aged.set_weights(W_new)
    elif event == "e2_stem":
        W_new = dict(W_old, **{"conv1/kernel": K.bumped("conv1/kernel", W_old["conv1/kernel"])})
        aged.set_weights(W_new)
    else:
        path = str(tmp_path / "donor.npz")
        save_weight_file(path, K.extractor_weights(1))
        aged.load_weights(path, by_name=True, exclude=["conv1", "bn_conv1"])
        W_new = _loaded(path, W_old, ("conv1", "bn_conv1"))
    assert aged._plans == {}
    want = K.extractor_observables(K.extractor_model(W_new))
    K.same(K.extractor_observables(aged), want, where)
    assert set(aged._plans) == set(K.EXTRACTOR_SHAPES)
    old = K.old_observables("extractor", lambda: K.extractor_observables(K.extractor_model(W_old)))
    K.moved(old, want, tuple(want), where)


# ------------------------------------------------------------------------------------------------------------------------------------
# the decoders
# ------------------------------------------------------------------------------------------------------------------------------------
def _decoder_case(where, event, make, W1, batch, observe, e2_keys, in_place, donors, floats, upstream=()):
    """The decoders' common case: histories h1 / h2 / h3 (predict twice, four train steps with the captured step, greedy and beam
    decode), the event, the observables, one further train step."""
    feat, words, targets = batch
    aged = make()
    aged.use_step_graph = True
    observe(aged)
    for _ in range(4):
        aged.train_on_batch([feat, words], targets)
    observe(aged)
    assert any(cs.graph is not None for cs in aged._steps.values()), "the history captured no step"
    W_old = aged.get_weights_dict()
    if event == "e1_full":
        aged.load_weights(W1)
    elif event.startswith("e2_"):
        aged.load_weights({k: K.bumped(k, W_old[k]) for k in e2_keys[event]})
    elif event == "e3_load":
        aged.load_weights(donors(where.split()[0], lambda: make(W1)), by_name=True)
    elif event == "e4_steps":
        for _ in range(3):
            aged.train_on_batch([feat, words], targets)
    else:
        assert event == "e5_in_place"
        in_place(aged)
        aged._weights_changed()
    W_new = aged.get_weights_dict()
    if aged.store.flat_bf16 is not None:
        assert not K.stale_shadow(aged.store), where
    fresh = make(W_new)
    fresh.use_step_graph = True
    want = observe(fresh)
    K.same(observe(aged), want, where)
    K.adopt_training_state(fresh, aged, lambda m: None)
    la, lf = aged.train_on_batch_device([feat, words], targets).clone(), fresh.train_on_batch_device([feat, words], targets).clone()
    K.same(dict(step_loss=la, flat_after_step=aged.store.flat), dict(step_loss=lf, flat_after_step=fresh.store.flat), where + " further step")
    if aged.store.flat_bf16 is not None:
        assert not K.stale_shadow(aged.store), where
    old = K.old_observables(where.split()[0], lambda: observe(make(W_old)))
    K.moved(old, want, tuple(f for f in floats if f not in upstream), where)
    return aged, fresh


DECODER_EVENTS = ["e1_full", "e2_head_variance", "e2_recurrent", "e3_load", "e4_steps", "e5_in_place"]
DECODER_FLOATS = ("probs", "greedy_scores", "beam_scores")


@pytest.mark.parametrize("event", DECODER_EVENTS)
def test_v2_decoder_follows_a_weight_event(gpu, donors, event):
    """CaptionModelV2 folds its frozen head on the host into NEW tensors (_head: captured steps hold the old ones) and packs the word
    LSTM's recurrent kernel once per decode call.  e2: mrcnn_class_bn1/moving_variance (the fold), lstm_1/recurrent_kernel (the pack)."""
    from image_captioning_amd.layers import V2_WORD_LSTM

    def in_place(m):
        m.store.flat.mul_(1.25)
        m.store.w["mrcnn_class_bn1/moving_variance"].mul_(1.5)
    _decoder_case("v2 " + event, event, lambda W=None: K.v2_model(K.v2_weights(0) if W is None else W), K.v2_weights(1), K.v2_batch(), K.v2_observables,
                  {"e2_head_variance": ["mrcnn_class_bn1/moving_variance"], "e2_recurrent": [V2_WORD_LSTM + "/recurrent_kernel"]}, in_place, donors,
                  DECODER_FLOATS)


V1_CASES = [("f32", "e2_recurrent"), ("f32", "e4_steps")] + [("bf16", e) for e in ("e1_full", "e2_recurrent", "e2_vocabulary", "e4_steps", "e5_in_place")]


@pytest.mark.parametrize("dtype,event", V1_CASES, ids=["%s-%s" % c for c in V1_CASES])
def test_v1_decoder_follows_a_weight_event(gpu, donors, dtype, event):
    """CaptionModelV1 packs both LSTMs' recurrent kernels once per decode call (Upk); the bf16 model decodes the vocabulary layer from
    the bucket shadow.  e2: imgcap_lstm1/recurrent_kernel (the pack), imgcap_lstm_d2/kernel (the shadow as the decoders read it)."""
    def in_place(m):
        m.store.flat.mul_(1.25)
        m.store.w["mrcnn_class_bn1/moving_variance"].mul_(1.5)
    _decoder_case("v1_%s %s" % (dtype, event), event, lambda W=None: K.v1_model(K.v1_weights(0) if W is None else W, dtype), K.v1_weights(1), K.v1_batch(),
                  K.v1_observables, {"e2_recurrent": ["imgcap_lstm1/recurrent_kernel"], "e2_vocabulary": ["imgcap_lstm_d2/kernel"]}, in_place, donors,
                  DECODER_FLOATS)


@pytest.mark.parametrize("event", ["e1_full", "e2_recurrent", "e3_load", "e4_steps", "e5_in_place"])
def test_whole_image_captioner_follows_a_weight_event_and_keeps_its_padding_zero(gpu, donors, event):
    """WholeImageCaptioner holds its 40-unit merged LSTM as 64 units: the entries under padding_mask(name) stay exactly 0 after every
    event and after the further train step.  e2: merged_model_lstm/recurrent_kernel, padded in rows and gate columns."""
    aged, fresh = _decoder_case("whole_image " + event, event, lambda W=None: K.whole_image_model(K.whole_image_weights(0) if W is None else W),
                                K.whole_image_weights(1), K.whole_image_batch(), K.whole_image_observables,
                                {"e2_recurrent": ["merged_model_lstm/recurrent_kernel"]}, lambda m: m.store.flat.mul_(1.25), donors,
                                ("probs", "beam_scores"))
    assert not K.padding_is_zero(aged) and not K.padding_is_zero(fresh)


def test_store_assign_refreshes_the_shadow_of_a_mirrored_weight(gpu):
    """ParamStore.assign on its own (refresh=True) re-casts the shadow when the weight is mirrored, and only then."""
    model = K.v1_model(K.v1_weights(0), "bf16")
    st = model.store
    key = "imgcap_lstm_d1/kernel"
    assert key in st.wb and K.stale_shadow(st) == []
    st.assign(key, K.bumped(key, K.v1_weights(0)[key]))
    assert K.stale_shadow(st) == []
    st.assign(key, K.v1_weights(0)[key], refresh=False)
    assert K.stale_shadow(st) == [key]
    st.refresh_shadow()
    assert K.stale_shadow(st) == []
