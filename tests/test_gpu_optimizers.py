"""dc_optimizer_step_f32 (Keras' Adam without amsgrad, SGD with momentum / nesterov / neither) and the models that train through it
(-m gpu), against the float64 restatement of tests/_optimizer_ref.py.  Tolerances are those of test_gpu_kernels.py's
test_amsgrad_trajectory: 1e-6 of the parameter scale on p, 1e-5 on the state."""
import numpy as np
import pytest
import torch

from image_captioning_amd._lib import DcapError

import _optimizer_ref as R
from _joint_cases import joint_inputs, make_joint

pytestmark = pytest.mark.gpu

POISON = 0x7FC0DEAD                          # a quiet NaN with a payload: no arithmetic produces these bits
GUARD = 64                                   # guard elements on either side (256 bytes: the carved buffer stays 16-byte aligned)

# variant -> (ops kind, restatement kind, state buckets, launch keywords, restatement keywords)
VARIANTS = {
    "adam": ("adam", "adam", 2, dict(), dict(lr=1e-3)),
    "sgd_momentum": ("sgd", "sgd", 1, dict(beta1=0.9), dict(lr=0.01, momentum=0.9)),
    "sgd_nesterov": ("sgd", "sgd", 1, dict(beta1=0.9, nesterov=True), dict(lr=0.01, momentum=0.9, nesterov=True)),
    "sgd_plain": ("sgd", "sgd", 0, dict(beta1=0.0), dict(lr=0.01)),
}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def close(got, want, tol):
    got = (got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)).astype(np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max()) / scale
    assert err < tol, "max err %.3e (scaled) exceeds %.1e" % (err, tol)


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy().copy()


def guarded(n, fill=None, dtype=torch.float32):
    """-> (whole buffer, the n-element view inside it): GUARD poisoned elements on either side of the view."""
    if dtype == torch.float32:
        whole = torch.full((n + 2 * GUARD,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    else:
        whole = torch.full((n + 2 * GUARD,), 0x7FC1, dtype=torch.int16, device="cuda").view(dtype)
    view = whole[GUARD:GUARD + n]
    if fill is not None:
        view.copy_(dev(fill, dtype))
    return whole, view


def guards_intact(whole, n):
    b = bits(whole)
    want = POISON if whole.element_size() == 4 else 0x7FC1
    return bool((b[:GUARD] == want).all() and (b[GUARD + n:] == want).all())


def step_of(variant, t, decay=0.0):
    """The host's step word of update t, as params computes it: Python floats, rounded once."""
    kw = VARIANTS[variant][4]
    return float(np.float32(R.adam_word(t, lr=kw["lr"], decay=decay) if variant == "adam" else R.lr_decayed(kw["lr"], decay, t)))


# ---- trajectories ---------------------------------------------------------------------------------------------------------------------
# 10 007: a vector part and a tail of 3;  3: no vector part at all;  2 098 179 = 2048 * 256 * 4 + 1027: the grid is capped at 2048
# blocks of 256 threads, so the grid-stride loop makes a second pass (of 256 vectors) and the bucket still ends in a tail of 3
@pytest.mark.parametrize("n,steps", [(10007, 5), (3, 5), (2098179, 1)])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_trajectory_matches_the_restatement(ops, variant, n, steps):
    kind, ref_kind, n_state, launch_kw, ref_kw = VARIANTS[variant]
    for clipnorm in (None, 0.5):
        for clipvalue in (None, 0.05):
            for grad_scale in (1.0, 0.5):
                rng = np.random.default_rng(8)
                p0 = rng.standard_normal(n).astype(np.float32)
                p = dev(p0)
                state = [torch.zeros(n, device="cuda") for _ in range(n_state)]
                ref = R.Trajectory(ref_kind, p0, clipnorm=clipnorm, clipvalue=clipvalue, **ref_kw)
                for t in range(1, steps + 1):
                    g = (rng.standard_normal(n) * (0.3 ** t)).astype(np.float32)
                    ref.step(g, grad_scale)
                    gd = dev(g)
                    ops.optimizer_step(kind, p, gd, state, step_of(variant, t), grad_scale=grad_scale, gnorm_sq=ops.sumsq(gd) if clipnorm else None,
                                       clipnorm=clipnorm or 0.0, clipvalue=clipvalue or 0.0, **launch_kw)
                what = (variant, n, clipnorm, clipvalue, grad_scale)
                assert not np.array_equal(p.cpu().numpy(), p0), what
                try:
                    close(p, ref.p, 1e-6)
                    for got, want in zip(state, ref.state):
                        close(got, want, 1e-5)
                except AssertionError as e:
                    raise AssertionError("%s: %s" % (what, e))


# ---- the regulariser inside the update ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_segments_regulariser_and_mask_inside_the_update(ops, variant):
    """dc_reg_sumsq_f32 + dc_optimizer_step_f32(reg=segments) against g' = g mask + 2 coef p -> global clip -> update.  The table of
    test_amsgrad_with_the_regulariser_inside_the_update: segments end inside float4 vectors (6 + 12 + 2 elements), two are frozen,
    every third has a zero coefficient, the bucket length is no multiple of 4."""
    kind, ref_kind, n_state, launch_kw, ref_kw = VARIANTS[variant]
    rng = np.random.default_rng(9)
    bounds = [0, 6, 18, 20, 1021, 1024, 5000, 5003, 9001, 10007]
    n = bounds[-1]
    coef = np.zeros(n, np.float32)
    mask = np.ones(n, np.float32)
    for s_, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        coef[lo:hi] = 0.0 if s_ % 3 == 2 else 1e-4 / (hi - lo)
        mask[lo:hi] = 0.0 if s_ in (3, 6) else 1.0
    coef[bounds[3]:bounds[4]] = 0.0                                       # a frozen segment carries no regulariser either (_masks())
    coef[bounds[6]:bounds[7]] = 0.0
    frozen = mask == 0.0
    for use_mask in (True, False):
        mk = mask if use_mask else None
        segs = ops.RegSegmentTable(coef, mk, "cuda")
        assert segs.nseg <= len(bounds) - 1 and segs.n == n
        p0 = rng.standard_normal(n).astype(np.float32)
        p = dev(p0)
        state = [torch.zeros(n, device="cuda") for _ in range(n_state)]
        ref = R.Trajectory(ref_kind, p0, clipnorm=0.5, **ref_kw)
        gn = torch.zeros(1, device="cuda")
        for t in range(1, 5):
            g = (rng.standard_normal(n) * (0.5 ** t)).astype(np.float32)
            gr = R.regularised(g, ref.p, coef, mk)
            ref.step(gr)
            gd = dev(g)
            keep = bits(gd)
            ops.reg_sumsq(p, gd, segs, gnorm_sq=gn)
            assert abs(float(gn.item()) - float((gr * gr).sum())) < 1e-5 * float((gr * gr).sum())
            ops.optimizer_step(kind, p, gd, state, step_of(variant, t), gnorm_sq=gn, clipnorm=0.5, reg=segs, **launch_kw)
            assert np.array_equal(bits(gd), keep), "the gradient bucket was written"
        close(p, ref.p, 1e-6)
        for got, want in zip(state, ref.state):
            close(got, want, 1e-5)
        if use_mask:
            assert np.array_equal(bits(p)[frozen], p0.view(np.int32)[frozen]), "frozen parameters moved"
            assert not np.array_equal(bits(p)[~frozen], p0.view(np.int32)[~frozen])
            for s in state:
                assert not bits(s)[frozen].any(), "the state of frozen parameters was touched"


# ---- each kind touches only its own streams -------------------------------------------------------------------------------------------
def test_adam_has_no_third_state_stream(ops):
    from image_captioning_amd import _lib
    fields = [f for f, _ in _lib.OptimizerDesc._fields_]
    assert "vhat" not in fields and [f for f in fields if f.startswith("state")] == ["state0", "state1"]
    n = 1027
    p, g = dev(np.ones(n)), dev(np.ones(n))
    three = [torch.zeros(n, device="cuda") for _ in range(3)]
    with pytest.raises(DcapError, match="at most two state buckets"):
        ops.optimizer_step("adam", p, g, three, 1e-3)
    assert float(p.min()) == 1.0


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_only_the_kinds_own_buffers_are_written(ops, variant):
    """Poisoned guard elements around p, g and every state bucket stay as they were; g is never written; plain SGD writes p alone."""
    kind, ref_kind, n_state, launch_kw, ref_kw = VARIANTS[variant]
    n = 4099                                                              # 1024 vectors + a tail of 3
    rng = np.random.default_rng(12)
    p0, g0 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    pw, p = guarded(n, p0)
    gw, g = guarded(n, g0)
    states = [guarded(n, np.zeros(n)) for _ in range(n_state)]
    ops.optimizer_step(kind, p, g, [s for _, s in states], step_of(variant, 1), **launch_kw)
    torch.cuda.synchronize()
    assert guards_intact(pw, n) and guards_intact(gw, n) and all(guards_intact(w, n) for w, _ in states)
    assert np.array_equal(bits(g), g0.view(np.int32))
    ref = R.Trajectory(ref_kind, p0, **ref_kw)
    ref.step(g0)
    close(p, ref.p, 1e-6)
    assert (bits(p) != p0.view(np.int32)).mean() > 0.99
    for (_, s), want in zip(states, ref.state):
        close(s, want, 1e-5)
        assert bits(s).any()


# ---- bf16 shadow ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_bf16_shadow_is_refreshed_in_the_same_pass(ops, variant):
    kind, _, n_state, launch_kw, _ = VARIANTS[variant]
    n, n_bf16 = 10007, 5000
    rng = np.random.default_rng(13)
    p, g = dev(rng.standard_normal(n)), dev(rng.standard_normal(n))
    state = [torch.zeros(n, device="cuda") for _ in range(n_state)]
    whole, shadow = guarded(n_bf16, dtype=torch.bfloat16)
    shadow.view(torch.int16).fill_(0x7FC1)                               # stale everywhere
    ops.optimizer_step(kind, p, g, state, step_of(variant, 1), p_bf16=shadow, **launch_kw)
    torch.cuda.synchronize()
    assert np.array_equal(bits(shadow), bits(p[:n_bf16].to(torch.bfloat16)))
    assert guards_intact(whole, n_bf16), "the shadow was written past n_bf16"
    with pytest.raises(DcapError, match="bf16 shadow"):                  # the shadow rule: a multiple of 4 inside the vectorised part
        ops.optimizer_step(kind, p, g, state, step_of(variant, 1), p_bf16=shadow[:4998], **launch_kw)


# ---- the step word from device memory -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_device_step_word_overrides_the_argument(ops, variant):
    kind, _, n_state, launch_kw, _ = VARIANTS[variant]
    n = 10007
    rng = np.random.default_rng(14)
    p0, g = rng.standard_normal(n), dev(rng.standard_normal(n))
    step = step_of(variant, 3)
    out = []
    for from_device in (False, True):
        p = dev(p0)
        state = [torch.zeros(n, device="cuda") for _ in range(n_state)]
        if from_device:
            ops.optimizer_step(kind, p, g, state, 123.0, step_dev=dev(np.array([step], np.float32)), **launch_kw)
        else:
            ops.optimizer_step(kind, p, g, state, step, **launch_kw)
        out.append([bits(p)] + [bits(s) for s in state])
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert not np.array_equal(out[0][0], dev(p0).view(torch.int32).cpu().numpy())


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ops):
    n = 1024
    rng = np.random.default_rng(15)
    p0 = rng.standard_normal(n + 4).astype(np.float32)
    big = {k: dev(p0) for k in ("p", "g", "m", "v")}
    ok = {k: t[:n] for k, t in big.items()}
    for moved in ("p", "g", "m", "v"):                                    # a buffer 4 bytes off a 16-byte boundary
        a = dict(ok, **{moved: big[moved][1:n + 1]})
        with pytest.raises(DcapError, match=r"code -?\d+\): dc_optimizer_step: buffers must be 16-byte aligned") as e:
            ops.optimizer_step("adam", a["p"], a["g"], [a["m"], a["v"]], 1e-3)
        from image_captioning_amd import _lib
        assert "(code %d)" % _lib.EALIGN in str(e.value)
    with pytest.raises(DcapError, match="Adam needs both moment buffers") as e:
        ops.optimizer_step("adam", ok["p"], ok["g"], [ok["m"]], 1e-3)
    assert "(code %d)" % _lib.EINVAL in str(e.value)
    with pytest.raises(DcapError, match="SGD with momentum needs its velocity buffer") as e:
        ops.optimizer_step("sgd", ok["p"], ok["g"], [], 1e-2, beta1=0.9)
    assert "(code %d)" % _lib.EINVAL in str(e.value)
    coef = np.full(100, 1e-4, np.float32)
    segs = ops.RegSegmentTable(coef, None, "cuda")                        # a table for another bucket size: refused in the wrapper
    with pytest.raises(DcapError, match="the segment table covers 100 elements, the bucket has 1024"):
        ops.optimizer_step("adam", ok["p"], ok["g"], [ok["m"], ok["v"]], 1e-3, reg=segs)
    with pytest.raises(DcapError, match="kind must be one of"):
        ops.optimizer_step("rmsprop", ok["p"], ok["g"], [], 1e-3)
    torch.cuda.synchronize()
    for t in big.values():
        assert np.array_equal(bits(t), p0.view(np.int32)), "a refused call wrote something"


# ---- the decoders ---------------------------------------------------------------------------------------------------------------------
def _v2(seed=0):
    from image_captioning_amd import synth
    from image_captioning_amd.text_generation_model_v2 import DenseCapConfig, build_model, SampleTables
    V, Tw, Rn = 1000, 6, 5
    cfg = DenseCapConfig(V, synth.embedding_matrix(seed + 3, V))
    cfg.PADDING_SIZE = Tw
    model = build_model((7, 7, 256), (Tw,), cfg, 256, True, seed=seed)
    model.use_step_graph = True                                           # (opt-in for this model)
    rng = np.random.default_rng(1)
    feat_r = rng.standard_normal((Rn, 7, 7, 256)).astype(np.float32)
    caps = synth.captions_v2(2, Rn, Tw + 2, V, full=False, lmin=1)
    from oracle import np_models as M                                     # (sample expansion only: the reference's batch layout)
    roi, words, tgt = M.v2_expand_samples(caps, Tw)
    feat = feat_r[roi]
    batch = ([feat, words], np.eye(V)[tgt])

    def gradient(m):
        tb = SampleTables.from_samples(np.asarray(words), np.asarray(tgt, np.int32), m.device)
        m._forward_train(m._dev_feat(feat), tb, want_grad=True)
        m._backward()
    return model, batch, gradient


def _v1(seed=0):
    from image_captioning_amd import synth
    from image_captioning_amd.text_generation_model import DenseCapConfig, build_lstm_model, caption_targets
    V, T, B = 40, 6, 4
    cfg = DenseCapConfig(V, synth.embedding_matrix(seed + 3, V), B)
    cfg.PADDING_SIZE = T
    model = build_lstm_model([7, 7, 256], cfg, 512, 'training', seed=seed)
    model.recurrent_dropout = 0.0                                         # a deterministic step: both models see the same graph
    rng = np.random.default_rng(21)
    feat = rng.standard_normal((B, 7, 7, 256)).astype(np.float32)
    caps = synth.captions_v1(22, B, T, V, lmin=1, lmax=3)
    batch = ([feat, caps], caption_targets(caps, V))

    def gradient(m):
        m._forward_train(m._dev_feat(feat), caps, caption_targets(caps), want_grad=True)
        m._backward()
    return model, batch, gradient


def _optimizers():
    from image_captioning_amd.params import Adam, SGD
    return {"adam": (lambda: Adam(), "adam", dict(lr=1e-3)),
            "sgd": (lambda: SGD(momentum=0.9, nesterov=True, decay=1e-2), "sgd", dict(lr=0.01, momentum=0.9, nesterov=True, decay=1e-2))}


@pytest.mark.parametrize("which", ["adam", "sgd"])
@pytest.mark.parametrize("make", [_v1, _v2], ids=["v1", "v2"])
def test_decoders_train_through_the_new_optimizers(ops, monkeypatch, make, which):
    """Two models from one seed.  B: five train_on_batch calls (two eager, the capture, two replays -- three graph launches with a
    changing step word).  A: before each of them it is given B's weights, runs _forward_train + _backward, and its gradient bucket goes
    to the restatement on the host, whose float64 state runs freely over the five steps; B's weights after the step and its state
    agree with the restatement's to the trajectory tolerance.  (A free-running pair of weight trajectories would also measure how the
    loss surface amplifies a last-bit difference between two sets of weights, which is no property of the update.)
    B with DCAP_STEP_GRAPH=0 equals B bit for bit."""
    new_opt, ref_kind, ref_kw = _optimizers()[which]
    a, _, gradient = make()
    runs = {}
    for graph in (True, False):
        monkeypatch.setenv("DCAP_STEP_GRAPH", "1" if graph else "0")
        b, (inputs, targets), _ = make()
        start = b.store.flat.cpu().numpy().copy()
        b.compile(optimizer=new_opt())
        ref = R.Trajectory(ref_kind, start, **ref_kw)
        seq = []
        for step in range(5):
            if graph:
                a.store.flat.copy_(b.store.flat)
                a._weights_changed()
                gradient(a)
                ref.p = b.store.flat.cpu().numpy().astype(np.float64)
                ref.step(a.store.flat_grad.cpu().numpy())
            b.train_on_batch(inputs, targets)
            seq.append(next(iter(b._steps.values())).last if b._steps else "eager")
            if graph:
                try:
                    close(b.store.flat, ref.p, 1e-6)
                    for got, want in zip(b.optimizer._state, ref.state):
                        close(got, want, 1e-5)
                except AssertionError as e:
                    raise AssertionError("step %d (%s): %s" % (step + 1, seq[-1], e))
        assert seq == (["eager", "eager", "capture", "replay", "replay"] if graph else ["eager"] * 5), seq
        assert b.optimizer.iterations == 5 and len(b.optimizer._state) == len(ref.state)
        runs[graph] = b.store.flat.cpu().numpy().copy()
        assert not np.array_equal(runs[graph], start)
    np.testing.assert_array_equal(runs[True], runs[False])


def test_compile_takes_the_keras_strings(ops):
    from image_captioning_amd import params
    m, (inputs, targets), _ = _v2()
    m.compile(optimizer="adam", loss="categorical_crossentropy")
    assert isinstance(m.optimizer, params.Adam) and not m.optimizer.amsgrad
    before = m.store.flat.clone()
    m.train_on_batch(inputs, targets)
    assert len(m.optimizer._state) == 2 and not torch.equal(before, m.store.flat)
    m.compile(optimizer="sgd")
    assert isinstance(m.optimizer, params.SGD)
    m.train_on_batch(inputs, targets)
    assert m.optimizer._state == ()


# ---- the joint model ------------------------------------------------------------------------------------------------------------------
def test_joint_model_trains_with_sgd_through_the_fused_regulariser(ops, monkeypatch):
    """compile(lr, optimizer=SGD(momentum=0.9, clipnorm=5.0)) on the small joint case: three train_on_batch steps (the third one
    captured and replayed), every step against the restatement.  A twin model is given the trained model's weights before each step
    (bit-equal weights draw the same RoI sample; the restatement's float64 velocity runs freely) and its forward_backward leaves g mask + 2 coef p in its gradient bucket -- the unfused
    regulariser pass --, which the host clips by its global norm and applies; the trained model takes the fused path (reg_sumsq +
    optimizer_step(reg=segments)).  Frozen elements (per _masks()) do not move.  Eager and captured runs are bit-equal."""
    from image_captioning_amd.params import SGD
    S, V, T = 128, 24, 5
    lr = 1e-3
    inputs = joint_inputs(S, V, T)
    inputs[0] = torch.tensor(inputs[0], device="cuda")
    twin, _, _ = make_joint(S, V, T, 1)
    runs = {}
    for mode in ("graph", "eager"):
        model, _, _ = make_joint(S, V, T, 1)
        opt = SGD(momentum=0.9, clipnorm=5.0)
        model.compile(lr, optimizer=opt)
        assert model.optimizer is opt and opt.lr == lr and model.caption_model.optimizer is opt
        model.use_step_graph = mode == "graph"
        called = []
        for name in ("reg_sumsq", "sumsq", "l2_reg", "amsgrad_step", "optimizer_step"):
            monkeypatch.setattr(ops, name, (lambda f, nm: lambda *a, **k: (called.append(nm), f(*a, **k))[1])(getattr(ops, name), name))
        vel = None
        for step in range(3):
            if mode == "graph":                                           # the host restatement of THIS step, from the twin's gradient
                before = model.store.flat.clone()
                twin.store.flat.copy_(before)
                twin._weights_changed()
                twin._dt_step = model._dt_step                            # the same detection-target stream position
                twin.forward_backward(inputs)
                _, mask = twin._masks()
                g = R.clipped(twin.store.flat_grad.cpu().numpy(), clipnorm=5.0)
                vel = np.zeros_like(g) if vel is None else vel
                want_p, vel = R.sgd_step(before.cpu().numpy().astype(np.float64), g, vel, step + 1, lr=lr, momentum=0.9)
            model.train_on_batch(inputs)
            if mode == "graph":
                close(model.store.flat, want_p, 1e-6)
                close(opt._state[0], vel, 1e-5)
                assert not torch.equal(model.store.flat, before)
                if mask is not None:
                    fz = (mask == 0).cpu().numpy()
                    assert np.array_equal(bits(model.store.flat)[fz], bits(before)[fz])
        monkeypatch.undo()
        if mode == "graph":
            assert any(k[0] == "train" for k in model._graphs), "the step was not captured"
        else:
            assert called == ["reg_sumsq", "optimizer_step"] * 3, called
        assert opt.iterations == 3
        runs[mode] = model.store.flat.cpu().numpy().copy()
    np.testing.assert_array_equal(runs["graph"], runs["eager"])


def test_joint_default_compile_keeps_the_amsgrad_launches(ops, monkeypatch):
    from image_captioning_amd.params import Adam
    S, V, T = 128, 24, 5
    model, _, _ = make_joint(S, V, T, 1)
    model.compile(1e-4)
    opt = model.optimizer
    assert isinstance(opt, Adam) and opt.amsgrad and opt.clipnorm == 0.5 and opt.lr == 1e-4 and opt.clipvalue is None
    model.use_step_graph = False
    called = []
    for name in ("reg_sumsq", "sumsq", "l2_reg", "amsgrad_step", "optimizer_step"):
        monkeypatch.setattr(ops, name, (lambda f, nm: lambda *a, **k: (called.append(nm), f(*a, **k))[1])(getattr(ops, name), name))
    model.train_on_batch(joint_inputs(S, V, T))
    assert called == ["reg_sumsq", "amsgrad_step"], called
    assert len(opt._state) == 3
