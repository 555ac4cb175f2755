"""The segment table of the fused optimizer passes on grids that make more than one pass (-m gpu): dc_reg_sumsq_f32,
dc_optimizer_step_f32(reg=) and dc_amsgrad_step_f32(reg=) against the exact restatements of tests/_reg_segment_cases.py, and
dc_l2_reg_f32's gradient write on 25 grid passes.

The cases (tests/test_reg_segment_cases.py proves what they reach): "big", 3 * 2^21 + 3111 elements under a full table of 1024
segments -- 249 992 vectors take the cursor's fast path, 799 361 search again after a stale cursor, segments end on every lane of a
vector and one starts inside the scalar tail --; "one", 4 * 2^21 + 1 elements under a single segment; "small", the 10 007-element table
of test_gpu_optimizers.py.  Coefficients are from {0, 1/4, 1/2, 3/4, 1} and the data dyadic, so SGD's results, Adam's moments and the
sparse sums are compared bit for bit: a neighbouring segment's coefficient on a single element fails them."""
import types

import numpy as np
import pytest
import torch

from image_captioning_amd._lib import DcapError

import _reg_segment_cases as RS

pytestmark = pytest.mark.gpu

POISON = 0x7FC0DEAD                          # a quiet NaN with a payload: no arithmetic produces these bits
GUARD = 64                                   # guard elements on either side (the carved buffer stays 16-byte aligned)

SGD_VARIANTS = {"plain": dict(beta1=0.0), "momentum": dict(beta1=RS.B1), "nesterov": dict(beta1=RS.B1, nesterov=True)}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy().copy()


def f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


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


_TABLES = {}


def table(ops, name, use_mask=True):
    """The case's ops.RegSegmentTable, built once from the per-element vectors as the model builds its own."""
    key = (name, use_mask)
    if key not in _TABLES:
        case = RS.build(name)
        segs = ops.RegSegmentTable(case.coef, case.mask if use_mask and case.nseg > 1 else None, "cuda")
        if use_mask:
            assert segs.nseg == case.nseg and np.array_equal(segs.start.cpu().numpy(), case.start)
            assert np.array_equal(segs.coef.cpu().numpy(), case.seg_coef) and np.array_equal(segs.mask.cpu().numpy(), case.seg_mask)
        assert 1 <= segs.nseg <= case.nseg and segs.n == case.n
        _TABLES[key] = segs
    return _TABLES[key]


def test_the_library_launches_the_grid_the_walk_model_assumes(ops):
    """dc_reg_sumsq_workspace_bytes(n) is two float partials per block of reg_sumsq_kernel's grid: the library's grid is the one
    the CPU model of the walk (test_reg_segment_cases.py) uses.  dc_amsgrad_step_f32 and dc_optimizer_step_f32 compute their grids by
    the same expression in source (csrc/loss.hip) but expose no such figure."""
    from image_captioning_amd import _lib
    lib = _lib.load()
    for name in ("big", "one", "small"):
        case = RS.build(name)
        assert int(lib.dc_reg_sumsq_workspace_bytes(case.n)) == 2 * 4 * case.grid, name
    assert RS.build("big").grid == RS.build("one").grid == 2048 and RS.build("small").grid == 11
    assert int(lib.dc_l2_reg_workspace_bytes(RS.build("big").n)) == 4 * RS.l2_reg_blocks(RS.build("big").n) == 4 * 1024


# ---- SGD: exact -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(SGD_VARIANTS))
@pytest.mark.parametrize("name", ["big", "one", "small"])
def test_sgd_with_the_table_is_exact_over_two_steps(ops, name, variant):
    """optimizer_step("sgd", reg=table): p and the velocity equal the restatement bit for bit after one step and after a second one
    from the first step's state, at grad_scale 1 without and 1/2 with a value clip; frozen elements and their velocity keep their
    bits; g is not written; the guard words around p, g and the velocity stay poisoned."""
    case, d, segs = RS.build(name), RS.dense_data(name), table(ops, name)
    n, frozen = case.n, case.mask == 0
    kw = SGD_VARIANTS[variant]
    for cfg_name, cfg in sorted(RS.CONFIGS.items()):
        pw, p = guarded(n, d["p"])
        buffers = [(pw, n)]
        state, vel_ref = [], None
        if variant != "plain":
            vw, vel = guarded(n, d["vel"])
            buffers.append((vw, n))
            state, vel_ref = [vel], d["vel"]
        p_ref = d["p"]
        for step, key in enumerate(("g", "g2")):
            gw, g = guarded(n, d[key])
            ops.optimizer_step("sgd", p, g, state, RS.STEP, reg=segs, **kw, **cfg)
            torch.cuda.synchronize()
            p_ref, vel_ref = RS.sgd_exact(p_ref, d[key], vel_ref, case.coef, case.mask, nesterov=kw.get("nesterov", False), **cfg)
            what = (name, variant, cfg_name, "step %d" % (step + 1))
            diff = np.flatnonzero(bits(p) != f32_bits(p_ref))
            assert len(diff) == 0, "%s: p differs on %d elements, first at %s" % (what, len(diff), diff[:8])
            if state:
                diff = np.flatnonzero(bits(state[0]) != f32_bits(vel_ref))
                assert len(diff) == 0, "%s: the velocity differs on %d elements, first at %s" % (what, len(diff), diff[:8])
            assert np.array_equal(bits(g), f32_bits(d[key])), "%s: the gradient bucket was written" % (what,)
            assert guards_intact(gw, n) and all(guards_intact(w, k) for w, k in buffers), what
        assert (bits(p) != f32_bits(d["p"]))[~frozen].mean() > 0.5           # (two clipped steps of opposite sign cancel)
        if frozen.any():
            assert np.array_equal(bits(p)[frozen], f32_bits(d["p"])[frozen]), "frozen parameters moved"
            assert not state or not bits(state[0])[frozen].any(), "the velocity of frozen parameters was touched"


# ---- Adam and AMSGrad: exact moments, a derived bound on p ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adam", "amsgrad"])
@pytest.mark.parametrize("name", ["big", "small"])
def test_adam_and_amsgrad_with_the_table(ops, name, kind):
    """m, v (and vhat) are dyadic and compared bit for bit.  p is held to |p - p_exact| <= K 2^-24 (|p| + |update|) per element with
    K = 10, derived in _reg_segment_cases.py from the kernel's chain p - step m / (sqrtf(v) + eps): sqrtf 1 ulp (2 units of 2^-24),
    the sum 1, the division 2.5 ulp (5), the difference 1 on |p| + |update|, and one for the second-order terms; p_exact is float64
    arithmetic on the exact moments.  The neighbouring segment's coefficient on one element misses this bound by a factor above 1000
    (test_reg_segment_cases.py).  Measured worst error / bound (printed): 0.201 for Adam, 0.195 for AMSGrad.
    The bf16 shadow over a prefix that covers A's end equals p.to(bfloat16) and is not written past its length."""
    case, d, segs = RS.build(name), RS.dense_data(name), table(ops, name)
    n, frozen = case.n, case.mask == 0
    n_bf16 = int(case.start[case.named["A"] + 1]) + 1 + 4096 if name == "big" else 5000
    assert n_bf16 % 4 == 0
    configs = RS.CONFIGS if kind == "adam" else {"plain": dict(grad_scale=1.0), "scaled": dict(grad_scale=0.5)}
    for cfg_name, cfg in sorted(configs.items()):
        buf = {key: guarded(n, d[key]) for key in ("p", "g", "m", "v") + (("vhat",) if kind == "amsgrad" else ())}
        sw, shadow = guarded(n_bf16, dtype=torch.bfloat16)
        p, g = buf["p"][1], buf["g"][1]
        if kind == "adam":
            ops.optimizer_step("adam", p, g, [buf["m"][1], buf["v"][1]], RS.STEP, beta1=RS.B1, beta2=RS.B2, eps=RS.EPS, p_bf16=shadow, reg=segs,
                               **cfg)
        else:
            ops.amsgrad_step(p, g, buf["m"][1], buf["v"][1], buf["vhat"][1], RS.STEP, beta1=RS.B1, beta2=RS.B2, eps=RS.EPS, p_bf16=shadow,
                             reg=segs, **cfg)
        torch.cuda.synchronize()
        p_ref, m_ref, v_ref, vhat_ref, upd = RS.adam_exact(d["p"], d["g"], d["m"], d["v"], d["vhat"] if kind == "amsgrad" else None, case.coef,
                                                           case.mask, **cfg)
        what = (name, kind, cfg_name)
        for key, want in (("m", m_ref), ("v", v_ref), ("vhat", vhat_ref)):
            if want is not None:
                diff = np.flatnonzero(bits(buf[key][1]) != f32_bits(want))
                assert len(diff) == 0, "%s: %s differs on %d elements, first at %s" % (what, key, len(diff), diff[:8])
        ratio = np.abs(p.cpu().numpy().astype(np.float64) - p_ref) / RS.adam_bound(d["p"], upd)
        worst = int(ratio.argmax())
        print("%s: worst |p - p_exact| / bound %.3f at element %d" % (what, ratio[worst], worst))
        assert ratio[worst] <= 1.0, "%s: %d elements beyond the bound, first at %s" % (what, (ratio > 1).sum(), np.flatnonzero(ratio > 1)[:8])
        assert np.array_equal(bits(g), f32_bits(d["g"])), "%s: the gradient bucket was written" % (what,)
        assert all(guards_intact(w, n) for w, _ in buf.values()) and guards_intact(sw, n_bf16), what
        assert np.array_equal(bits(shadow), bits(p[:n_bf16].to(torch.bfloat16))), what
        assert (bits(p) != f32_bits(d["p"]))[~frozen].mean() > 0.9
        assert np.array_equal(bits(p)[frozen], f32_bits(d["p"])[frozen]), "frozen parameters moved"
        for key in buf:
            if key not in ("p", "g"):
                assert not bits(buf[key][1])[frozen].any(), "the state of frozen parameters was touched"


# ---- reg_sumsq ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["big", "one", "small"])
def test_reg_sumsq_is_exact_on_sparse_integers(ops, name):
    """w in {0, +-1, +-2}, g in {0, +-1}, non-zero near every boundary, every multiple of the grid pass, on the tail and on a regular
    sample: every float32 partial sum is an integer multiple of 1/4 below 2^24, so loss and gnorm_sq equal the float64 sums bit for
    bit whatever the order -- with and without the mask, each output alone and both together, and twice."""
    case = RS.build(name)
    w_h, g_h = RS.sparse_data(name)
    ww, w = guarded(case.n, w_h)
    gw, g = guarded(case.n, g_h)
    for use_mask in (True, False):
        segs = table(ops, name, use_mask)
        loss_ref, norm_ref, units = RS.reg_sums(w_h, g_h, case.coef, case.mask if use_mask else np.ones(case.n))
        assert units < 2 ** 24
        seen = []
        for want_loss, want_norm in ((True, True), (True, False), (False, True), (True, True)):
            loss, norm = dev([np.nan]), dev([np.nan])
            ops.reg_sumsq(w, g, segs, loss=loss if want_loss else None, gnorm_sq=norm if want_norm else None)
            torch.cuda.synchronize()
            what = (name, use_mask, want_loss, want_norm)
            if want_loss:
                assert float(loss.item()) == loss_ref, "%s: loss %r, exactly %r" % (what, float(loss.item()), loss_ref)
            else:
                assert np.isnan(loss.item()), what
            if want_norm:
                assert float(norm.item()) == norm_ref, "%s: gnorm_sq %r, exactly %r" % (what, float(norm.item()), norm_ref)
            else:
                assert np.isnan(norm.item()), what
            seen.append((bits(loss)[0], bits(norm)[0]))
        assert seen[0] == seen[3]
    assert np.array_equal(bits(w), f32_bits(w_h)) and np.array_equal(bits(g), f32_bits(g_h))
    assert guards_intact(ww, case.n) and guards_intact(gw, case.n)


@pytest.mark.parametrize("name", ["big", "small"])
def test_reg_sumsq_on_the_dense_data(ops, name):
    """The dyadic optimizer data (every element non-zero): float32 sums of 6.3 M terms round, so the 1e-5 relative tolerance of
    test_segments_regulariser_and_mask_inside_the_update; two calls are bit-identical."""
    case, d, segs = RS.build(name), RS.dense_data(name), table(ops, name)
    w, g = dev(d["p"]), dev(d["g"])
    loss_ref, norm_ref, _ = RS.reg_sums(d["p"], d["g"], case.coef, case.mask)
    out = []
    for _ in range(2):
        loss, norm = dev([np.nan]), dev([np.nan])
        ops.reg_sumsq(w, g, segs, loss=loss, gnorm_sq=norm)
        assert abs(float(loss.item()) - loss_ref) < 1e-5 * loss_ref and abs(float(norm.item()) - norm_ref) < 1e-5 * norm_ref
        out.append((bits(loss)[0], bits(norm)[0]))
    assert out[0] == out[1]


# ---- the unfused regulariser pass -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_mask", [True, False])
def test_l2_reg_writes_the_gradient_on_every_grid_pass(ops, use_mask):
    """dc_l2_reg_f32 with the per-element coef / mask vectors of "big": its grid is capped at 1024 blocks, so the 6.3 M elements take
    25 passes (24 full).  The written gradient equals g mask + 2 coef w bit for bit (dyadic data), w, coef and mask are not written,
    and the loss is bit-equal for two calls and within 1e-5 of the float64 sum."""
    case, d = RS.build("big"), RS.dense_data("big")
    n = case.n
    mask_h = case.mask if use_mask else np.ones(n, np.float32)
    want = RS.reg_grad(d["g"], d["p"], case.coef, mask_h)
    loss_ref = RS.reg_sums(d["p"], d["g"], case.coef, mask_h)[0]
    ww, w = guarded(n, d["p"])
    cw, coef = guarded(n, case.coef)
    mw, mask = guarded(n, case.mask)
    seen = []
    for _ in range(2):
        gw, g = guarded(n, d["g"])
        loss = dev([np.nan])
        ops.l2_reg(w, coef, grad=g, loss=loss, mask=mask if use_mask else None)
        torch.cuda.synchronize()
        diff = np.flatnonzero(bits(g) != f32_bits(want))
        assert len(diff) == 0, "the gradient differs on %d elements, first at %s" % (len(diff), diff[:8])
        assert abs(float(loss.item()) - loss_ref) < 1e-5 * loss_ref
        assert guards_intact(gw, n)
        seen.append(bits(loss)[0])
    assert seen[0] == seen[1]
    assert np.array_equal(bits(w), f32_bits(d["p"])) and np.array_equal(bits(coef), f32_bits(case.coef)) and np.array_equal(bits(mask), f32_bits(case.mask))
    assert guards_intact(ww, n) and guards_intact(cw, n) and guards_intact(mw, n)
    if use_mask:
        assert not want[case.mask == 0].any()                                      # a frozen element's gradient is zero, not g


# ---- one segment more than the table holds --------------------------------------------------------------------------------------------
def test_a_table_of_1025_segments_is_refused_and_nothing_is_written(ops):
    from image_captioning_amd import _lib
    case, d = RS.build("over"), RS.dense_data("over")
    segs = ops.RegSegmentTable(case.coef, case.mask, "cuda")
    assert segs.nseg == 1025 == ops.RegSegmentTable.MAX_SEGMENTS + 1
    buf = {key: guarded(case.n, d[key]) for key in ("p", "g", "m", "v", "vhat")}
    t = {key: view for key, (_, view) in buf.items()}
    loss, norm = dev([np.nan]), dev([np.nan])
    calls = {
        "dc_reg_sumsq": lambda: ops.reg_sumsq(t["p"], t["g"], segs, loss=loss, gnorm_sq=norm),
        "dc_amsgrad_step": lambda: ops.amsgrad_step(t["p"], t["g"], t["m"], t["v"], t["vhat"], RS.STEP, reg=segs),
        "dc_optimizer_step": lambda: ops.optimizer_step("adam", t["p"], t["g"], [t["m"], t["v"]], RS.STEP, reg=segs),
        "dc_optimizer_step (momentum)": lambda: ops.optimizer_step("sgd", t["p"], t["g"], [t["m"]], RS.STEP, beta1=RS.B1, reg=segs),
        "dc_optimizer_step (plain)": lambda: ops.optimizer_step("sgd", t["p"], t["g"], [], RS.STEP, beta1=0.0, reg=segs),
    }
    for who, call in calls.items():
        with pytest.raises(DcapError, match=r"%s: the segment table needs 1\.\.1024 segments, got 1025" % who.split(" ")[0]) as e:
            call()
        assert "(code %d)" % _lib.EINVAL in str(e.value), who
    torch.cuda.synchronize()
    for key, (whole, view) in buf.items():
        assert np.array_equal(bits(view), f32_bits(d[key])) and guards_intact(whole, case.n), "a refused call wrote %s" % key
    assert np.isnan(loss.item()) and np.isnan(norm.item())


def test_the_model_takes_the_unfused_passes_above_the_table_size(ops):
    """DenseImageCapRCNN._reg_segments() hands the step a table only while it fits the kernels' LDS copy (no model is built: the
    method reads the cached table alone)."""
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    model = object.__new__(DenseImageCapRCNN)
    model._reg_coef, model._train_mask = torch.zeros(1), None               # _masks() has run
    for nseg, fused in ((1, True), (1024, True), (1025, False), (5000, False)):
        model._reg_segs = types.SimpleNamespace(nseg=nseg)
        assert (model._reg_segments() is model._reg_segs) == fused and (fused or model._reg_segments() is None), nseg
