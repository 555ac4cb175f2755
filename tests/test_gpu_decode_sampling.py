"""Stochastic caption decoding on the device: ops.vocab_sample (the vocabulary GEMM fused with a Gumbel-max draw) against the float64
restatement of tests/_sampling_ref.py, and decoder='sampling' of CaptionModelV1, CaptionModelV2 and the joint model's generate_captions."""
import functools

import numpy as np
import pytest
import torch

import _sampling_ref as S
from _decode_cases import _dev, _exact_operands, _feat, record_host_syncs, v1_model

F64 = np.float64
SEED, OFFSET = 99, 1000
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib, ops
    _lib.load()
    return ops


# ---------------------------------------------------------------------------------------------- kernel
# name -> (M, K, V, ldw (None: contiguous), scale of W): one row / one column; a few columns; two row tiles and a ragged last column
# tile; V no multiple of 4 (the wrapper's padded copy of W); 40 column tiles; a W view with a row stride, handed over in place; W x 8
# (still exact in fp32 and bf16: peaked rows).
CASES = {"1x1": (1, 32, 1, None, 1), "5x7": (5, 32, 7, None, 1), "130x1000": (130, 64, 1000, None, 1), "257x333": (257, 32, 333, None, 1),
         "64x5003": (64, 256, 5003, None, 1), "ldw136": (45, 64, 130, 136, 1), "x8": (130, 64, 1000, None, 8)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(X, W [K,ldw or V], b, V, float64 logits z [M,V]) of a case, computed once and never changed."""
    Mr, K, V, ldw, scale = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    X, W, _ = _exact_operands(rng, Mr, K, ldw or V)
    _, _, b = _exact_operands(rng, 1, 32, V)
    W = W * np.float32(scale)
    if ldw:
        W[:, V:] = 64.0                                 # columns past V must never win
    z = X.astype(F64) @ W[:, :V].astype(F64) + b.astype(F64)
    for a in (X, W, b, z):
        a.setflags(write=False)
    return X, W, b, V, z


def _operands(name, bf):
    X, W, b, V, _ = _case(name)
    dt = BF16 if bf else torch.float32
    Xd, Wd = _dev(X).to(dt), _dev(W).to(dt)[:, :V]
    assert np.array_equal(Xd.float().cpu().numpy(), X)  # (exact in bf16 too)
    return Xd, Wd, _dev(b)


def _sample(ops, Xd, Wd, bd, **kw):
    """One call with every output: tokens, ids into column 1 of an [M,3] buffer, probs into column 2 of another, mask."""
    M_ = Xd.shape[0]
    out_ids = torch.full((M_, 3), -7, dtype=torch.int32, device="cuda:0")
    out_p = torch.full((M_, 3), -7.0, dtype=torch.float32, device="cuda:0")
    mask = torch.full((M_,), 9, dtype=torch.uint8, device="cuda:0")
    tok = ops.vocab_sample(Xd, Wd, bd, ids=out_ids[:, 1], probs=out_p[:, 2], mask=mask, **kw)
    torch.cuda.synchronize()
    ids, p = out_ids.cpu().numpy(), out_p.cpu().numpy()
    assert np.all(ids[:, [0, 2]] == -7) and np.all(p[:, [0, 1]] == -7.0)          # only the addressed columns are written
    tok = tok.cpu().numpy()
    np.testing.assert_array_equal(ids[:, 1], tok)
    np.testing.assert_array_equal(mask.cpu().numpy(), (tok != 0).astype(np.uint8))
    return tok, p[:, 2].copy()


@pytest.mark.gpu
@pytest.mark.parametrize("tau", [1.0, 0.7])
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_vocab_sample_against_the_float64_restatement(ops, name, bf, tau):
    """Every id equals the restatement's argmax, on inputs where NO row is undecided (asserted first, on the host: the restatement's
    two best perturbed values differ by at least 1e-4 on every row).  Why 1e-4 is enough: the operands are exact (_exact_operands), so
    the device's logits z are the float64 ones, bit for bit, in fp32 and in bf16; inv_t is the same float on both sides.  The device
    forms y = fma(z, inv_t, g): one rounding of a value of magnitude < 16 + 17 = 33, at most 1.9e-6.  Its g = -logf(-logf(u)) has u
    exact; the inner logf is within 1 ulp (1.2e-7 relative) of t = -log u, which moves log t by 1.2e-7 absolute, and the outer logf adds
    1 ulp of a value below 16.7, 1.9e-6: y is within 4e-6 < 1e-5 of the restatement for |z inv_t| <= 16, so the order of two values
    1e-4 apart cannot change.  probs within 1e-6 relative of the float64 softmax(z)[id] at temperature 1 (1e-5 on the x 8 case, whose
    logits are large, as the top-1 tests allow); tokens, mask and the strided ids / probs columns are checked by _sample."""
    _, _, _, V, z = _case(name)
    assert np.abs(z * S.inv_t(tau)).max() <= 16
    want, gap = S.choose(S.perturbed(z, tau, SEED, OFFSET))
    print("%s tau %g: smallest gap %.3g" % (name, tau, gap.min()))
    assert gap.min() >= S.GAP, "an undecided row: pick another seed"
    tok, p = _sample(ops, *_operands(name, bf), temperature=tau, seed=SEED, offset=OFFSET, **(dict(tile=128) if bf else {}))
    np.testing.assert_array_equal(tok, want)
    np.testing.assert_allclose(p, S.softmax_of(z, want), rtol=1e-5 if name == "x8" else 1e-6, atol=0)
    if V > 7:
        assert (tok != z.argmax(1)).any()                                         # (it samples: not the greedy choice everywhere)


@pytest.mark.gpu
@pytest.mark.parametrize("top_k", [None, 5])
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
def test_the_noise_depends_on_seed_offset_row_and_column_alone(ops, bf, top_k):
    """Rows [0, 64) of an M = 257 call (three row tiles) equal an M = 64 call on those rows at the same offset, bit for bit; an offset
    shifted by +3 reproduces rows 3.. of the unshifted call on the correspondingly shifted inputs; another seed draws other words."""
    Xd, Wd, bd = _operands("257x333", bf)
    kw = dict(temperature=0.7, top_k=top_k, **(dict(tile=128) if bf else {}))
    tok, p = _sample(ops, Xd, Wd, bd, seed=SEED, offset=OFFSET, **kw)
    tok64, p64 = _sample(ops, Xd[:64], Wd, bd, seed=SEED, offset=OFFSET, **kw)
    assert np.array_equal(tok[:64], tok64) and np.array_equal(p[:64].view(np.int32), p64.view(np.int32))
    tok3, p3 = _sample(ops, Xd[3:].contiguous(), Wd, bd, seed=SEED, offset=OFFSET + 3, **kw)
    assert np.array_equal(tok[3:], tok3) and np.array_equal(p[3:].view(np.int32), p3.view(np.int32))
    wrap, _ = _sample(ops, Xd[:8], Wd, bd, seed=SEED, offset=2 ** 32 - 3, **kw)   # the row counter wraps at 2^32
    low, _ = _sample(ops, Xd[3:8].contiguous(), Wd, bd, seed=SEED, offset=0, **kw)
    assert np.array_equal(wrap[3:], low)
    other, _ = _sample(ops, Xd, Wd, bd, seed=SEED + 1, offset=OFFSET, **kw)
    assert (other != tok).mean() > 0.25
    again, p_again = _sample(ops, Xd, Wd, bd, seed=SEED, offset=OFFSET, **kw)
    assert np.array_equal(again, tok) and np.array_equal(p_again.view(np.int32), p.view(np.int32))
    if bf:                                                                        # the precision path does not enter the noise either
        f32, _ = _sample(ops, *_operands("257x333", False), seed=SEED, offset=OFFSET, temperature=0.7, top_k=top_k)
        assert np.array_equal(f32, tok)


@pytest.mark.gpu
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
def test_a_vanishing_temperature_is_greedy(ops, bf):
    """tau = 2^-20: distinct exact logits differ by at least 1/2048, 512 after scaling, far above the noise's range of 19.4 (g lies in
    [-2.82, 16.64]): the ids are ops.vocab_top1's on every row whose two best logits are not exactly equal."""
    Xd, Wd, bd = _operands("130x1000", bf)
    z = _case("130x1000")[4]
    top2 = np.sort(z, axis=1)[:, -2:]
    clear = top2[:, 1] > top2[:, 0]
    assert clear.mean() > 0.9
    tok, p = _sample(ops, Xd, Wd, bd, temperature=2.0 ** -20, seed=SEED, offset=OFFSET)
    want = ops.vocab_top1(Xd, Wd, bd).cpu().numpy()
    np.testing.assert_array_equal(tok[clear], want[clear])
    np.testing.assert_array_equal(want, z.argmax(1))
    np.testing.assert_allclose(p[clear], S.softmax_of(z, want)[clear], rtol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [None, 128, 256], ids=["f32", "bf16-128", "bf16-256"])
def test_top_k_1_is_vocab_top1_bit_for_bit(ops, tile):
    for name in ("130x1000", "257x333", "5x7", "1x1"):
        Xd, Wd, bd = _operands(name, tile is not None)
        kw = dict(tile=tile) if tile else {}
        M_ = Xd.shape[0]
        want_p = torch.empty((M_,), dtype=torch.float32, device="cuda:0")
        want = ops.vocab_top1(Xd, Wd, bd, probs=want_p, **kw).cpu().numpy()
        for tau in (1.0, 0.7, 2.0 ** -20, 50.0):
            tok, p = _sample(ops, Xd, Wd, bd, temperature=tau, top_k=1, seed=SEED, offset=OFFSET, **kw)
            np.testing.assert_array_equal(tok, want)
            np.testing.assert_array_equal(p.view(np.int32), want_p.cpu().numpy().view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [None, 128, 256], ids=["f32", "bf16-128", "bf16-256"])
@pytest.mark.parametrize("name", ["130x1000", "64x5003", "5x7", "x8"])
def test_top_k_5_draws_among_the_five_best(ops, name, tile):
    """Every id is one of ops.vocab_topk(k=5)'s and equals the restatement's choice among the float64 top five (value descending, then
    column ascending: the exact logits make both lists the same), on inputs with no undecided row; probs keep their meaning; the two
    bf16 tiles draw the same words."""
    _, _, _, V, z = _case(name)
    tau = 2.0
    order = np.argsort(-z, axis=1, kind="stable")[:, :5]
    allowed = np.zeros(z.shape, bool)
    np.put_along_axis(allowed, order, True, axis=1)
    want, gap = S.choose(S.perturbed(z, tau, SEED, OFFSET), allowed)
    assert gap.min() >= S.GAP, "an undecided row: pick another seed"
    Xd, Wd, bd = _operands(name, tile is not None)
    kw = dict(tile=tile) if tile else {}
    top_ids, _ = ops.vocab_topk(Xd, Wd, bd, 5, **kw)
    np.testing.assert_array_equal(top_ids.cpu().numpy(), order)
    tok, p = _sample(ops, Xd, Wd, bd, temperature=tau, top_k=5, seed=SEED, offset=OFFSET, **kw)
    assert (tok[:, None] == order).any(1).all()
    np.testing.assert_array_equal(tok, want)
    np.testing.assert_allclose(p, S.softmax_of(z, want), rtol=1e-5 if name == "x8" else 1e-6, atol=0)
    assert (tok != order[:, 0]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
def test_rows_without_an_orderable_logit_and_nan_logits(ops, bf):
    """A bias of -inf everywhere makes every logit -inf: id 0, as ops.vocab_top1 answers.  A NaN logit never wins: with one NaN bias
    the ids are the restatement's with that column left out, over the whole vocabulary and among the top five."""
    X, W, b, V, z = _case("130x1000")
    Xd, Wd, _ = _operands("130x1000", bf)
    none = torch.full((V,), float("-inf"), device="cuda:0")
    for top_k in (None, 1, 5):
        tok, _ = _sample(ops, Xd, Wd, none, temperature=1.0, top_k=top_k, seed=SEED, offset=OFFSET)
        assert np.all(tok == 0)
    assert np.all(ops.vocab_top1(Xd, Wd, none).cpu().numpy() == 0)
    y = S.perturbed(z, 1.0, SEED, OFFSET)
    col = int(np.bincount(S.choose(y)[0], minlength=V).argmax())                  # the column the sampler draws most often
    bn = b.copy()
    bn[col] = np.nan
    y[:, col] = np.nan
    want, gap = S.choose(y)
    assert gap.min() >= S.GAP and np.all(want != col)
    tok, _ = _sample(ops, Xd, Wd, _dev(bn), temperature=1.0, seed=SEED, offset=OFFSET)
    np.testing.assert_array_equal(tok, want)
    zn = z.copy()
    zn[:, col] = -np.inf
    order = np.argsort(-zn, axis=1, kind="stable")[:, :5]
    allowed = np.zeros(z.shape, bool)
    np.put_along_axis(allowed, order, True, axis=1)
    want5, gap5 = S.choose(y, allowed)
    assert gap5.min() >= S.GAP
    tok5, _ = _sample(ops, Xd, Wd, _dev(bn), temperature=1.0, top_k=5, seed=SEED, offset=OFFSET)
    np.testing.assert_array_equal(tok5, want5)


@pytest.mark.gpu
def test_vocab_sample_refusals_on_the_device(ops):
    from image_captioning_amd import _lib
    Xd, Wd, bd = _operands("5x7", True)
    with pytest.raises(_lib.DcapError, match="128"):                              # the 256 tile has no sampling epilogue
        ops.vocab_sample(Xd, Wd, bd, seed=1, tile=256)
    ops.vocab_sample(Xd, Wd, bd, seed=1, tile=256, top_k=2)
    with pytest.raises(_lib.DcapError, match="top_k"):
        ops.vocab_sample(Xd, Wd, bd, seed=1, top_k=8)                             # above V = 7
    Xf, Wf, bf_ = _operands("5x7", False)
    with pytest.raises(_lib.DcapError, match="tile"):
        ops.vocab_sample(Xf, Wf, bf_, seed=1, tile=128)
    with pytest.raises(_lib.DcapError, match="tokens"):
        ops.vocab_sample(Xf, Wf, bf_, seed=1, tokens=torch.empty((4,), dtype=torch.int32, device="cuda:0"))
    assert tuple(ops.vocab_sample(Xf[:0], Wf, bf_, seed=1).shape) == (0,)         # M = 0: no launch
    lib = _lib.load()
    assert lib.dc_vocab_sample_workspace_bytes(130, 1000, 0) == 130 * 8 * 24 + (-130 * 8 * 24) % 256
    assert lib.dc_vocab_sample_workspace_bytes(130, 1000, 5) == lib.dc_vocab_topk_workspace_bytes(130, 1000, 5)
    assert lib.dc_vocab_sample_bf16_workspace_bytes(130, 1000, 64, 0, 256) == 0
    d = _lib.VocabSampleBf16Desc()                                                # the C entry point itself refuses the 256 tile too
    d.M, d.V, d.K, d.X, d.ldx, d.W, d.ldw = 5, 7, 32, Xd.data_ptr(), 32, Xd.data_ptr(), 8
    tok = torch.empty((5,), dtype=torch.int32, device="cuda:0")
    d.tokens, d.inv_t, d.tile = tok.data_ptr(), 1.0, 256
    assert lib.dc_vocab_sample_bf16(d, None, 0, None) != 0 and b"128" in lib.dc_last_error()


# ---------------------------------------------------------------------------------------------- Model 3
V1_SEED = 7


def _teacher_forced(step_probs, ids, scores, tau, top_k, seed, cap):
    """The device's words fed step by step to the float64 decoder: at every (RoI, step) the device's word is the float64 argmax of
    log p / tau + g unless the two best values lie within 1e-3 (well above the 1e-5-grade error these small models' logits show against
    the oracle); at most `cap` cells may be that close; every word score within 1e-5 of the float64 probability of the device's word
    (the incremental oracle tests' tolerance)."""
    n, T = ids.shape
    choice, gap, p = S.decode(step_probs, n, T, tau, top_k, seed, forced=ids)
    undecided = gap < 1e-3
    print("undecided cells: %d of %d; smallest gap %.3g" % (undecided.sum(), undecided.size, gap.min()))
    assert undecided.sum() <= cap
    np.testing.assert_array_equal(ids[~undecided], choice[~undecided])
    chosen = np.take_along_axis(p, ids[:, :, None].astype(np.int64), 2)[:, :, 0]
    assert np.abs(scores - chosen).max() < 1e-5


@pytest.fixture(scope="module")
def v1(ops):
    V, T, B = 1000, 6, 37
    model = v1_model(V, T, B, seed=80)
    return model, {k: v.astype(F64) for k, v in model.get_weights_dict().items()}, _feat(81, B), T, B


@pytest.mark.gpu
@pytest.mark.parametrize("tau,top_k", [(1.0, None), (0.7, None), (1.5, 5)])
def test_v1_sampling_decoder_teacher_forced_against_float64(v1, tau, top_k):
    """37 RoIs x 6 steps = 222 cells.  The seed is one at which the float64 decoder, sampling freely on its own tokens, has no
    undecided cell (asserted): then the device's captions are that decoder's, and under teacher forcing at most 2 cells may be close."""
    model, Wt, feat, T, B = v1
    step = S.v1_step_probs(Wt, feat, T)
    free, free_gap, _ = S.decode(step, B, T, tau, top_k, V1_SEED)
    assert free_gap.min() >= 1e-3, "an undecided cell: pick another seed"
    probs, ids, scores = model.generate(feat, return_probabilities=False, decoder="sampling", seed=V1_SEED, temperature=tau, top_k=top_k)
    assert probs is None and ids.shape == (B, T) and ids.dtype == np.int32 and scores.shape == (B, T) and scores.dtype == np.float32
    _teacher_forced(step, ids, scores, tau, top_k, V1_SEED, cap=2)
    np.testing.assert_array_equal(ids, free)
    _, greedy, _ = model.generate(feat, return_probabilities=False, decoder="incremental")
    assert (ids != greedy).any()


@pytest.mark.gpu
def test_v1_sampling_is_reproducible_and_top_k_1_is_incremental(v1, monkeypatch):
    model, _, feat, T, B = v1
    fd = torch.tensor(feat, device="cuda:0")
    a = model._decode_greedy(fd, None, (0.8, None, 11)).clone()
    b = model._decode_greedy(fd, None, (0.8, None, 11)).clone()
    c = model._decode_greedy(fd, None, (0.8, None, 12)).clone()
    assert torch.equal(a, b) and not torch.equal(a[0], c[0])                       # the same seed twice: identical buffers
    calls = record_host_syncs(monkeypatch)
    ids, scores = model.decode_sampling(fd, 11, temperature=0.8)
    ids5, _ = model.decode_sampling(fd, 11, top_k=5)
    monkeypatch.undo()
    assert calls == []                                                            # no host synchronisation
    assert ids.is_cuda and scores.is_cuda and ids.dtype == torch.int32 and scores.dtype == torch.float32 and tuple(ids.shape) == (B, T)
    assert torch.equal(ids, a[0])
    g_ids, g_scores = (t.clone() for t in model.decode_greedy(fd))
    for tau in (1.0, 0.3):
        k_ids, k_scores = model.decode_sampling(fd, 11, temperature=tau, top_k=1)
        assert torch.equal(k_ids, g_ids) and torch.equal(k_scores.view(torch.int32), g_scores.view(torch.int32))
    _, e_ids, e_sc = model.generate(np.zeros((0, 7, 7, 256), np.float32), return_probabilities=False, decoder="sampling", seed=1)
    assert e_ids.shape == (0, T) and e_sc.shape == (0, T)


@pytest.mark.gpu
def test_v1_bf16_sampling_decoder(ops):
    """vocab_math='bf16' under the rule of 'incremental': top_k=1 is that decoder bit for bit, and the same seed draws the same captions."""
    model = v1_model(1000, 6, 37, seed=80, compute_dtype="bf16")
    fd = torch.tensor(_feat(81, 37), device="cuda:0")
    g_ids, g_scores = (t.clone() for t in model.decode_greedy(fd, vocab_math="bf16"))
    k_ids, k_scores = model.decode_sampling(fd, 3, temperature=0.5, top_k=1, vocab_math="bf16")
    assert torch.equal(k_ids, g_ids) and torch.equal(k_scores.view(torch.int32), g_scores.view(torch.int32))
    a = [t.clone() for t in model.decode_sampling(fd, 3, vocab_math="bf16")]
    b = model.decode_sampling(fd, 3, vocab_math="bf16")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], g_ids)
    assert bool(((a[1] > 0) & (a[1] <= 1)).all())


# ---------------------------------------------------------------------------------------------- v2 decoders
V2_SEED = 3


@pytest.mark.gpu
@pytest.mark.parametrize("inject", [True, False], ids=["inject", "merge"])
def test_v2_sampling_decoder(ops, monkeypatch, inject):
    """With start_ids: top_k=1 equals the incremental decoder (ids, and word scores bit for bit); the same seed twice gives identical
    buffers; no host synchronisation; and the teacher-forced check against the float64 decoder (12 RoIs x 9 steps; the seed is one at
    which the free-running float64 decoder has no undecided cell)."""
    from test_gpu_decode_v2 import _make_v2
    V, Tw, R, tau = 1000, 10, 12, 0.9
    model, Wt = _make_v2(V, inject, Tw, seed=91, scale=4.0)
    feat = _feat(92, R)
    start = np.random.default_rng(93).integers(1, V, R).astype(np.int32)
    start[::5] = 0
    g_ids, g_scores = model.generate(feat, decoder="incremental", start_ids=start)
    k_ids, k_scores = model.generate(feat, decoder="sampling", start_ids=start, seed=V2_SEED, temperature=tau, top_k=1)
    np.testing.assert_array_equal(k_ids, g_ids)
    np.testing.assert_array_equal(k_scores.view(np.int32), g_scores.view(np.int32))
    fd, sd = torch.tensor(feat, device="cuda:0"), _dev(start, torch.int32)
    a = model._decode_greedy(fd, None, sd, (tau, None, V2_SEED)).clone()
    b = model._decode_greedy(fd, None, sd, (tau, None, V2_SEED)).clone()
    assert torch.equal(a, b)
    calls = record_host_syncs(monkeypatch)
    d_ids, d_scores = model.decode_sampling(fd, V2_SEED, start_ids=sd, temperature=tau)
    monkeypatch.undo()
    assert calls == [] and d_ids.is_cuda and tuple(d_ids.shape) == (R, Tw - 1) and torch.equal(d_ids, a[0])
    ids, scores = model.generate(feat, decoder="sampling", start_ids=start, seed=V2_SEED, temperature=tau)
    np.testing.assert_array_equal(ids, d_ids.cpu().numpy())
    step = S.v2_step_probs(Wt, feat, Tw, inject, start)
    free, free_gap, _ = S.decode(step, R, Tw - 1, tau, None, V2_SEED)
    assert free_gap.min() >= 1e-3, "an undecided cell: pick another seed"
    _teacher_forced(step, ids, scores, tau, None, V2_SEED, cap=2)
    np.testing.assert_array_equal(ids, free)
    assert (ids != g_ids).any()


# ---------------------------------------------------------------------------------------------- the joint model
def _scores_apart(model, sampling, b):
    """The condition of tests/test_gpu_refine_generations.py on the input: the float64 caption scores that order image b's NMS differ
    by more than 1e-9 relative between sorted neighbours (the zero-padded proposals, identical in everything, count once)."""
    from image_captioning_amd import decoding
    props = model.last_proposals
    feats = model.plan().roi_features(boxes_norm=props)
    cm = model.caption_model
    _, sc = decoding.greedy_views(cm._decode_greedy(feats[b], None, sampling, b * cm.T * props.shape[1]).cpu().numpy())
    s = np.log(sc.astype(F64)).sum(1)
    real = np.abs(props[b].cpu().numpy()).sum(1) > 0
    s = np.sort(np.concatenate([s[real], s[~real][:1]]))
    assert np.all(np.diff(s) > 1e-9 * np.maximum(1.0, np.abs(s[1:]))), "near-tie in the caption scores: pick another seed"
    return int(real.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2])
def test_generate_captions_sampling_device_equals_host(ops, monkeypatch, batch):
    """256 x 256 images, V = 1000, 300 proposals: postprocess='device' equals 'host' on every key, with one host copy per call; the
    same call twice gives the same results; and the two images of a batch do not get the same noise (image b decodes at offset
    b * T * K): the same image twice in one batch is captioned differently, where the incremental decoder captions it alike."""
    from image_captioning_amd import synth
    from test_gpu_refine_generations import _joint, _same
    model, cfg = _joint(batch)
    img = synth.images(7, 1, 256, 256)[0]
    imgs = [img] * batch
    kw = dict(decoder="sampling", seed=21, temperature=0.8)
    host = model.generate_captions(imgs, return_probabilities=False, **kw)
    for b in range(batch):
        assert _scores_apart(model, (0.8, None, 21), b) > 50
    device = model.generate_captions(imgs, return_probabilities=False, postprocess="device", **kw)
    assert all(sorted(r) == ["ids", "rois"] and 0 < len(r["rois"]) <= cfg.DETECTION_MAX_INSTANCES for r in host)
    _same(host, device)
    calls = record_host_syncs(monkeypatch)
    again = model.generate_captions(imgs, return_probabilities=False, postprocess="device", **kw)
    monkeypatch.undo()
    assert calls == ["cpu", "numpy"]
    _same(device, again)
    other = model.generate_captions(imgs, return_probabilities=False, postprocess="device", decoder="sampling", seed=22, temperature=0.8)
    assert not np.array_equal(other[0]["ids"], device[0]["ids"])
    if batch == 2:
        greedy = model.generate_captions(imgs, return_probabilities=False, postprocess="device", decoder="incremental")
        assert np.array_equal(greedy[0]["ids"], greedy[1]["ids"]) and np.array_equal(greedy[0]["rois"], greedy[1]["rois"])
        assert device[0]["ids"].shape != device[1]["ids"].shape or not np.array_equal(device[0]["ids"], device[1]["ids"])
        cm, K = model.caption_model, model.last_proposals.shape[1]
        feats = model.plan().roi_features(boxes_norm=model.last_proposals)
        first = cm._decode_greedy(feats[1], None, (0.8, None, 21), 0).clone()
        second = cm._decode_greedy(feats[1], None, (0.8, None, 21), cm.T * K).clone()
        assert torch.equal(first, cm._decode_greedy(feats[0], None, (0.8, None, 21), 0)) and not torch.equal(first[0], second[0])
