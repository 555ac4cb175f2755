"""Incremental on-device greedy decoding: ops.vocab_top1 (the vocabulary GEMM fused with the row top-1), ops.lstm_step (one LSTM
timestep with carried state), CaptionModelV1.decode_greedy / generate(decoder='incremental') and the joint model's
generate_captions(decoder='incremental').  GPU tests are marked; the argument checks at the end run without a GPU."""
import numpy as np
import pytest
import torch

from _decode_cases import _dev, _exact_operands, joint_model, record_host_syncs, v1_model
from oracle import np_models as M
from oracle import np_oracle as O

MEAN = [123.7, 116.8, 103.9]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _ref_top1(X, W, b):
    z = X.astype(np.float64) @ W.astype(np.float64) + b.astype(np.float64)
    ids = z.argmax(1)
    m = z.max(1, keepdims=True)
    p = 1.0 / np.exp(z - m).sum(1)
    top2 = np.sort(z, axis=1)[:, -2:] if z.shape[1] > 1 else np.concatenate([z - 1.0, z], axis=1)
    return ids, p, top2[:, 1] - top2[:, 0]


def _top1(X, W, b, M_):
    from image_captioning_amd import ops
    out_ids = torch.full((M_, 3), -7, dtype=torch.int32, device="cuda:0")
    out_p = torch.full((M_, 3), -7.0, dtype=torch.float32, device="cuda:0")
    mask = torch.empty((M_,), dtype=torch.uint8, device="cuda:0")
    tok = ops.vocab_top1(X, W, b, ids=out_ids[:, 1], probs=out_p[:, 2], mask=mask)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), out_ids.cpu().numpy(), out_p.cpu().numpy(), mask.cpu().numpy()


# ---------------------------------------------------------------------------------------------- kernel
@pytest.mark.gpu
@pytest.mark.parametrize("Mr", [1, 37, 1000])
@pytest.mark.parametrize("V", [24, 1001, 10000, 50000])
def test_vocab_top1_against_float64(gpu, Mr, V):
    """ids exact (exact logits: exact ties included, the lowest index winning as in NumPy), p within 1e-6 relative, the strided output
    columns and the mask byte, and two calls bit-identical.  Then N(0,1) data, whose fp32 logits carry GEMM rounding: ids exact wherever
    the float64 top-two gap exceeds 1e-5 (most rows), p within 1e-5."""
    K = 256
    rng = np.random.default_rng(Mr * 7 + V)
    X, W, b = _exact_operands(rng, Mr, K, V)
    want_ids, want_p, gap = _ref_top1(X, W, b)
    tok, ids, p, mask = _top1(_dev(X), _dev(W), _dev(b), Mr)
    np.testing.assert_array_equal(tok, want_ids)
    np.testing.assert_array_equal(ids[:, 1], tok)
    assert np.all(ids[:, [0, 2]] == -7) and np.all(p[:, [0, 1]] == -7.0)        # only the addressed columns are written
    np.testing.assert_array_equal(mask, (tok != 0).astype(np.uint8))
    np.testing.assert_allclose(p[:, 2], want_p, rtol=1e-6, atol=0)
    tok2, ids2, p2, mask2 = _top1(_dev(X), _dev(W), _dev(b), Mr)
    assert np.array_equal(tok, tok2) and np.array_equal(ids, ids2) and np.array_equal(p.view(np.int32), p2.view(np.int32))
    X = rng.standard_normal((Mr, K)).astype(np.float32)
    W = (rng.standard_normal((K, V)) / np.sqrt(K)).astype(np.float32)
    b = (0.5 * rng.standard_normal(V)).astype(np.float32)
    want_ids, want_p, gap = _ref_top1(X, W, b)
    tok, _, p, _ = _top1(_dev(X), _dev(W), _dev(b), Mr)
    ok = gap > 1e-5
    assert ok.mean() > 0.9
    np.testing.assert_array_equal(tok[ok], want_ids[ok])
    np.testing.assert_allclose(p[:, 2], want_p, rtol=1e-5, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("V,ldw", [(1, 4), (3, 8), (1001, 1004), (130, 132)])
def test_vocab_top1_ragged_v_in_place(gpu, V, ldw):
    """V % 4 != 0 handed to the kernel directly (a [K,ldw] buffer viewed as [K,V], ldw % 4 == 0): the last column tile's guard.
    (test_vocab_top1_against_float64's contiguous V = 1001 takes the other branch: the wrapper's padded copy of W.)"""
    K, Mr = 64, 45
    rng = np.random.default_rng(V)
    X, Wfull, _ = _exact_operands(rng, Mr, K, ldw)
    _, _, b = _exact_operands(rng, 1, 32, V)
    Wfull[:, V:] = 64.0                                # columns past V must never win
    want_ids, want_p, gap = _ref_top1(X, Wfull[:, :V], b)
    Wd = _dev(Wfull)[:, :V]
    assert Wd.stride(0) == ldw
    tok, _, p, _ = _top1(_dev(X), Wd, _dev(b), Mr)
    np.testing.assert_array_equal(tok, want_ids)
    np.testing.assert_allclose(p[:, 2], want_p, rtol=1e-6)


@pytest.mark.gpu
def test_vocab_top1_ties_lowest_index_wins(gpu):
    """Duplicated columns give bit-identical logits: the lowest index wins, inside one 128-column tile and across tiles."""
    K, Mr, V = 128, 70, 5000
    rng = np.random.default_rng(3)
    X, W, b = _exact_operands(rng, Mr, K, V)
    for group in ((5, 9, 4000), (131, 300, 4999)):    # a tie inside one 128-column tile, and ties across tiles
        src = group[0]
        for c in group[1:]:
            W[:, c] = W[:, src]
        b[list(group)] = 8.0                           # the duplicated columns are every row's maximum
    tok, _, p, _ = _top1(_dev(X), _dev(W), _dev(b), Mr)
    want_ids, want_p, _ = _ref_top1(X, W, b)          # (float64 argmax: the first of the exactly equal maxima)
    assert set(want_ids) == {5, 131}                   # every row's maximum is one of the two triplicated columns
    np.testing.assert_array_equal(tok, want_ids)
    np.testing.assert_allclose(p[:, 2], want_p, rtol=1e-6)


@pytest.mark.gpu
def test_vocab_top1_large_logits(gpu):
    """Logits of magnitude ~80 (exp(z) alone would be near fp32 overflow): no inf / NaN, exact ids.  p is held to 2e-5 relative here:
    rounding z to fp32 at |z| = 80 alone moves z - max by up to 7.6e-6."""
    K, Mr, V = 256, 300, 20000
    rng = np.random.default_rng(5)
    X = rng.standard_normal((Mr, K)).astype(np.float32)
    W = (rng.standard_normal((K, V)) / np.sqrt(K)).astype(np.float32)
    b = rng.uniform(-80.0, 80.0, V).astype(np.float32)
    want_ids, want_p, gap = _ref_top1(X, W, b)
    tok, _, p, _ = _top1(_dev(X), _dev(W), _dev(b), Mr)
    assert np.all(np.isfinite(p[:, 2])) and np.all(p[:, 2] > 0) and np.all(p[:, 2] <= 1)
    ok = gap > 1e-4
    assert ok.mean() > 0.9
    np.testing.assert_array_equal(tok[ok], want_ids[ok])
    np.testing.assert_allclose(p[:, 2], want_p, rtol=2e-5)


# ---------------------------------------------------------------------------------------------- LSTM step
@pytest.mark.gpu
@pytest.mark.parametrize("U,packed", [(512, True), (512, False), (36, False)])
def test_lstm_step_matches_sequence(gpu, U, packed):
    """T calls of ops.lstm_step feeding (h, c) forward under a mask with holes in the middle of rows == lstm_seq_fwd, bit for bit
    (the same kernels at the same B)."""
    from image_captioning_amd import ops
    B, T = 37, 6
    rng = np.random.default_rng(U)
    z = (0.5 * rng.standard_normal((T * B, 4 * U))).astype(np.float32)
    Ur = (rng.standard_normal((U, 4 * U)) / np.sqrt(U)).astype(np.float32)
    mask = np.ones((T, B), np.uint8)
    mask[2:4, ::3] = 0                                 # holes in the middle of rows
    mask[0, 1::5] = 0                                  # and masked first steps (state stays zero)
    assert mask[:, 0].tolist() == [1, 1, 0, 0, 1, 1]
    Ud = _dev(Ur)
    h_seq, c_seq = ops.lstm_seq_fwd(_dev(z), Ud, _dev(mask.reshape(-1), torch.uint8), B, T)
    pk = ops.lstm_pack_urec(Ud) if packed else None
    h = c = None
    hs, cs = [], []
    for t in range(T):
        zt = _dev(z[t * B:(t + 1) * B])
        h, c = ops.lstm_step(zt, Ud, h, c, _dev(mask[t], torch.uint8), U_packed=pk)
        hs.append(h)
        cs.append(c)
    got_h, got_c = torch.cat(hs).cpu().numpy(), torch.cat(cs).cpu().numpy()
    np.testing.assert_array_equal(got_h, h_seq.cpu().numpy())
    np.testing.assert_array_equal(got_c, c_seq.cpu().numpy())
    hm = got_h.reshape(T, B, U)
    assert np.array_equal(hm[3, 0], hm[1, 0]) and not np.array_equal(hm[4, 0], hm[3, 0])      # the carry over the hole


# ---------------------------------------------------------------------------------------------- v1 decoder
def _v1(V, T, B, seed=30, units=512):
    return v1_model(V, T, B, seed, units)


@pytest.mark.gpu
@pytest.mark.parametrize("V,T,B", [(1000, 6, 3), (10000, 15, 200)])
def test_v1_incremental_decoder_against_oracle(gpu, V, T, B):
    """ids against the float64 oracle's greedy decoder; word scores within 1e-5 of its chosen-word probabilities.  At B = 200 the ids
    are held exact on every row whose oracle decisions all have a top-two probability gap above 1e-5 relative (nearly all rows: a
    closer call is inside fp32 rounding, and a caption diverges after it)."""
    model = _v1(V, T, B)
    Wt = {k: v.astype(np.float64) for k, v in model.get_weights_dict().items()}
    feat = np.random.default_rng(31).standard_normal((B, 7, 7, 256)).astype(np.float32)
    probs, ids, scores = model.generate(feat, return_probabilities=False, decoder="incremental")
    assert probs is None and ids.shape == (B, T) and ids.dtype == np.int32 and scores.shape == (B, T) and scores.dtype == np.float32
    want_p, want_ids = M.v1_greedy_decode(Wt, feat, T)
    top2 = np.sort(want_p, axis=2)[:, :, -2:]
    sure = ((top2[:, :, 1] - top2[:, :, 0]) > 1e-5 * top2[:, :, 1]).all(axis=1)
    if B <= 3:
        assert sure.all()
    assert sure.mean() > 0.95
    np.testing.assert_array_equal(ids[sure], want_ids[sure])
    chosen = np.take_along_axis(want_p, want_ids[:, :, None].astype(np.int64), 2)[:, :, 0]
    assert np.abs(scores[sure] - chosen[sure]).max() < 1e-5


def _zero_bias_for_mid_caption_zeros(model, feat):
    """Raise the bias of word 0 so that some RoI emits a non-zero first word and 0 later (chosen from the prefix decoder's
    probabilities: the decode path only changes from the first step where word 0 wins)."""
    probs, _ = model.generate(feat)
    r = np.log(probs.max(-1)) - np.log(probs[:, :, 0])          # [B,T]: how far word 0 is behind the winner
    later = r[:, 1:].min(1)
    b = int(np.argmax(r[:, 0] - later))
    assert r[b, 0] - later[b] > 1e-2
    delta = 0.5 * (r[b, 0] + later[b])
    bias = model.store.w['imgcap_lstm_d2/bias']
    bias[0:1] += float(delta)
    return b


@pytest.mark.gpu
def test_incremental_agrees_with_prefix_through_the_mask_carry(gpu):
    """ids identical to decoder='prefix' and word scores within 2e-6 relative, on RoIs that emit id 0 in mid-caption (the two decoders run
    the same fp32 products, but GEMMs over B rows and over T*B rows may split K differently: ~1e-6 on a probability).  A generated 0 is
    masked: the state is carried over it, so the greedy choice repeats -- 0 with the same probability, bit for bit, in both decoders
    (a 0 followed by a non-zero id cannot happen under the carry; without it the embedding of word 0 would move the state)."""
    V, T, B = 1000, 8, 24
    model = _v1(V, T, B, seed=40)
    feat = np.random.default_rng(41).standard_normal((B, 7, 7, 256)).astype(np.float32)
    row = _zero_bias_for_mid_caption_zeros(model, feat)
    _, ids_p, sc_p = model.generate(feat, return_probabilities=False)
    _, ids_i, sc_i = model.generate(feat, return_probabilities=False, decoder="incremental")
    np.testing.assert_array_equal(ids_i, ids_p)
    np.testing.assert_allclose(sc_i, sc_p, rtol=2e-6, atol=0)
    assert ids_i[row, 0] != 0 and (ids_i[row] == 0).any()
    for ids, sc in ((ids_i, sc_i), (ids_p, sc_p)):
        for b in range(B):
            z = np.flatnonzero(ids[b] == 0)
            if z.size:
                j = z[0]
                assert np.all(ids[b, j:] == 0) and np.all(sc[b, j:].view(np.int32) == sc[b, j].view(np.int32)), (b, ids[b], sc[b])


@pytest.mark.gpu
def test_decode_greedy_never_syncs_with_the_host(gpu, monkeypatch):
    model = _v1(1000, 6, 5, seed=50)
    feat = torch.tensor(np.random.default_rng(51).standard_normal((5, 7, 7, 256)).astype(np.float32), device="cuda:0")
    model.decode_greedy(feat)                              # warm: buffers and workspaces
    calls = record_host_syncs(monkeypatch)
    ids, scores = model.decode_greedy(feat)
    monkeypatch.undo()
    assert calls == []
    assert ids.is_cuda and scores.is_cuda and ids.dtype == torch.int32 and scores.dtype == torch.float32
    assert tuple(ids.shape) == (5, 6) and tuple(scores.shape) == (5, 6)
    _, want_ids, want_sc = model.generate(feat, return_probabilities=False)
    np.testing.assert_array_equal(ids.cpu().numpy(), want_ids)


@pytest.mark.gpu
def test_degenerate_batches(gpu):
    model = _v1(1000, 1, 4, seed=60)
    feat = np.random.default_rng(61).standard_normal((4, 7, 7, 256)).astype(np.float32)
    _, ids_i, sc_i = model.generate(feat, return_probabilities=False, decoder="incremental")
    _, ids_p, sc_p = model.generate(feat, return_probabilities=False)
    assert ids_i.shape == (4, 1)
    np.testing.assert_array_equal(ids_i, ids_p)
    np.testing.assert_allclose(sc_i, sc_p, rtol=2e-6)
    model = _v1(1000, 6, 4, seed=60)
    probs, ids, sc = model.generate(np.zeros((0, 7, 7, 256), np.float32), return_probabilities=False, decoder="incremental")
    assert probs is None and ids.shape == (0, 6) and sc.shape == (0, 6)


# ---------------------------------------------------------------------------------------------- joint model
@pytest.mark.gpu
def test_joint_model_incremental_captions(gpu, monkeypatch):
    """generate_captions(decoder='incremental') at the shape of test_joint_model_inference_captions: the same rois and ids as the prefix
    decoder (with the caption scores that order the NMS well apart), and the prefix decoder's ids match the oracle's decode of the
    oracle's features."""
    from image_captioning_amd import synth, dense_model
    S, V, T = 128, 24, 5
    model, cfg, Wt = joint_model(S, V, T)
    img = synth.images(7, 1, S, S)
    seen = []
    orig = dense_model.refine_generations
    monkeypatch.setattr(dense_model, "refine_generations", lambda rois, ws, window, config: (seen.append(np.array(ws)), orig(rois, ws, window, config))[1])
    res = model.generate_captions([img[0]])[0]
    light = model.generate_captions([img[0]], return_probabilities=False, decoder="incremental")[0]
    assert len(seen) == 2
    cap = np.sort(np.log(seen[1].astype(np.float64)).sum(1))
    assert np.diff(cap).min() > 1e-5                       # no near-tie in the NMS order
    np.testing.assert_allclose(seen[1], seen[0], rtol=2e-6)        # (see test_incremental_agrees_with_prefix_through_the_mask_carry)
    assert "captions" not in light
    np.testing.assert_array_equal(light["rois"], res["rois"])
    np.testing.assert_array_equal(light["ids"], res["ids"])
    K = res["rois"].shape[0]
    assert 0 < K <= 10
    props = model.last_proposals.cpu().numpy()
    x = O.mold_image(img, MEAN)
    _, C2, C3, C4, C5 = M.resnet_graph(x, Wt, 1)
    maps = M.fpn_graph(C2, C3, C4, C5, Wt)[:4]
    feats = O.pyramid_roi_align(props, list(maps), (S, S, 3), 7)[0]
    want_probs, want_ids = M.v1_greedy_decode(Wt, feats, T)
    hits = 0
    for k in range(K):
        d = np.abs(want_probs - res["captions"][k][None]).reshape(len(want_probs), -1).max(1)
        j = int(d.argmin())
        assert d[j] < 1e-3
        hits += int(np.array_equal(want_ids[j], light["ids"][k]))
    assert hits == K


# ---------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("rp", [True, None])
def test_incremental_decoder_needs_return_probabilities_false(rp):
    from image_captioning_amd.text_generation_model import CaptionModelV1
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    stub = object.__new__(CaptionModelV1)
    with pytest.raises(ValueError, match="return_probabilities=False"):
        CaptionModelV1.generate(stub, np.zeros((2, 7, 7, 256), np.float32), return_probabilities=rp, decoder="incremental")
    with pytest.raises(ValueError, match="return_probabilities=False"):
        DenseImageCapRCNN.generate_captions(object.__new__(DenseImageCapRCNN), [np.zeros((8, 8, 3), np.uint8)], return_probabilities=rp,
                                            decoder="incremental")


def test_unknown_decoder_is_refused():
    from image_captioning_amd.text_generation_model import CaptionModelV1
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    with pytest.raises(ValueError, match="decoder"):
        CaptionModelV1.generate(object.__new__(CaptionModelV1), np.zeros((2, 7, 7, 256), np.float32), return_probabilities=False, decoder="beam")
    with pytest.raises(ValueError, match="decoder"):
        DenseImageCapRCNN.generate_captions(object.__new__(DenseImageCapRCNN), [np.zeros((8, 8, 3), np.uint8)], return_probabilities=False,
                                            decoder="beam")


def test_decode_ops_refuse_cpu_tensors():
    from image_captioning_amd import ops, _lib
    with pytest.raises(_lib.DcapError):
        ops.vocab_top1(torch.zeros(4, 32), torch.zeros(32, 8), torch.zeros(8))
    with pytest.raises(_lib.DcapError):
        ops.lstm_step(torch.zeros(4, 128), torch.zeros(32, 128))
    with pytest.raises(_lib.DcapError):
        ops.lstm_pack_urec(torch.zeros(32, 128))
