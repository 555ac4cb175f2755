"""The fused vocabulary top-1 / top-k on bf16 operands (dc_vocab_top1_bf16 / dc_vocab_topk_bf16 through ops.vocab_top1 / ops.vocab_topk,
both tile shapes and the automatic choice) and the incremental decoders' vocab_math='bf16'.

References are float64 products of the operands the kernel reads (the bf16 values, exactly representable in float64), so no tolerance
here stands for the distance between bf16 and fp32 arithmetic:
  * operands on coarse binary grids (at most 5 significant bits: exact in bf16; every product and partial sum exact in fp32 up to
    K = 1024) must give the float64 answer outright -- ids identical on every row, exact ties included;
  * on random operands the kernel's fp32 accumulation is allowed the textbook bound of an fp32 dot product of length K summed in any
    order, |error| <= K 2^-24 sum_k |x_k w_kv| per logit: a row's ids are held exact when all its top-(k+1) adjacent float64 gaps
    exceed twice that bound at the row's worst column (RULE below); at most 10 % of the rows may fall outside."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from _decode_cases import _dev, _exact_operands, joint_model, record_host_syncs, v1_model

MEAN = [123.7, 116.8, 103.9]
TILES = (128, 256, 0)
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _bf(a):
    """float32 host array -> bf16 device tensor, rounded to nearest even by the library's cast."""
    return _dev(a).to(BF16)


def _f64(t):
    """device tensor (bf16 or float32) -> float64 host array of exactly its values."""
    return t.detach().to(torch.float32).cpu().numpy().astype(np.float64)


def _ref_topk(z, k):
    """float64 logits [M,V] -> (ids [M,k+1] in the family's strict order: value descending, column ascending; their values; the softmax
    probabilities of the first k).  k+1 rounds of argmax (NumPy's argmax takes the first of equal maxima), as the kernel's rounds."""
    z = z.copy()
    m = z.max(1, keepdims=True)
    s = np.exp(z - m).sum(1)
    n = min(k + 1, z.shape[1])
    ids = np.zeros((z.shape[0], n), np.int64)
    val = np.zeros((z.shape[0], n))
    rows = np.arange(z.shape[0])
    for r in range(n):
        ids[:, r] = z.argmax(1)
        val[:, r] = z[rows, ids[:, r]]
        z[rows, ids[:, r]] = -np.inf
    p = np.exp(val[:, :k] - m) / s[:, None]
    return ids, val, p


def _rule(X64, W64, val):
    """RULE: rows whose top-(k+1) adjacent float64 gaps all exceed 2 K 2^-24 max_v sum_k |x_k w_kv|."""
    K = X64.shape[1]
    bound = 2.0 * K * 2.0 ** -24 * (np.abs(X64) @ np.abs(W64)).max(1)
    gaps = val[:, :-1] - val[:, 1:]
    return gaps.min(1) > bound


def _topk(X, W, b, k, tile):
    from image_captioning_amd import ops
    ids, p = ops.vocab_topk(X, W, b, k, tile=tile)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), p.cpu().numpy()


def _top1(X, W, b, M_, tile):
    from image_captioning_amd import ops
    out_ids = torch.full((M_, 3), -7, dtype=torch.int32, device="cuda:0")
    out_p = torch.full((M_, 3), -7.0, dtype=torch.float32, device="cuda:0")
    mask = torch.full((M_,), 9, dtype=torch.uint8, device="cuda:0")
    tok = ops.vocab_top1(X, W, b, ids=out_ids[:, 1], probs=out_p[:, 2], mask=mask, tile=tile)
    torch.cuda.synchronize()
    return tok.cpu().numpy(), out_ids.cpu().numpy(), out_p.cpu().numpy(), mask.cpu().numpy()


# ---------------------------------------------------------------------------------------------- kernel: exact operands
@functools.lru_cache(maxsize=1)
def _exact_case(Mr, V, K):
    rng = np.random.default_rng(Mr * 7 + V + K)
    X, W, b = _exact_operands(rng, Mr, K, V)
    z = X.astype(np.float64) @ W.astype(np.float64) + b.astype(np.float64)
    return X, W, b, z


# a covering selection: every M, V, K, k at least once per tile shape; the corner 1000 x 50 000 x 1024 at k = 1 and k = 8
EXACT_SHAPES = [(1, 24, 256, 1), (1, 10000, 256, 3), (37, 1001, 256, 3), (37, 10000, 1024, 8), (1000, 50000, 1024, 1), (1000, 50000, 1024, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("Mr,V,K,k,tile", [s + (t,) for s in EXACT_SHAPES for t in TILES])
def test_exact_operands_give_the_float64_answer(gpu, Mr, V, K, k, tile):
    """ids identical on every row, top-k order included; probabilities within 1e-6 relative (the fp32 family's tolerance for its own
    exp / sum).  At k = 1 through vocab_top1: strided outputs write only the addressed columns, the mask byte; through vocab_topk too."""
    X, W, b, z = _exact_case(Mr, V, K)
    want_ids, _, want_p = _ref_topk(z, k)
    Xd, Wd, bd = _bf(X), _bf(W), _dev(b)
    assert np.array_equal(_f64(Xd), X.astype(np.float64)) and np.array_equal(_f64(Wd), W.astype(np.float64))    # exact in bf16
    ids, p = _topk(Xd, Wd, bd, k, tile)
    err = np.abs(p - want_p).max() / want_p.min()
    print("exact M=%d V=%d K=%d k=%d tile=%d: ids equal %s, worst p error / smallest p %.3e" % (Mr, V, K, k, tile, np.array_equal(ids, want_ids[:, :k]), err))
    np.testing.assert_array_equal(ids, want_ids[:, :k])
    np.testing.assert_allclose(p, want_p, rtol=1e-6, atol=0)
    if k == 1:
        tok, oi, op, mask = _top1(Xd, Wd, bd, Mr, tile)
        np.testing.assert_array_equal(tok, want_ids[:, 0])
        np.testing.assert_array_equal(oi[:, 1], tok)
        assert np.all(oi[:, [0, 2]] == -7) and np.all(op[:, [0, 1]] == -7.0)        # only the addressed columns are written
        np.testing.assert_array_equal(mask, (tok != 0).astype(np.uint8))
        np.testing.assert_allclose(op[:, 2], want_p[:, 0], rtol=1e-6, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("k", [1, 3, 8])
def test_exact_ties_inside_a_cell_across_cells_and_across_the_tile_edge(gpu, k, tile):
    """Duplicated columns give bit-identical logits; the lowest column wins and the tied columns come out in ascending order: two
    columns of one 64-column slice, columns of different cells of one 256-column tile, and columns either side of a 256-column edge."""
    K, Mr, V = 128, 70, 5000
    rng = np.random.default_rng(3)
    X, W, b = _exact_operands(rng, Mr, K, V)
    for group in ((5, 9, 200, 4000), (131, 255, 256, 4999)):
        for c in group[1:]:
            W[:, c] = W[:, group[0]]
        b[list(group)] = 8.0                           # the duplicated columns are every row's best
    z = X.astype(np.float64) @ W.astype(np.float64) + b.astype(np.float64)
    want_ids, _, want_p = _ref_topk(z, k)
    assert set(want_ids[:, 0]) == {5, 131}
    if k >= 3:
        assert all(tuple(r[:3]) in ((5, 9, 200), (131, 255, 256)) for r in want_ids)
    ids, p = _topk(_bf(X), _bf(W), _dev(b), k, tile)
    np.testing.assert_array_equal(ids, want_ids[:, :k])
    np.testing.assert_allclose(p, want_p, rtol=1e-6, atol=0)
    if k == 1:
        tok, _, op, _ = _top1(_bf(X), _bf(W), _dev(b), Mr, tile)
        np.testing.assert_array_equal(tok, want_ids[:, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("V,ldw", [(1, 8), (3, 8), (1001, 1008), (130, 136), (250, 264), (257, 272)])
def test_ragged_v_in_place_with_poisoned_padding(gpu, V, ldw, tile):
    """V % 8 != 0 handed to the kernel in place (a [K,ldw] buffer viewed as [K,V], ldw % 8 == 0): the columns V .. ldw - 1 hold 64.0
    and must never win or enter the sum.  (The contiguous V = 1001 of the test above takes the wrapper's padded copy instead.)"""
    K, Mr = 64, 45
    rng = np.random.default_rng(V)
    X, Wfull, _ = _exact_operands(rng, Mr, K, ldw)
    _, _, b = _exact_operands(rng, 1, 32, V)
    Wfull[:, V:] = 64.0
    z = X.astype(np.float64) @ Wfull[:, :V].astype(np.float64) + b.astype(np.float64)
    Wd = _bf(Wfull)[:, :V]
    assert Wd.stride(0) == ldw and Wd.data_ptr() % 16 == 0
    tok, _, op, _ = _top1(_bf(X), Wd, _dev(b), Mr, tile)
    want_ids, _, want_p = _ref_topk(z, 1)
    np.testing.assert_array_equal(tok, want_ids[:, 0])
    np.testing.assert_allclose(op[:, 2], want_p[:, 0], rtol=1e-6)
    k = min(3, V)
    want_ids, _, want_p = _ref_topk(z, k)
    ids, p = _topk(_bf(X), Wd, _dev(b), k, tile)
    np.testing.assert_array_equal(ids, want_ids[:, :k])
    np.testing.assert_allclose(p, want_p, rtol=1e-6)


# ---------------------------------------------------------------------------------------------- kernel: random operands
def _random_case(seed, Mr, K, V, bias_scale=0.5, uniform=None):
    rng = np.random.default_rng(seed)
    Xd = _bf(rng.standard_normal((Mr, K)).astype(np.float32))
    Wd = _bf((rng.standard_normal((K, V)) / np.sqrt(K)).astype(np.float32))
    b = (rng.uniform(-uniform, uniform, V) if uniform else bias_scale * rng.standard_normal(V)).astype(np.float32)
    X64, W64 = _f64(Xd), _f64(Wd)
    z = X64 @ W64 + b.astype(np.float64)
    return Xd, Wd, _dev(b), X64, W64, z


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("Mr,K,V,k", [(300, 256, 10000, 1), (300, 256, 10000, 5), (300, 256, 10000, 8), (300, 1024, 50000, 1), (300, 1024, 50000, 3)])
def test_random_operands_against_float64_of_the_rounded_operands(gpu, Mr, K, V, k, tile):
    """N(0,1) X, N(0,1)/sqrt(K) W rounded to bf16; the reference is the float64 product of the ROUNDED operands plus the fp32 bias.
    ids exact on every row inside RULE (at most 10 % outside); probabilities within 1e-5 relative (the fp32 family's random-data
    tolerance; the r-th best value is compared, which does not depend on which of two near-tied columns holds it)."""
    Xd, Wd, bd, X64, W64, z = _random_case(K + V + k, Mr, K, V)
    want_ids, val, want_p = _ref_topk(z, k)
    ok = _rule(X64, W64, val)
    ids, p = _topk(Xd, Wd, bd, k, tile)
    rel = np.abs(p - want_p) / want_p
    print("random K=%d V=%d k=%d tile=%d: %.1f %% of rows inside the rule, ids equal on them: %s; worst p error %.3e relative"
          % (K, V, k, tile, 100 * ok.mean(), np.array_equal(ids[ok], want_ids[ok, :k]), rel.max()))
    assert ok.mean() >= 0.9
    np.testing.assert_array_equal(ids[ok], want_ids[ok, :k])
    np.testing.assert_allclose(p, want_p, rtol=1e-5, atol=0)
    if k == 1:
        tok, _, op, _ = _top1(Xd, Wd, bd, Mr, tile)
        np.testing.assert_array_equal(tok[ok], want_ids[ok, 0])
        np.testing.assert_allclose(op[:, 2], want_p[:, 0], rtol=1e-5, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_large_bias_logits_stay_finite(gpu, tile):
    """Logits of magnitude ~80 (exp(z) alone would be near fp32 overflow): finite probabilities in (0, 1], ids by RULE.  p is held to
    2e-5 relative here, as the fp32 family holds it: rounding z to fp32 at |z| = 80 alone moves z - max by up to 7.6e-6."""
    Mr, K, V = 300, 256, 20000
    Xd, Wd, bd, X64, W64, z = _random_case(5, Mr, K, V, uniform=80.0)
    want_ids, val, want_p = _ref_topk(z, 3)
    ok = _rule(X64, W64, val) & (val[:, :-1] - val[:, 1:] > 2 * 2.0 ** -18).all(1)      # (and half an fp32 ulp of |z| <= 128 on either logit)
    ids, p = _topk(Xd, Wd, bd, 3, tile)
    assert np.all(np.isfinite(p)) and np.all(p > 0) and np.all(p <= 1)
    assert ok.mean() >= 0.9
    np.testing.assert_array_equal(ids[ok], want_ids[ok, :3])
    np.testing.assert_allclose(p, want_p, rtol=2e-5, atol=0)
    tok, _, op, _ = _top1(Xd, Wd, bd, Mr, tile)
    assert np.all(np.isfinite(op[:, 2])) and np.all(op[:, 2] > 0) and np.all(op[:, 2] <= 1)
    np.testing.assert_array_equal(tok[ok], want_ids[ok, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [128, 256])
def test_deterministic_and_the_same_at_every_m(gpu, tile):
    """Two calls bit-identical; with the tile shape fixed, a row decoded alone and inside a batch of 300 gives the same ids and the same
    probability bits.  (Across the two tile shapes the accumulation order of a logit differs: only RULE holds between them.)"""
    Mr, K, V, k = 300, 512, 10000, 5
    Xd, Wd, bd, _, _, _ = _random_case(77, Mr, K, V)
    ids, p = _topk(Xd, Wd, bd, k, tile)
    ids2, p2 = _topk(Xd, Wd, bd, k, tile)
    assert np.array_equal(ids, ids2) and np.array_equal(p.view(np.int32), p2.view(np.int32))
    tok, _, op, _ = _top1(Xd, Wd, bd, Mr, tile)
    for r in (0, 129, 299):
        ids1, p1 = _topk(Xd[r:r + 1].clone(), Wd, bd, k, tile)
        assert np.array_equal(ids1[0], ids[r]) and np.array_equal(p1.view(np.int32)[0], p.view(np.int32)[r]), r
        t1, _, o1, _ = _top1(Xd[r:r + 1].clone(), Wd, bd, 1, tile)
        assert t1[0] == tok[r] and o1[0, 2].view(np.int32) == op[r, 2].view(np.int32), r


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_topk_at_k1_is_top1_bit_for_bit(gpu, tile):
    Mr, K, V = 130, 256, 3000
    Xd, Wd, bd, _, _, _ = _random_case(78, Mr, K, V)
    ids, p = _topk(Xd, Wd, bd, 1, tile)
    tok, oi, op, _ = _top1(Xd, Wd, bd, Mr, tile)
    np.testing.assert_array_equal(tok, ids[:, 0])
    np.testing.assert_array_equal(op[:, 2].view(np.int32), p[:, 0].view(np.int32))


@pytest.mark.gpu
def test_the_automatic_tile_is_one_of_the_two_and_sizes_the_workspace(gpu):
    from image_captioning_amd import ops, _lib
    lib = _lib.load()
    for M_, V, K in ((1, 24, 256), (200, 10000, 1024), (1000, 50000, 1024), (3000, 50000, 1024)):
        t = ops.vocab_topk_bf16_tile(M_, V, K)
        assert t in (128, 256)
        for k in (1, 8):
            assert lib.dc_vocab_topk_bf16_workspace_bytes(M_, V, K, k, 0) == lib.dc_vocab_topk_bf16_workspace_bytes(M_, V, K, k, t)
            cells = (V + 63) // 64 if t == 256 else (V + 127) // 128
            assert lib.dc_vocab_topk_bf16_workspace_bytes(M_, V, K, k, t) >= M_ * cells * (k + 1) * 8
        assert lib.dc_vocab_top1_bf16_workspace_bytes(M_, V, K, t) == lib.dc_vocab_topk_bf16_workspace_bytes(M_, V, K, 1, t)
    assert ops.vocab_topk_bf16_tile(3000, 50000, 1024) == 256          # the training step's shape: dc_vocab_ce's large tile
    assert ops.vocab_topk_bf16_tile(1, 24, 256) == 128


@pytest.mark.gpu
def test_argument_refusals(gpu):
    """Mixed dtypes, K % 8, a misaligned base, a tile that is none of 0 / 128 / 256, a workspace that is too small: the wrapper's DcapError
    and the family's codes from the C entry points (DC_EINVAL -1, DC_EALIGN -2, DC_EWORKSPACE -3)."""
    from image_captioning_amd import ops, _lib
    lib = _lib.load()
    X = torch.zeros((4, 64), dtype=BF16, device="cuda:0")
    W = torch.zeros((64, 40), dtype=BF16, device="cuda:0")
    b = torch.zeros(40, device="cuda:0")
    for fn in (lambda x, w, **kw: ops.vocab_top1(x, w, b, **kw), lambda x, w, **kw: ops.vocab_topk(x, w, b, 2, **kw)):
        with pytest.raises(_lib.DcapError):
            fn(X, W.float())
        with pytest.raises(_lib.DcapError):
            fn(X.float(), W)
        with pytest.raises(_lib.DcapError, match="multiple of 8"):
            fn(X[:, :36].contiguous(), W[:36])
        with pytest.raises(_lib.DcapError, match="tile"):
            fn(X, W, tile=64)
        with pytest.raises(_lib.DcapError, match="tile"):
            fn(X.float(), W.float(), tile=128)             # tile= is a bf16 option
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
    ids = torch.zeros((4, 2), dtype=torch.int32, device="cuda:0")
    pr = torch.zeros((4, 2), device="cuda:0")

    def desc(**kw):
        d = _lib.VocabTopkBf16Desc()
        d.M, d.V, d.K, d.k = 4, 40, 64, 2
        d.X, d.ldx, d.W, d.ldw = X.data_ptr(), 64, W.data_ptr(), 40
        d.bias, d.ids, d.probs, d.tile = b.data_ptr(), ids.data_ptr(), pr.data_ptr(), 0
        for key, v in kw.items():
            setattr(d, key, v)
        return d

    def call(d, nbytes=1 << 20):
        return lib.dc_vocab_topk_bf16(C.byref(d), C.c_void_p(ws.data_ptr()), nbytes, None)

    assert call(desc()) == 0
    assert call(desc(K=36)) == -2
    assert call(desc(ldw=44)) == -2
    assert call(desc(X=X.data_ptr() + 2)) == -2
    assert call(desc(W=W.data_ptr() + 8)) == -2
    assert call(desc(V=41)) == -1                          # ldw < V rounded up to 8
    assert call(desc(tile=64)) == -1
    assert call(desc(k=9)) == -1
    for tile in TILES:
        need = lib.dc_vocab_topk_bf16_workspace_bytes(4, 40, 64, 2, tile)
        assert need > 0 and call(desc(tile=tile), need - 1) == -3 and call(desc(tile=tile), need) == 0
    d1 = _lib.VocabTop1Bf16Desc()
    tok = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    d1.M, d1.V, d1.K, d1.X, d1.ldx, d1.W, d1.ldw, d1.tokens, d1.tile = 4, 40, 64, X.data_ptr(), 64, W.data_ptr(), 40, tok.data_ptr(), 0
    assert lib.dc_vocab_top1_bf16(C.byref(d1), C.c_void_p(ws.data_ptr()), 1 << 20, None) == 0
    d1.tile = 7
    assert lib.dc_vocab_top1_bf16(C.byref(d1), C.c_void_p(ws.data_ptr()), 1 << 20, None) == -1
    d1.tile, d1.K = 0, 36
    assert lib.dc_vocab_top1_bf16(C.byref(d1), C.c_void_p(ws.data_ptr()), 1 << 20, None) == -2
    d1.K = 64
    assert lib.dc_vocab_top1_bf16(C.byref(d1), C.c_void_p(ws.data_ptr()), 15, None) == -3
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- models
def _v1_bf16(V, T, B, seed=30, units=512):
    return v1_model(V, T, B, seed, units, compute_dtype="bf16")


class _Recorder(object):
    """Wraps ops.vocab_top1 (and ops.gemm_bf16's gather index) to keep each token step's operands and outputs."""

    def __init__(self, monkeypatch):
        from image_captioning_amd import ops
        self.steps, self.gathers = [], []
        top1, gemm_bf16 = ops.vocab_top1, ops.gemm_bf16

        def rec_top1(X, W, bias=None, tokens=None, ids=None, probs=None, mask=None, **kw):
            out = top1(X, W, bias, tokens=tokens, ids=ids, probs=probs, mask=mask, **kw)
            self.steps.append(dict(X=X.clone(), X_dtype=X.dtype, X_shape=tuple(X.shape), W=W, W_ptr=W.data_ptr(), bias=bias, tokens=tokens.clone(),
                                   tok_ptr=tokens.data_ptr(), ids=ids.clone(), probs=probs.clone(), mask=mask.clone()))
            return out

        def rec_gemm(A, Bm, *a, **kw):
            if kw.get("gather") is not None:
                self.gathers.append((kw["gather"].data_ptr(), kw["gather"].clone()))
            return gemm_bf16(A, Bm, *a, **kw)

        monkeypatch.setattr(ops, "vocab_top1", rec_top1)
        monkeypatch.setattr(ops, "gemm_bf16", rec_gemm)


@pytest.mark.gpu
@pytest.mark.parametrize("V,T,B", [(1000, 6, 24), (10000, 15, 200)])
def test_v1_bf16_vocabulary_wiring_against_float64(gpu, monkeypatch, V, T, B):
    """generate(decoder='incremental', vocab_math='bf16'): every token step hands ops.vocab_top1 the bf16 tensor of a1 [B,1024], the
    model's bf16 mirror itself (the same storage at every step, no per-token copy) and the layer's bias; the step's ids are the float64
    argmax over exactly those operands (RULE); the tokens written at step j are the gather index of step j + 1's embedding GEMM; the
    returned ids / scores are the recorded per-step outputs."""
    model = _v1_bf16(V, T, B)
    feat = np.random.default_rng(31).standard_normal((B, 7, 7, 256)).astype(np.float32)
    rec = _Recorder(monkeypatch)
    probs, ids, scores = model.generate(feat, return_probabilities=False, decoder="incremental", vocab_math="bf16")
    monkeypatch.undo()
    assert probs is None and ids.shape == (B, T) and ids.dtype == np.int32 and scores.shape == (B, T) and scores.dtype == np.float32
    assert len(rec.steps) == T and len(rec.gathers) == T
    mirror = model.store.wb['imgcap_lstm_d2/kernel']
    bias = model.store.w['imgcap_lstm_d2/bias']
    W64, b64 = _f64(mirror.view(-1, V)), _f64(bias)
    np.testing.assert_array_equal(rec.gathers[0][1].cpu().numpy(), np.ones(B, np.int32))      # the start token
    inside = []
    for j, s in enumerate(rec.steps):
        assert s["X_dtype"] == BF16 and s["X_shape"] == (B, 1024)
        assert s["W"].dtype == BF16 and s["W_ptr"] == mirror.data_ptr() and tuple(s["W"].shape) == (1024, V) and s["W"].stride(0) == V
        assert s["bias"].data_ptr() == bias.data_ptr()
        X64 = _f64(s["X"])
        want_ids, val, want_p = _ref_topk(X64 @ W64 + b64, 1)
        ok = _rule(X64, W64, val)
        inside.append(ok.mean())
        got = s["tokens"].cpu().numpy()
        np.testing.assert_array_equal(got[ok], want_ids[ok, 0])
        np.testing.assert_allclose(s["probs"].cpu().numpy(), want_p[:, 0], rtol=1e-5, atol=0)
        np.testing.assert_array_equal(s["ids"].cpu().numpy(), got)
        np.testing.assert_array_equal(s["mask"].cpu().numpy(), (got != 0).astype(np.uint8))
        np.testing.assert_array_equal(ids[:, j], got)
        np.testing.assert_array_equal(scores[:, j].view(np.int32), s["probs"].cpu().numpy().view(np.int32))
        if j + 1 < T:
            assert rec.gathers[j + 1][0] == s["tok_ptr"]
            np.testing.assert_array_equal(rec.gathers[j + 1][1].cpu().numpy(), got)
    print("wiring V=%d: share of rows inside the rule per step: min %.3f" % (V, min(inside)))
    assert min(inside) >= 0.9


@pytest.mark.gpu
@pytest.mark.parametrize("V,T,B", [(1000, 6, 24), (10000, 15, 200)])
def test_every_disagreement_with_the_fp32_vocabulary_is_operand_rounding(gpu, monkeypatch, V, T, B):
    """Decode once with vocab_math='f32' and once with 'bf16'.  Up to and including a RoI's first differing step both runs carry the
    same LSTM state, so there the fp32 run's word f and the bf16 run's word b can both be scored in float64 from the fp32 run's recorded
    operands.  Rounding an operand to bf16 (8 significant bits, nearest even) moves it by at most 2^-8 relative, a product by at most
    2^-7 + 2^-16, so logit v by at most e_v = (2^-7 + 2^-16) sum_k |a_k| |W_kv|; with the accumulation bound a_v = K 2^-24 sum_k |x_k w_kv|
    of the bf16 kernel (on its rounded operands, themselves within e_v's factor): z64(f) - z64(b) <= e_f + e_b + 2 a_f + 2 a_b.  No cap on
    how many RoIs differ: the bound is the test."""
    model = _v1_bf16(V, T, B)
    feat = np.random.default_rng(31).standard_normal((B, 7, 7, 256)).astype(np.float32)
    rec32 = _Recorder(monkeypatch)
    _, ids32, _ = model.generate(feat, return_probabilities=False, decoder="incremental", vocab_math="f32")
    monkeypatch.undo()
    rec16 = _Recorder(monkeypatch)
    _, ids16, _ = model.generate(feat, return_probabilities=False, decoder="incremental", vocab_math="bf16")
    monkeypatch.undo()
    assert all(s["X_dtype"] == torch.float32 for s in rec32.steps) and all(s["X_dtype"] == BF16 for s in rec16.steps)
    W64 = _f64(model.store.w['imgcap_lstm_d2/kernel'].view(-1, V))
    b64 = _f64(model.store.w['imgcap_lstm_d2/bias'])
    differ = np.flatnonzero((ids32 != ids16).any(1))
    worst = 0.0
    for r in differ:
        j = int(np.flatnonzero(ids32[r] != ids16[r])[0])
        assert np.array_equal(ids32[r, :j], ids16[r, :j])
        a = _f64(rec32.steps[j]["X"][r])
        np.testing.assert_array_equal(_f64(rec16.steps[j]["X"][r]), _f64(rec32.steps[j]["X"][r].to(BF16)))      # the same state, rounded once
        f, b = int(ids32[r, j]), int(ids16[r, j])
        zf, zb = a @ W64[:, f] + b64[f], a @ W64[:, b] + b64[b]
        sf, sb = np.abs(a) @ np.abs(W64[:, f]), np.abs(a) @ np.abs(W64[:, b])
        K = a.shape[0]
        bound = (2.0 ** -7 + 2.0 ** -16) * (sf + sb) + 2 * K * 2.0 ** -24 * (sf + sb)
        worst = max(worst, (zf - zb) / bound)
        assert zf - zb <= bound, (r, j, f, b, zf - zb, bound)
    print("vocab_math f32 vs bf16, V=%d B=%d: %d of %d RoIs differ (%.1f %% identical captions); worst gap / bound %.3f"
          % (V, B, differ.size, B, 100.0 * (1 - differ.size / B), worst))


@pytest.mark.gpu
def test_joint_bf16_model_captions_with_the_bf16_vocabulary(gpu, monkeypatch):
    """generate_captions(decoder='incremental', vocab_math='bf16') on a compute_dtype='bf16' joint model: well-formed results, the word
    scores that order the NMS are the recorded outputs of the bf16 vocabulary steps, and vocab_math=None is the call without the keyword."""
    from image_captioning_amd import synth, dense_model
    S, V, T = 128, 24, 5
    model, cfg, _ = joint_model(S, V, T, compute_dtype="bf16")
    img = synth.images(7, 1, S, S)
    seen = []
    orig = dense_model.refine_generations
    monkeypatch.setattr(dense_model, "refine_generations", lambda rois, ws, window, config: (seen.append(np.array(ws)), orig(rois, ws, window, config))[1])
    rec = _Recorder(monkeypatch)
    res = model.generate_captions([img[0]], return_probabilities=False, decoder="incremental", vocab_math="bf16")[0]
    steps = list(rec.steps)
    plain = model.generate_captions([img[0]], return_probabilities=False, decoder="incremental")[0]
    none = model.generate_captions([img[0]], return_probabilities=False, decoder="incremental", vocab_math=None)[0]
    f32 = model.generate_captions([img[0]], return_probabilities=False, decoder="incremental", vocab_math="f32")[0]
    later = rec.steps[len(steps):]
    monkeypatch.undo()
    assert len(steps) == T and all(s["X_dtype"] == BF16 and s["W"].dtype == BF16 and s["X_shape"][1] == 1024 for s in steps)
    assert len(later) == 3 * T and all(s["X_dtype"] == torch.float32 for s in later)
    n = steps[0]["X_shape"][0]
    assert len(seen) == 4 and seen[0].shape == (n, T)
    want = np.stack([s["probs"].cpu().numpy() for s in steps], axis=1)
    np.testing.assert_array_equal(seen[0].view(np.int32), want.view(np.int32))
    K = res["rois"].shape[0]
    assert 0 < K <= 10 and res["rois"].shape == (K, 4) and res["ids"].shape == (K, T) and res["ids"].dtype == np.int32
    assert res["ids"].min() >= 0 and res["ids"].max() < V and "captions" not in res
    for other in (none, f32):
        np.testing.assert_array_equal(other["rois"], plain["rois"])
        np.testing.assert_array_equal(other["ids"], plain["ids"])
    np.testing.assert_array_equal(seen[2].view(np.int32), seen[1].view(np.int32))
    np.testing.assert_array_equal(seen[3].view(np.int32), seen[1].view(np.int32))


@pytest.mark.gpu
def test_decode_greedy_bf16_never_syncs_with_the_host(gpu, monkeypatch):
    model = _v1_bf16(1000, 6, 5, seed=50)
    feat = torch.tensor(np.random.default_rng(51).standard_normal((5, 7, 7, 256)).astype(np.float32), device="cuda:0")
    model.decode_greedy(feat, vocab_math="bf16")           # warm: buffers and workspaces
    calls = record_host_syncs(monkeypatch)
    ids, scores = model.decode_greedy(feat, vocab_math="bf16")
    monkeypatch.undo()
    assert calls == []
    assert ids.is_cuda and scores.is_cuda and ids.dtype == torch.int32 and scores.dtype == torch.float32
    assert tuple(ids.shape) == (5, 6) and tuple(scores.shape) == (5, 6)
    _, want_ids, want_sc = model.generate(feat, return_probabilities=False, decoder="incremental", vocab_math="bf16")
    np.testing.assert_array_equal(ids.cpu().numpy(), want_ids)
    np.testing.assert_array_equal(scores.cpu().numpy().view(np.int32), want_sc.view(np.int32))


@pytest.mark.gpu
def test_a_mirror_whose_rows_are_not_16_byte_chunks_is_padded_once(gpu):
    """V = 1004 (a multiple of 4, as the model requires, not of 8): the decoder's operand is one zero-padded copy of the mirror (the same
    buffer from call to call) that ops.vocab_top1 takes as it is, and it scores words as the mirror's own values do (RULE)."""
    from image_captioning_amd import ops
    V, B = 1004, 9
    model = _v1_bf16(V, 4, B, seed=70)
    mirror = model.store.wb['imgcap_lstm_d2/kernel'].view(-1, V)
    Wv = model._vocab_mirror()
    assert Wv.data_ptr() != mirror.data_ptr() and Wv.data_ptr() % 16 == 0 and Wv.stride(0) == 1008 and tuple(Wv.shape) == (1024, V)
    assert model._vocab_mirror().data_ptr() == Wv.data_ptr()
    W64, b64 = _f64(mirror), _f64(model.store.w['imgcap_lstm_d2/bias'])
    np.testing.assert_array_equal(_f64(Wv), W64)
    Xd = _bf(np.random.default_rng(71).standard_normal((B, 1024)).astype(np.float32))
    seen = []
    orig = ops._vocab_operands
    ops._vocab_operands = lambda X, W, b: (seen.append(W.data_ptr()), orig(X, W, b))[1]
    try:
        tok = ops.vocab_top1(Xd, Wv, model.store.w['imgcap_lstm_d2/bias'])
    finally:
        ops._vocab_operands = orig
    assert seen == [Wv.data_ptr()]
    X64 = _f64(Xd)
    want_ids, val, _ = _ref_topk(X64 @ W64 + b64, 1)
    ok = _rule(X64, W64, val)
    np.testing.assert_array_equal(tok.cpu().numpy()[ok], want_ids[ok, 0])
