"""Beam search for the Model-3 decoder (CaptionModelV1, two 512-unit LSTMs) and the joint model, on the device: ops.beam_step (the
beam-selection kernel with row sets and an end token) against a NumPy restatement on planted candidates, CaptionModelV1.decode_beam /
generate(decoder='beam') against decode_greedy (one beam) and against a float64 beam loop over oracle.np_models (roi_head_forward +
v1_word_model_forward on post-padded prefixes), the structure and edge cases, and DenseImageCapRCNN.generate_captions(decoder='beam')."""
import collections

import numpy as np
import pytest
import torch

from _decode_cases import _dev, _feat, joint_model, record_host_syncs, v1_model
from oracle import np_models as M


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------- the kernel
def _np_beam_step(cid, cp, sin, nb, log, end_id=None, fin=None):
    """The step restated: per RoI the candidates (score, parent, word) -- a finished beam's single (its score, itself, 0), a live beam's k
    proposals at float32(score + p) or float32(score + float32 log p) -- sorted by (-score, parent, word); the first k.  Returns
    scores [R,k] float32, parents, tokens [R,k], finished [R,k]."""
    R, k = cid.shape[0] // cid.shape[1], cid.shape[1]
    sc, par, tok, fo = np.zeros((R, k), np.float32), np.zeros((R, k), np.int32), np.zeros((R, k), np.int32), np.zeros((R, k), np.uint8)
    for r in range(R):
        c = []
        for b in range(nb):
            base = np.float32(0.0) if sin is None else sin[r, b]
            if fin is not None and fin[b * R + r]:
                c.append((base, b, 0))
                continue
            for i in range(k):
                p = cp[b * R + r, i]
                c.append((np.float32(base + (np.log(p) if log else p)), b, int(cid[b * R + r, i])))
        c.sort(key=lambda x: (-x[0], x[1], x[2]))
        assert len(c) >= k
        for q in range(k):
            sc[r, q], par[r, q], tok[r, q] = c[q]
            fo[r, q] = int((fin is not None and fin[par[r, q] * R + r]) or (end_id is not None and tok[r, q] == end_id))
    return sc, par, tok, fo


def _run_step(cid, cp, sin, nb, log, widths, end_id=None, fin=None, seed=0):
    """ops.beam_step on fresh buffers (outputs pre-filled with sentinels) -> host copies of everything it wrote, and the row sets."""
    from image_captioning_amd import ops
    k = cid.shape[1]
    R = cid.shape[0] // k
    rng = np.random.default_rng(seed)
    src = [rng.standard_normal((k * R, U)).astype(np.float32) for U in widths]
    dst = [torch.full((k * R, U), -7.0, device="cuda:0") for U in widths]
    par, hist = (torch.full((2, R, k), -1, dtype=torch.int32, device="cuda:0") for _ in range(2))
    so = torch.full((R, k), 99.0, device="cuda:0")
    tok = torch.full((k * R,), -1, dtype=torch.int32, device="cuda:0")
    mask, fo = (torch.full((k * R,), 9, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    end = {} if end_id is None else dict(end_id=end_id, finished_in=None if fin is None else _dev(fin, torch.uint8), finished_out=fo)
    ops.beam_step(_dev(cid, torch.int32), _dev(cp), None if sin is None else _dev(sin), so, par, hist, 1, nb, log, tokens=tok, mask=mask,
                  rows=[(_dev(s), d) for s, d in zip(src, dst)], **end)
    torch.cuda.synchronize()
    assert np.all(par[0].cpu().numpy() == -1) and np.all(hist[0].cpu().numpy() == -1)          # only step j = 1 of the history is written
    return dict(scores=so.cpu().numpy(), parents=par[1].cpu().numpy(), tokens_hist=hist[1].cpu().numpy(), tokens=tok.cpu().numpy(),
                mask=mask.cpu().numpy(), finished=fo.cpu().numpy(), src=src, dst=[d.cpu().numpy() for d in dst])


def _check_step(got, want, R, k, log, end):
    sc, par, tok, fo = want
    if log:               # the device's logf and NumPy's float32 log may differ in the last place; the order was checked exactly
        np.testing.assert_allclose(got["scores"], sc, rtol=1e-6, atol=1e-6)
    else:
        np.testing.assert_array_equal(got["scores"].view(np.int32), sc.view(np.int32))
    np.testing.assert_array_equal(got["parents"], par)
    np.testing.assert_array_equal(got["tokens_hist"], tok)
    np.testing.assert_array_equal(got["tokens"].reshape(k, R).T, tok)                         # beam-major rows q * R + r
    np.testing.assert_array_equal(got["mask"].reshape(k, R).T, (tok != 0).astype(np.uint8))
    if end:
        np.testing.assert_array_equal(got["finished"].reshape(k, R).T, fo)
    else:
        assert np.all(got["finished"] == 9)                                                   # not written without an end token
    rows = (par * R + np.arange(R)[:, None]).T.reshape(-1)                                    # source row of destination row q * R + r
    for s, d in zip(got["src"], got["dst"]):
        np.testing.assert_array_equal(d.view(np.int32), s[rows].view(np.int32))


def _planted(rng, R, k, log, words=12):
    """Candidate rows with many exact ties: distinct word ids per row from a small range, probabilities on a dyadic grid (multiples of
    1/64; powers of two under the log rule, whose equal inputs give equal logs), scores_in on the same grid with repeats."""
    cid = np.stack([rng.permutation(max(words, k))[:k] for _ in range(k * R)]).astype(np.int32)
    if log:
        cp = (2.0 ** -rng.integers(0, 4, (k * R, k))).astype(np.float32)
        sin = -rng.integers(1, 3, (R, k)).astype(np.float32)
    else:
        cp = (rng.integers(1, 9, (k * R, k)) / 64.0).astype(np.float32)
        sin = (rng.integers(0, 3, (R, k)) / 64.0).astype(np.float32)
    return cid, cp, sin


WIDTHS = [(), (8,), (8, 12), (8, 12, 516, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("widths", WIDTHS, ids=["0 sets", "1 set", "2 sets", "4 sets"])
@pytest.mark.parametrize("k", [1, 2, 8])
def test_beam_step_against_numpy(gpu, k, widths):
    """R = 5, k in {1, 2, 8} (k = nb = 8 fills the 64 lanes), no / one / two / four row sets of different widths (one above 64 float4
    chunks).  The first step (one beam, no scores_in), planted ties on score and on parent under both score rules, and the end token:
    everything equals the restatement, bit for bit (scores under the log rule to 1e-6: logf is not NumPy's log)."""
    R = 5
    rng = np.random.default_rng(100 * k + len(widths))
    for log in (False, True):
        cid, cp, sin = _planted(rng, R, k, log)
        got = _run_step(cid, cp, None, 1, log, widths)                                        # first step
        _check_step(got, _np_beam_step(cid, cp, None, 1, log), R, k, log, False)
        assert np.all(got["parents"] == 0)
        if k > 1:
            b0, b1 = np.arange(k) * R, np.arange(k) * R + 1
            sin[0], cp[b0] = sin[0, 0], 1.0 if log else 0.5                                   # RoI 0: every candidate ties: beam 0's words by id
            sin[1], cp[b1, 0], cp[b1, 1:] = sin[1, 0], 1.0 if log else 0.5, 1.0 / 128         # RoI 1: the beams' first words tie: by parent
        got = _run_step(cid, cp, sin, k, log, widths, seed=1)                                 # ties
        want = _np_beam_step(cid, cp, sin, k, log)
        _check_step(got, want, R, k, log, False)
        if k > 1:
            tied = want[0][:, 1:] == want[0][:, :-1]
            assert tied[:2].all() and np.all(want[1][0] == 0) and np.all(want[1][1] == np.arange(k))     # the planted ties are the kept beams
            assert np.all((want[1][:, 1:] >= want[1][:, :-1])[tied])                          # ... ordered by parent,
            same = tied & (want[1][:, 1:] == want[1][:, :-1])
            assert np.all((want[2][:, 1:] > want[2][:, :-1])[same])                           # ... then by word id
    # the end token: RoI 0 all finished, RoI 1 none, the rest mixed; the finished beams' candidate rows are poisoned
    end_id = 3
    for log in (False, True):
        cid, cp, sin = _planted(rng, R, k, log, words=6)
        fin = rng.integers(0, 2, (k, R)).astype(np.uint8)
        fin[:, 0], fin[:, 1] = 1, 0
        if k > 1:
            fin[0, 2], fin[1, 2] = 1, 0
            sin[2, 0] = 0.0 if log else 1.0                                                   # RoI 2's finished beam 0 leads: it is kept
        fin = fin.reshape(-1)
        cid[1] = [end_id] + [w for w in range(max(6, k) + 1) if w != end_id][:k - 1]          # RoI 1's live beam 0 leads with the end word
        cp[1, 0], cp[1, 1:], sin[1, 0] = (1.0, 1.0 / 128, 0.0) if log else (0.5, 1.0 / 128, 1.0)
        cp[fin == 1], cid[fin == 1] = np.nan, 1 << 30
        got = _run_step(cid, cp, sin, k, log, widths, end_id, fin, seed=2)
        want = _np_beam_step(cid, cp, sin, k, log, end_id, fin)
        _check_step(got, want, R, k, log, True)
        sc, par, tok = got["scores"], got["parents"], got["tokens_hist"]
        fo, mask = got["finished"].reshape(k, R).T, got["mask"].reshape(k, R).T
        assert np.all(np.isfinite(sc)) and tok.max() <= max(6, k)
        for r in range(R):
            for b in range(k):
                q = np.flatnonzero(par[r] == b)
                if fin[b * R + r]:            # proposes itself once: token 0, the score unchanged, stays finished, its state is carried
                    assert q.size <= 1
                    for x in q:
                        assert tok[r, x] == 0 and sc[r, x].view(np.int32) == sin[r, b].view(np.int32) and fo[r, x] == 1 and mask[r, x] == 0
                else:
                    for x in q:
                        assert fo[r, x] == (tok[r, x] == end_id)
        assert np.all(fo[0] == 1) and np.all(tok[0] == 0) and sorted(par[0]) == list(range(k))     # all finished: every beam kept as it is
        np.testing.assert_array_equal(fo[1], tok[1] == end_id)
        assert par[1, 0] == 0 and tok[1, 0] == end_id and fo[1, 0] == 1 and mask[1, 0] == 1      # a live beam that picks the end word is finished
        if k > 1:
            assert (par[2] == 0).sum() == 1


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 8])
def test_beam_select_and_beam_step_are_one_kernel(gpu, k):
    """ops.beam_select and ops.beam_step with the same two row sets and no end token: identical outputs, bit for bit."""
    from image_captioning_amd import ops
    R, U = 5, 516
    rng = np.random.default_rng(7 + k)
    for log in (False, True):
        cid, cp, sin = _planted(rng, R, k, log)
        h, c = (rng.standard_normal((k * R, U)).astype(np.float32) for _ in range(2))
        outs = []
        for fn in ("select", "step"):
            par, hist = (torch.full((3, R, k), -1, dtype=torch.int32, device="cuda:0") for _ in range(2))
            so, ho, co = torch.zeros((R, k), device="cuda:0"), torch.zeros((k * R, U), device="cuda:0"), torch.zeros((k * R, U), device="cuda:0")
            tok = torch.zeros((k * R,), dtype=torch.int32, device="cuda:0")
            mask = torch.zeros((k * R,), dtype=torch.uint8, device="cuda:0")
            args = (_dev(cid, torch.int32), _dev(cp), _dev(sin), so, par, hist, 2, k, log)
            if fn == "select":
                ops.beam_select(*args, tokens=tok, mask=mask, h_in=_dev(h), c_in=_dev(c), h_out=ho, c_out=co)
            else:
                ops.beam_step(*args, tokens=tok, mask=mask, rows=[(_dev(h), ho), (_dev(c), co)])
            outs.append([t.cpu().numpy() for t in (so, par, hist, tok, mask, ho, co)])
        for a, b in zip(*outs):
            np.testing.assert_array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)
        rows = (outs[0][1][2] * R + np.arange(R)[:, None]).T.reshape(-1)
        np.testing.assert_array_equal(outs[0][5], h[rows])


# ---------------------------------------------------------------------------------------------- models and float64 loops
_MODELS = {}


def _v1(V, T, scale=1.0, dtype="f32", seed=70):
    """The Model-3 decoder on synthetic weights (as tests/test_gpu_decode._v1), the vocabulary kernel scaled by `scale` (more peaked word
    distributions: clearer decisions).  One model per configuration for the whole module; returns (model, float64 weights)."""
    key = (V, T, scale, dtype, seed)
    if key not in _MODELS:
        model = v1_model(V, T, 32, seed, compute_dtype=dtype, scale=scale)
        _MODELS[key] = (model, {k: v.astype(np.float64) for k, v in model.get_weights_dict().items()})
    return _MODELS[key]


def _post_pad(seqs, T):
    out = np.zeros((len(seqs), T))
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out


def _oracle_beam(Wt, feat, T, k, log, end_id=None):
    """The beam loop in float64, batched over the RoIs' live beams: start [1]; a live beam proposes its k most probable words after its
    post-padded prefix (score + p, or + log p), a finished beam (its last word is end_id) the single candidate (0, its score); the k best
    in the order (-score, parent, word) survive.  Returns per RoI the k (tokens [T], score, steps until finished or T) best first and the
    smallest margin of any keep/drop decision (a word proposed or not within a live beam, a candidate kept or dropped), in score units."""
    f = np.log if log else (lambda x: x)
    fr, _ = M.roi_head_forward(feat, Wt)
    R = len(feat)
    beams = [[([1], 0.0, None)] for _ in range(R)]                       # (sequence, score, length when finished)
    margin = np.full(R, np.inf)
    for j in range(T):
        flat = [(r, b) for r in range(R) for b in range(len(beams[r])) if beams[r][b][2] is None]
        cands = [[(sc, b, 0, seq + [0], n) for b, (seq, sc, n) in enumerate(beams[r]) if n is not None] for r in range(R)]
        if flat:
            p, _ = M.v1_word_model_forward(Wt, fr[[r for r, _ in flat]], _post_pad([beams[r][b][0] for r, b in flat], T))
            for (r, b), row in zip(flat, p):
                order = np.argsort(-row, kind="stable")
                margin[r] = min(margin[r], f(row[order[k - 1]]) - f(row[order[k]]))
                seq, sc, _ = beams[r][b]
                cands[r] += [(sc + f(row[w]), b, int(w), seq + [int(w)], j + 1 if end_id is not None and w == end_id else None) for w in order[:k]]
        for r in range(R):
            c = sorted(cands[r], key=lambda x: (-x[0], x[1], x[2]))
            if len(c) > k:
                margin[r] = min(margin[r], c[k - 1][0] - c[k][0])
            beams[r] = [(x[3], x[0], x[4]) for x in c[:k]]
    return [[(np.array(s[1:], np.int32), sc, T if n is None else n) for s, sc, n in beams[r]] for r in range(R)], margin


def _rescore(Wt, feat, tokens, log, end_id=None):
    """float64 score of given sequences tokens [R,k,T]: the sum of p (or log p) of each token after its prefix, up to and including the
    first end_id; also whether every token after the end word is 0."""
    f = np.log if log else (lambda x: x)
    R, k, T = tokens.shape
    fr = np.repeat(M.roi_head_forward(feat, Wt)[0], k, axis=0)
    seqs = [[1] + tokens[r, b].tolist() for r in range(R) for b in range(k)]
    total, live, clean = np.zeros(R * k), np.ones(R * k, bool), True
    for j in range(T):
        p, _ = M.v1_word_model_forward(Wt, fr, _post_pad([s[:j + 1] for s in seqs], T))
        nxt = np.array([s[j + 1] for s in seqs])
        total += np.where(live, f(p[np.arange(R * k), nxt]), 0.0)
        clean = clean and bool(np.all(nxt[~live] == 0))
        if end_id is not None:
            live &= nxt != end_id
    return total.reshape(R, k), clean


# ---------------------------------------------------------------------------------------------- one beam is greedy
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_beam_size_1_is_greedy(gpu, dtype):
    """beam_size = 1 without an end token: decode_greedy's ids exactly, the sum of its word scores (atol 1e-6) or of their logs (rtol
    1e-6).  On a bf16 model with vocab_math='bf16' against decode_greedy(vocab_math='bf16'): the beam decoder's whole bf16 check (the top-k
    kernels are held to float64 elsewhere)."""
    V, T, B = 1000, 6, 37
    model, _ = _v1(V, T, dtype=dtype)
    vm = "bf16" if dtype == "bf16" else None
    feat = _feat(52, B)
    ids, scores = model.decode_greedy(feat, vocab_math=vm)
    ids, scores = ids.cpu().numpy(), scores.cpu().numpy().astype(np.float64)
    _, toks, bsc = model.generate(feat, return_probabilities=False, decoder="beam", beam_size=1, vocab_math=vm)
    assert toks.shape == (B, 1, T) and toks.dtype == np.int32 and bsc.shape == (B, 1) and bsc.dtype == np.float32
    np.testing.assert_array_equal(toks[:, 0], ids)
    np.testing.assert_allclose(bsc[:, 0], np.log(scores).sum(1), rtol=1e-6)
    _, toks, bsc = model.generate(feat, return_probabilities=False, decoder="beam", beam_size=1, score="prob", vocab_math=vm)
    np.testing.assert_array_equal(toks[:, 0], ids)
    np.testing.assert_allclose(bsc[:, 0], scores.sum(1), rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------------------- the float64 beam loop
def _check_against_oracle(model, Wt, feat, T, k, score, end_id):
    log = score == "logprob"
    R = len(feat)
    toks_d, sc_d = model.decode_beam(feat, k, score=score, end_id=end_id)
    assert toks_d.is_cuda and toks_d.dtype == torch.int32 and sc_d.dtype == torch.float32
    _, toks, sc = model.generate(feat, return_probabilities=False, decoder="beam", beam_size=k, score=score, end_id=end_id)
    np.testing.assert_array_equal(toks, toks_d.cpu().numpy())
    np.testing.assert_array_equal(sc.view(np.int32), sc_d.cpu().numpy().view(np.int32))
    assert toks.shape == (R, k, T) and sc.shape == (R, k)
    want, margin = _oracle_beam(Wt, feat, T, k, log, end_id)
    re, clean = _rescore(Wt, feat, toks, log, end_id)
    assert clean                                                    # every token after the end word is 0
    tol = 1e-5 * np.maximum(1.0, np.abs(re))
    print("k=%d %s end=%r: max |score - rescore| %.3e, sure %.3f" % (k, score, end_id, np.abs(sc - re).max(), (margin > 1e-5).mean()))
    assert np.all(np.abs(sc - re) < tol), np.abs(sc - re).max()
    assert np.all(np.diff(sc, axis=1) <= 0)
    best = np.array([w[0][1] for w in want])
    assert np.all(re[:, 0] >= best - tol[:, 0])
    sure = margin > 1e-5
    assert sure.mean() >= 0.8, sure.mean()
    for r in np.flatnonzero(sure):
        np.testing.assert_array_equal(toks[r], np.stack([s for s, _, _ in want[r]]))
        assert np.all(np.abs(sc[r] - [x for _, x, _ in want[r]]) < tol[r])
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("score", ["prob", "logprob"])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_decode_beam_against_float64_beam_loop(gpu, k, score):
    """No end token, V = 1000, vocabulary kernel x16.  Every returned score equals the float64 re-score of its own sequence within 1e-5
    (relative to max(1, |score|): a sum of log p carries the fp32 rounding of logits of magnitude ~10 as an absolute error of ~1e-5 at
    scores near -10), the scores are ordered best first, the best is no worse than the oracle's best; on RoIs where every oracle keep/drop
    decision has a margin above 1e-5 (at least 80 %) the sequences and their order are the oracle's."""
    V, T, R = 1000, 6, 32
    model, Wt = _v1(V, T, scale=16.0)
    _check_against_oracle(model, Wt, _feat(72, R), T, k, score, None)


@pytest.mark.gpu
@pytest.mark.parametrize("score", ["prob", "logprob"])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_decode_beam_with_end_token_against_float64_beam_loop(gpu, k, score):
    """The same with an end token, V = 24, vocabulary kernel x8: the end word is the most frequent word at interior positions of the
    oracle's beams without an end token, so that beams do finish in mid-caption (on at least 25 % of the RoIs)."""
    V, T, R = 24, 6, 32
    model, Wt = _v1(V, T, scale=8.0)
    feat = _feat(72, R)
    free, _ = _oracle_beam(Wt, feat, T, k, score == "logprob")
    count = collections.Counter(int(w) for beams in free for s, _, _ in beams for w in s[:-1] if w != 0)
    end_id = count.most_common(1)[0][0]
    want = _check_against_oracle(model, Wt, feat, T, k, score, end_id)
    early = np.mean([any(n < T for _, _, n in beams) for beams in want])
    print("end_id %d, RoIs with a beam finished in mid-caption %.3f" % (end_id, early))
    assert early >= 0.25, early


# ---------------------------------------------------------------------------------------------- structure and edges
def _frequent_interior_word(toks):
    inner = toks[:, :, :-1].reshape(-1)
    return int(np.bincount(inner[inner > 0]).argmax())


@pytest.mark.gpu
def test_decode_beam_is_independent_of_the_batch(gpu):
    """A RoI decoded alone gets the tokens it gets inside a batch of 300 (k = 3, without and with an end token)."""
    V, T, R = 1000, 6, 300
    model, _ = _v1(V, T, scale=16.0)
    feat = _feat(42, R)
    _, free, _ = model.generate(feat, return_probabilities=False, decoder="beam", beam_size=3)
    for end_id in (None, _frequent_interior_word(free)):
        _, toks, _ = model.generate(feat, return_probabilities=False, decoder="beam", beam_size=3, end_id=end_id)
        if end_id is not None:
            assert (toks[:, :, :-1] == end_id).any()
        for r in (0, 1, 150, 299):
            _, one, _ = model.generate(feat[r:r + 1], return_probabilities=False, decoder="beam", beam_size=3, end_id=end_id)
            np.testing.assert_array_equal(one[0], toks[r])


@pytest.mark.gpu
def test_decode_beam_edge_cases(gpu):
    V, T = 1000, 6
    model, _ = _v1(V, T)
    _, toks, sc = model.generate(np.zeros((0, 7, 7, 256), np.float32), return_probabilities=False, decoder="beam", beam_size=4, end_id=2)
    assert toks.shape == (0, 4, T) and sc.shape == (0, 4)
    feat = _feat(82, 3)
    _, toks, sc = model.generate(feat[:1], return_probabilities=False, decoder="beam", beam_size=4)
    assert toks.shape == (1, 4, T) and sc.shape == (1, 4) and np.all(np.diff(sc, axis=1) <= 0) and toks.min() >= 0 and toks.max() < V
    _, all3, _ = model.generate(feat, return_probabilities=False, decoder="beam", beam_size=4)
    np.testing.assert_array_equal(all3[0], toks[0])
    with pytest.raises(ValueError, match="end_id"):
        model.decode_beam(feat, 2, end_id=V)
    # T = 1: a single step (one live beam, no gather): the k most probable first words, in order, with their (log) probabilities
    one, Wt = _v1(V, 1)
    for score, f in (("prob", lambda x: x), ("logprob", np.log)):
        _, toks, sc = one.generate(feat, return_probabilities=False, decoder="beam", beam_size=3, score=score, end_id=2)
        assert toks.shape == (3, 3, 1) and sc.shape == (3, 3)
        p, _ = M.v1_word_model_forward(Wt, M.roi_head_forward(feat, Wt)[0], np.ones((3, 1)))
        np.testing.assert_array_equal(toks[:, :, 0], np.argsort(-p, axis=1, kind="stable")[:, :3])
        np.testing.assert_allclose(sc, f(-np.sort(-p, axis=1)[:, :3]), rtol=1e-5)
    small, _ = _v1(4, T)
    with pytest.raises(ValueError, match="vocabulary"):
        small.decode_beam(feat, 5)
    _, toks, _ = small.generate(feat, return_probabilities=False, decoder="beam", beam_size=4)
    assert toks.shape == (3, 4, T) and toks.min() >= 0 and toks.max() < 4


@pytest.mark.gpu
@pytest.mark.parametrize("score", ["logprob", "prob"])
def test_every_beam_ends_at_once_when_the_end_word_dominates(gpu, score):
    """end_id = 2 on a model whose word-2 bias is raised by 50: every beam takes the end word at step 0 or 1, all later tokens are 0 and
    the scores are finite (log p of the other first words is about -50, not -inf)."""
    V, T, B, k = 1000, 6, 9, 4
    model, _ = _v1(V, T, seed=90)
    bias = model.get_weights_dict()['imgcap_lstm_d2/bias'].copy()
    bias[2] += np.float32(50.0)
    model.load_weights({'imgcap_lstm_d2/bias': bias})
    _MODELS.pop((V, T, 1.0, "f32", 90))                               # (changed: not for sharing)
    _, toks, sc = model.generate(_feat(91, B), return_probabilities=False, decoder="beam", beam_size=k, score=score, end_id=2)
    assert np.all(np.isfinite(sc)) and np.all(np.diff(sc, axis=1) <= 0)
    assert np.all(toks[:, 0, 0] == 2)
    assert np.all((toks[:, :, 0] == 2) | (toks[:, :, 1] == 2))
    assert np.all(toks[:, :, 2:] == 0) and np.all(toks[:, :, 1][toks[:, :, 0] == 2] == 0)


@pytest.mark.gpu
def test_decode_beam_never_syncs_with_the_host(gpu, monkeypatch):
    model, _ = _v1(1000, 6)
    feat = torch.tensor(_feat(51, 5), device="cuda:0")
    model.decode_beam(feat, 3, end_id=2)                    # warm: buffers and workspaces
    calls = record_host_syncs(monkeypatch)
    toks, sc = model.decode_beam(feat, 3, end_id=2)
    toks_p, sc_p = model.decode_beam(feat, 3, score="prob")
    monkeypatch.undo()
    assert calls == []
    for t, s in ((toks, sc), (toks_p, sc_p)):
        assert t.is_cuda and s.is_cuda and t.dtype == torch.int32 and s.dtype == torch.float32
        assert tuple(t.shape) == (5, 3, 6) and tuple(s.shape) == (5, 3)
    _, want, _ = model.generate(feat, return_probabilities=False, decoder="beam", beam_size=3, end_id=2)
    np.testing.assert_array_equal(toks.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------- joint model
@pytest.mark.gpu
def test_joint_model_beam_captions(gpu):
    """generate_captions(decoder='beam', beam_size=3, end_id=2): well-formed results whose rois and ids are what refine_generations gives
    from caption_model.decode_beam's best-beam scores on the same RoI features; with one beam and no end token, the incremental
    decoder's captions (the caption scores that order the NMS well apart)."""
    from image_captioning_amd import synth, dense_model
    S, V, T, k = 128, 24, 5, 3
    model, cfg, _ = joint_model(S, V, T)
    img = synth.images(7, 1, S, S)[0]
    res = model.generate_captions([img], return_probabilities=False, decoder="beam", beam_size=k, end_id=2)
    assert len(res) == 1 and sorted(res[0]) == ["beam_ids", "beam_scores", "ids", "rois"]
    res = res[0]
    K = res["rois"].shape[0]
    assert 0 < K <= 10 and res["rois"].shape == (K, 4) and res["rois"].dtype == np.int32
    assert res["ids"].shape == (K, T) and res["beam_ids"].shape == (K, k, T) and res["beam_scores"].shape == (K, k)
    assert res["ids"].dtype == np.int32 and res["beam_scores"].dtype == np.float32
    np.testing.assert_array_equal(res["ids"], res["beam_ids"][:, 0])
    assert np.all(np.diff(res["beam_scores"], axis=1) <= 0) and np.all(np.isfinite(res["beam_scores"]))
    assert res["beam_ids"].min() >= 0 and res["beam_ids"].max() < V
    for seq in res["beam_ids"].reshape(-1, T):
        e = np.flatnonzero(seq == 2)
        assert e.size <= 1 and (e.size == 0 or np.all(seq[e[0] + 1:] == 0))

    def by_hand(**kw):
        """generate_captions' own steps after the captioner, from decode_beam on the RoI features of the same proposals."""
        props = model.last_proposals
        feats = model.plan().roi_features(boxes_norm=props)
        toks, sc = model.caption_model.decode_beam(feats[0], **kw)
        toks, sc = toks.cpu().numpy(), sc.cpu().numpy()
        _, _, windows = model.mold_inputs([img])
        boxes, keep = dense_model.refine_generations(props[0].cpu().numpy(), None, windows[0], cfg, caption_scores=sc[:, 0])
        final, ok = dense_model.unmold_generations(boxes, img.shape, windows[0])
        return final[ok], toks[keep[ok]], sc[keep[ok]], sc[:, 0]

    rois, toks, sc, _ = by_hand(beam_size=k, end_id=2)
    np.testing.assert_array_equal(res["rois"], rois)
    np.testing.assert_array_equal(res["beam_ids"], toks)
    np.testing.assert_array_equal(res["beam_scores"].view(np.int32), sc.view(np.int32))
    # one beam, no end token: the incremental decoder's captions
    one = model.generate_captions([img], return_probabilities=False, decoder="beam", beam_size=1)[0]
    _, _, _, cap = by_hand(beam_size=1)
    assert np.diff(np.sort(cap.astype(np.float64))).min() > 1e-5               # no near-tie in the NMS order
    light = model.generate_captions([img], return_probabilities=False, decoder="incremental")[0]
    np.testing.assert_array_equal(one["rois"], light["rois"])
    np.testing.assert_array_equal(one["ids"], light["ids"])
    assert one["beam_ids"].shape == (len(light["ids"]), 1, T)
