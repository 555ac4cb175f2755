"""The two on-device decode loops every caption model shares, greedy() and beam(), with their packed output buffers, and the argument
rules common to the models' check_decoder.  No model knowledge (a model describes one decode call as a Decode) and no host synchronisation."""
import collections

import numpy as np
import torch

from . import ops

DECODERS = ("prefix", "incremental", "beam", "sampling")
SCORES = ("prob", "logprob")


def check_decoder(decoder, beam_size, score, beam_only=None, own=None, score_for_beam_only=False):
    """The argument rules the models share, in their order of refusal: a known decoder; beam_size an integer (not a bool) in
    1..ops.TOPK_MAX with decoder='beam', and neither it nor any of beam_only ({name: value}: the model's further beam-only arguments)
    given otherwise; then own (the model's own refusal at this place: its message, or None); then a known score (score_for_beam_only:
    asked of 'beam' alone).  The sampling arguments have their own rules, check_sampling, which the models apply after all of theirs."""
    if decoder not in DECODERS:
        raise ValueError("decoder must be one of %s, got %r" % (DECODERS, decoder))
    beam_only = dict(beam_size=beam_size, **(beam_only or {}))
    if decoder == "beam":
        if beam_size is None or isinstance(beam_size, bool) or int(beam_size) != beam_size or not 1 <= beam_size <= ops.TOPK_MAX:
            raise ValueError("decoder='beam' needs beam_size in 1..%d, got %r" % (ops.TOPK_MAX, beam_size))
    elif any(v is not None for v in beam_only.values()):
        raise ValueError("%s %s only for decoder='beam' (got decoder=%r)" % (" and ".join(beam_only), "are" if len(beam_only) > 1 else "is", decoder))
    if own is not None:
        raise ValueError(own)
    if (decoder == "beam" or not score_for_beam_only) and score not in SCORES:
        raise ValueError("score must be one of %s, got %r" % (SCORES, score))


def check_sampling(decoder, temperature, top_k, seed):
    """The rules of decoder='sampling' (the models call this after every other refusal) -> (temperature, top_k, seed) as greedy()'s
    sampler takes them.  temperature, top_k and seed belong to 'sampling' alone.  With it, seed is required: an integer (not a bool) in
    [0, 2^32) -- there is no hidden generator state, the same call twice draws the same captions; temperature (default 1.0) is a finite
    number > 0; top_k is None (the whole vocabulary) or an integer (not a bool) in 1..ops.TOPK_MAX."""
    if decoder != "sampling":
        given = [n for n, v in (("temperature", temperature), ("top_k", top_k), ("seed", seed)) if v is not None]
        if given:
            raise ValueError("%s %s only for decoder='sampling' (got decoder=%r)" % (" and ".join(given), "are" if len(given) > 1 else "is", decoder))
        return None
    if seed is None or isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 32:
        raise ValueError("decoder='sampling' needs seed, an integer in [0, 2^32), got %r" % (seed,))
    temperature = 1.0 if temperature is None else temperature
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float, np.integer, np.floating)) or \
            not (np.isfinite(temperature) and temperature > 0):
        raise ValueError("temperature must be a finite number > 0, got %r" % (temperature,))
    if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or not 1 <= top_k <= ops.TOPK_MAX):
        raise ValueError("top_k must be None or an integer in 1..%d, got %r" % (ops.TOPK_MAX, top_k))
    return float(temperature), None if top_k is None else int(top_k), int(seed)


def sampler(n, temperature, top_k, seed, offset0=0):
    """greedy()'s per-step selection that draws every word instead of taking the best: ops.vocab_sample with the noise of step j over the
    n rows at offset offset0 + j * n (so no two (step, row) cells of a call share noise, and a caller that decodes several calls with
    one seed spaces their offset0 by n * T)."""
    def select(j, x, W, bias, **out):
        ops.vocab_sample(x, W, bias, temperature=temperature, top_k=top_k, seed=seed, offset=(offset0 + j * n) % 2 ** 32, **out)
    return select


def _top1(j, x, W, bias, **out):
    ops.vocab_top1(x, W, bias, **out)


# One decode call over n rows, as a model's setup hands it to the drivers:
#   buf, prefix   the model's scratch cache, buf(key, shape, dtype=float32) -> tensor, and the key prefix of this call's buffers
#   tok, live     int32 [n]: the start tokens, then each step's chosen words (the selection ops write them); uint8 [n]: tok != 0
#   mask0         the first step's mask (None: no row is masked); every later step's is live
#   states        two sets of carried-state tensors [n, units] (the same number in each)
#   step          step(tok, mask, prev, cur): the model's launches for one token -- the state set prev (None: zeros) takes tok where mask is
#                 set, into the set cur -- returning the vocabulary layer's input [n, K];  vocab: that layer's (W [K,V], bias [V])
Decode = collections.namedtuple("Decode", "buf prefix tok live mask0 states step vocab")


def _f32(x):
    return x.view(torch.float32 if isinstance(x, torch.Tensor) else np.float32)


def greedy_views(out):
    """(ids int32 [n,T], word scores float32 [n,T]) of greedy()'s [2,n,T] buffer, on the device or (after out.cpu().numpy()) on the host."""
    return out[0], _f32(out[1])


def beam_views(out, B, k, T):
    """(tokens int32 [B,k,T], scores float32 [B,k]) of beam()'s flat buffer, on the device or on the host."""
    return out[:B * k * T].reshape(B, k, T), _f32(out[B * k * T:]).reshape(B, k)


def greedy(n, T, device, setup, select=_top1):
    """T greedy steps over n rows into one int32 [2,n,T] device buffer, [0] the ids, [1] the word scores' float32 bits: per step the
    model's step (setup() -> Decode, called when there are rows), then ops.vocab_top1 into column j and into tok / live for the next
    step.  The steps write the two state sets in turn.  select(j, x, W, bias, tokens=, ids=, probs=, mask=) is the per-step selection:
    the default is that ops.vocab_top1 call; sampler() draws the words instead (decoder='sampling')."""
    out = torch.empty((2, n, T), dtype=torch.int32, device=device)
    if n == 0:
        return out
    d = setup()
    ids, scores = greedy_views(out)
    W, bias = d.vocab
    for j in range(T):
        x = d.step(d.tok, d.live if j else d.mask0, d.states[(j + 1) % 2] if j else None, d.states[j % 2])
        select(j, x, W, bias, tokens=d.tok, ids=ids[:, j], probs=scores[:, j], mask=d.live)
    return out


def beam(B, k, T, device, setup, log_score, end_id=None):
    """T beam-search steps over the n = k*B beam-major rows (beam b of item r = row b*B + r) into one flat int32 device buffer, the [B,k,T]
    tokens, then the [B,k] scores' float32 bits: the model's step writes state set S = states[0], ops.vocab_topk proposes every beam's k
    words, ops.beam_step keeps the k best per item (the first step: of beam 0's alone, from score 0; end_id: see there), writes their words
    into tok / live and gathers their parents' rows of S into G = states[1], which the next step reads (the last step gathers nothing and
    writes the final scores); ops.beam_backtrace then unrolls the history."""
    n = k * B
    out = torch.empty((n * (T + 1),), dtype=torch.int32, device=device)
    if n == 0:
        return out
    d = setup()
    p = d.prefix
    tokens, final = beam_views(out, B, k, T)
    S, G = d.states
    parents, hist = d.buf(p + 'par', (T, B, k), torch.int32), d.buf(p + 'hist', (T, B, k), torch.int32)
    sc = [d.buf(p + 'sc%d' % q, (B, k)) for q in range(2)]
    fin = [d.buf(p + 'fin%d' % q, (n,), torch.uint8) for q in range(2)] if end_id is not None else None
    cids, cprobs = d.buf(p + 'cid', (n, k), torch.int32), d.buf(p + 'cp', (n, k))
    W, bias = d.vocab
    for j in range(T):
        first, last = j == 0, j + 1 == T
        x = d.step(d.tok, d.mask0 if first else d.live, None if first else G, S)
        ops.vocab_topk(x, W, bias, k, ids=cids, probs=cprobs)
        end = {} if fin is None else dict(end_id=int(end_id), finished_in=None if first else fin[j % 2], finished_out=fin[(j + 1) % 2])
        ops.beam_step(cids, cprobs, None if first else sc[j % 2], final if last else sc[(j + 1) % 2], parents, hist, j, 1 if first else k,
                      log_score, tokens=d.tok, mask=d.live, rows=() if last else tuple(zip(S, G)), **end)
    ops.beam_backtrace(parents, hist, out=tokens)
    return out
