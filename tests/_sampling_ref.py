"""The float64 restatement of the Gumbel-max sampler (include/dcap.h, dc_vocab_sample_f32) that the sampling
tests compare the device with: Philox-2x32-10 with both output words, the uniform u, the Gumbel noise g and the perturbed argmax.  A
plain module (`import _sampling_ref as S`), NumPy only."""
import numpy as np

_M = np.uint64(0xD256D193)
_W = np.uint64(0x9E3779B9)
_LO = np.uint64(0xFFFFFFFF)
GAP = 1e-4          # a row is undecided when the restatement's two best perturbed values lie closer than this


def philox2x32_pair(c0, c1, key):
    """Philox-2x32-10 on counters (c0, c1) (broadcast together) and one key -> both output words (uint32 arrays)."""
    c0, c1 = np.broadcast_arrays(np.asarray(c0, np.uint64) & _LO, np.asarray(c1, np.uint64) & _LO)
    key = np.uint64(int(key) & 0xFFFFFFFF)
    for _ in range(10):
        p = _M * c0
        c0, c1 = (p >> np.uint64(32)) ^ key ^ c1, p & _LO
        key = (key + _W) & _LO
    return c0.astype(np.uint32), c1.astype(np.uint32)


def noise(seed, offset, rows, cols):
    """g(i, v) float64 [len(rows), len(cols)] for rows i (the counter is offset + i, wrapping at 2^32) and columns v."""
    rows, cols = np.asarray(rows, np.uint64), np.asarray(cols, np.uint64)
    r0, r1 = philox2x32_pair((cols >> np.uint64(1))[None, :], ((np.uint64(offset) + rows) & _LO)[:, None], seed)
    r = np.where((cols & np.uint64(1))[None, :] == 1, r1, r0)
    u = ((r >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    return -np.log(-np.log(u))


def inv_t(temperature):
    """The descriptor's float field, as the wrapper computes it."""
    return float(np.float32(1.0 / float(temperature)))


def perturbed(z, temperature, seed, offset=0):
    """y [M,V] float64 = z * inv_t + g for float64 logits z [M,V] (row i of z is row i of the call)."""
    z = np.asarray(z, np.float64)
    return z * inv_t(temperature) + noise(seed, offset, np.arange(z.shape[0]), np.arange(z.shape[1]))


def choose(y, allowed=None):
    """(ids [M], gap [M]): the argmax of each row of y (the lower column on equal values; NaN never wins; allowed: a boolean [M,V] mask of
    the candidates) and the distance to the second best value (inf with a single candidate).  A row with no candidate gets id 0."""
    y = np.where(np.isnan(y), -np.inf, y)
    if allowed is not None:
        y = np.where(allowed, y, -np.inf)
    ids = np.argmax(y, axis=1)
    if y.shape[1] == 1:
        return ids.astype(np.int64), np.full(y.shape[0], np.inf)
    top2 = np.partition(y, -2, axis=1)[:, -2:]
    with np.errstate(invalid="ignore"):
        gap = top2[:, 1] - top2[:, 0]
    return ids.astype(np.int64), np.where(np.isnan(gap), np.inf, gap)


def softmax_of(z, ids):
    """softmax(z)[i, ids[i]] in float64 (temperature 1, the whole vocabulary): what probs reports."""
    z = np.asarray(z, np.float64)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    return e[np.arange(z.shape[0]), ids] / e.sum(axis=1)


# ---------------------------------------------------------------------------------------------- the caption models, in float64
def decode(step_probs, n, T, temperature, top_k, seed, forced=None, offset0=0):
    """The sampling decoder over n rows and T steps on a float64 model: step_probs(prefixes) -> probabilities [n,V] after each row's
    token prefix (a list of n lists, without the start token).  Step j perturbs log p / temperature (the logits up to a constant per
    row, which no argmax sees) with the noise of offset offset0 + j * n.  forced None: the decoder feeds its own choices (free-running);
    forced int [n,T]: it is fed those tokens instead (teacher forcing: a divergence cannot cascade).  Returns (choice [n,T], gap [n,T]:
    the distance between the two best perturbed values, p [n,T,V])."""
    prefixes = [[] for _ in range(n)]
    choice, gap, ps = np.zeros((n, T), np.int64), np.zeros((n, T)), []
    for j in range(T):
        p = step_probs(prefixes)
        with np.errstate(divide="ignore"):
            y = np.log(p) * inv_t(temperature) + noise(seed, (offset0 + j * n) % 2 ** 32, np.arange(n), np.arange(p.shape[1]))
        allowed = None
        if top_k is not None:
            order = np.argsort(-p, axis=1, kind="stable")[:, :top_k]
            allowed = np.zeros(p.shape, bool)
            np.put_along_axis(allowed, order, True, axis=1)
        choice[:, j], gap[:, j] = choose(y, allowed)
        ps.append(p)
        fed = choice[:, j] if forced is None else forced[:, j]
        for r in range(n):
            prefixes[r].append(int(fed[r]))
    return choice, gap, np.stack(ps, axis=1)


def v1_step_probs(Wt, feat, T):
    """step_probs of the Model-3 decoder (oracle.np_models.v1_word_model_forward on [1, prefix..., 0...])."""
    from oracle import np_models as M
    f, _ = M.roi_head_forward(feat, Wt)

    def step(prefixes):
        ctx = np.zeros((len(prefixes), T))
        ctx[:, 0] = 1
        for r, s in enumerate(prefixes):
            ctx[r, 1:1 + len(s)] = s
        return M.v1_word_model_forward(Wt, f, ctx)[0]
    return step


def v2_step_probs(Wt, feat, Tw, inject, start=None):
    """step_probs of the v2 decoders (oracle.np_models.v2_forward on the pre-padded [start, prefix...])."""
    from oracle import np_models as M
    first = [0] * len(feat) if start is None else [int(s) for s in start]
    return lambda prefixes: M.v2_forward(Wt, feat, M.pad_sequences_pre([[first[r]] + s for r, s in enumerate(prefixes)], Tw), inject)[0]
