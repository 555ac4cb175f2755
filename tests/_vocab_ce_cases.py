"""The fused vocabulary loss (dc_vocab_ce, csrc/vocab_ce.hip) and its unfused fallback (dc_softmax_ce_f32, csrc/loss.hip) on EXACT
logits: the cases tests/test_gpu_vocab_ce_elementwise.py runs on the device and tests/test_vocab_ce_cases.py proves on the host.
Plain module, no fixtures; torch and the package are imported nowhere here.

tests/test_gpu_bf16.py and tests/test_gpu_operand_placement.py hold the gradient in max-norm against its LARGEST entry, the target's
p_t - 1 (about 1); every other entry is about 1 / V.  Their slack exists because the float64 oracle and the device may round a logit to
different bf16 neighbours.  Here the operands come from the binary grids of _placement_cases / _bf16_exact_cases (X in steps of 1/8
within +-1, W in steps of 1/256 within +-1/16, the bias in steps of 2^-11): every product is a multiple of 2^-11 and every partial sum
is exact in fp32 for K < 2^17, in any order and on either pipe, so the device's logits EQUAL the float64 logits (asserted on the host).

  1. the row maximum and z_k - m are exact: the device's p_k differs from the oracle's by expf, the row sum and one division only;
  2. on the materialised route the parked logit IS bf16_of(z): no entry rounds the other way; many logits are exact bf16 ties, so
     ties-away in the parking store moves p_k by a whole bf16 ulp of the logit (tie_shares, asserted on the host);
  3. which rows take the CLIP pass and which entries lie outside [1e-7, 1 - 1e-7] is the same on both sides -- no p lies within
     EDGE_MARGIN (relative) of a clip edge (asserted on the host).

THE BOUNDS (u = 2^-24; TINY = 2^-126, the smallest normal fp32 / bf16 number: below it neither format has relative precision and the
hardware exponential may flush, so a term gs * TINY stands beside every relative bound -- it is 1e-31 of the smallest unclipped entry):
  fp32 dlogits   categorical:  |got - want| <= C_G u gs_row (p_k + [k == t])
                 keras_sparse: |got - want| <= C_G u gs_row p_k (u_k / S + [k == t] live / q_t + UP / S + live p_t / q_t)
                 -- relative to the TERMS, not to their difference: p_t -> 1 stays fair;
  bf16 dlogits   the output is a round-to-nearest of SOME fp32 value inside that bound: in ordered bit patterns
                 bf16_round(want - e) <= got <= bf16_round(want + e) (truncation fails on about half of the entries);
  loss_rows      C_L u (1 + |ln q_t|) w_row;
  dbias          C_B u sum_m |g_mk| per column, against the ORACLE's column sums;
  probs          C_G u p_k (softmax_ce).
The constants are 4 x the largest ratio a float32 NumPy stand-in of the same formulas reaches against the float64 oracle on the same
cases, rounded up to one digit (DESIGN.md section 3d's rule; test_vocab_ce_cases.py computes the floors and asserts the rule).  Two
stand-ins: exp="libm" (float32 exp, what dc_softmax_ce_f32's expf is) and exp="fast": the fused kernels call __expf, which the compiler
lowers to exp2(fl32(x * log2 e)) -- the product's rounding is an ABSOLUTE error of half an ulp of |x| log2 e in the exponent, i.e. a
relative error of about |x| u in the result, so a probability e^-30 below the row maximum carries 20 u however good the hardware exp2
is.  That is format reasoning, not a measurement of the device; the fused kernels are held to the "fast" constants."""
import functools

import numpy as np

import _bf16_exact_cases as X
import _placement_cases as P

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
EPS = 1e-7                          # K.epsilon(): the clip range is [EPS, 1 - EPS]
EPS32_LO, EPS32_HI = F32(1e-7), F32(1.0) - F32(1e-7)          # the device's edges (1e-7f, 1.f - 1e-7f)
EDGE_MARGIN = 1e-3
EDGE_MARGIN_HI = 0.5
TIE_SHARE = X.TIE_SHARE
ROUTE_SHARE = 0.5                   # of the entries: the gradients of bf16_of(z) and of z further apart than the bound allows
ROUTE_SHARE_BF16 = 0.1              # ... and still after the bf16 rounding of the output (more than 10^5 entries of every case)
LOG2E = F32(1.4426950408889634)

# The stand-in's floors -- its largest ratio to the unit of each bound, by the exponential the kernel calls and by variation, measured
# by test_vocab_ce_cases.py::test_constants_are_four_times_the_stand_ins_floor -- and the asserted constants:
# 4 x the floor, rounded up to one digit.
FLOOR = {
    "fast": {"categorical":  {"g": 9.67, "loss": 1.28, "dbias": 3.20},
             "sparse none":  {"g": 3.34, "loss": 1.82, "dbias": 3.16},
             "sparse all":   {"g": 3.11, "loss": 2.04, "dbias": 3.24},
             "sparse mixed": {"g": 5.48, "loss": 6.44, "dbias": 3.52}},
    "libm": {"categorical":  {"g": 5.66, "loss": 1.02},
             "sparse none":  {"g": 5.66, "loss": 1.45},
             "sparse all":   {"g": 5.46, "loss": 1.76},
             "sparse mixed": {"g": 5.48, "loss": 6.44}},
}
FLOOR_TOLERANCE = 0.25              # of a recorded floor: float32 exp differs by an ulp between NumPy builds and CPUs


def one_digit_up(x):
    """x rounded up to one significant digit."""
    e = 10.0 ** np.floor(np.log10(x))
    return float(np.ceil(x / e - 1e-9) * e)


CONST = {e: {v: {k: one_digit_up(4.0 * f) for k, f in kinds.items()} for v, kinds in per.items()} for e, per in FLOOR.items()}

SMALL = [(130, 1016, 2048), (264, 1000, 256)]                                   # the 128-square tile: ragged M and V
BIG = [(3000, 4104, 256), (1500, 8200, 512), (1500, 8200, 1024)]                # the 256-square tile (bf16 operands)
SHAPES = SMALL + BIG
VARIATIONS = ["categorical", "sparse none", "sparse all", "sparse mixed"]
# the mixed case's clipped-high row needs sum |W[:, c]| (about K / 32) more than ln(V 1e7) above the row's other logits: K >= 1024
MIXED_K = 1024
HI_COL, PAIR = 5, (7, 9)            # mixed: the clipped-high row's word; the two words the clipped-low row makes equal (W[:, 9] = W[:, 7])
HI_ROW, LO_ROW = 15, 3             # both in the first row tile of either tile size
CLIP_COL = 11                       # "sparse all": the word whose bias is -80
ZERO_ROW, BIAS_ROW = 2, 1           # the zero-weight row (keras_sparse); the row whose X is zero (logits = the bias alone)
BIAS_BOUND = 1.0
CUT = 3                             # softmax_ce's V % 4 != 0 case: the first small shape's columns from here on

# routes: name -> (operand type, gradient type, materialize_bf16, shapes, rows per tile, exponential)
ROUTES = {
    "f32 128":            ("f32", "f32", False, SMALL, 128),
    "bf16 128":           ("bf16", "f32", False, SMALL, 128),
    "bf16 128, bf16 dl":  ("bf16", "bf16", False, SMALL, 128),
    "bf16 256":           ("bf16", "f32", False, BIG, 256),
    "bf16 256, bf16 dl":  ("bf16", "bf16", False, BIG, 256),
    "bf16 256 parked":    ("bf16", "bf16", True, BIG, 256),
}
SOFTMAX_SHAPES = [(130, 1016, 2048), (264, 1000, 256), (37, 1003, 2048)]        # the last: V % 4 != 0 (the scalar loops)


def variations(M, V, K):
    return [v for v in VARIATIONS if v != "sparse mixed" or K >= MIXED_K]


def all_cases(shapes=None):
    return [(M, V, K, v) for (M, V, K) in (shapes or SHAPES) for v in variations(M, V, K)]


def _seed(*key):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(repr(key)))


def _frozen(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def bf16_value(bits):
    """bf16 bit patterns -> their values (float32)."""
    return (np.asarray(bits).astype(np.uint32) << 16).view(F32)


def bf16_of(v, rule="even"):
    """fp32-exact values -> the nearest bf16 value (float32), by X.bf16_round's rule."""
    return bf16_value(X.bf16_round(np.asarray(v, F32), rule))


# ---------------------------------------------------------------------------------------------------------------------------------
# operands and exact logits

@functools.lru_cache(maxsize=3)
def _base(M, V, K):
    assert K < X.K_LIMIT
    rng = np.random.default_rng(_seed("vocab ce", M, V, K))
    Xm = P.grid(rng, (M, K), 1 / 8, 1.0)
    Xm[BIAS_ROW] = 0.0
    W = P.grid(rng, (K, V), 1 / 256, 1 / 16)
    bias = P.grid(rng, (V,), 2.0 ** -11, BIAS_BOUND)
    t = rng.integers(0, V, M).astype(np.int32)
    w = rng.integers(1, 65, M).astype(F64) / 64.0               # row weights in steps of 1/64 within (0, 1]
    w[ZERO_ROW] = 0.0
    return _frozen({"X": Xm, "W": W, "bias": bias, "t": t, "w": w, "z": Xm @ W + bias})


@functools.lru_cache(maxsize=4)
def operands(M, V, K, variation):
    """X [M, K], W [K, V], bias [V], targets t [M], row weights w [M] (None: categorical), grad_scale gs (an fp32 value), the flavour
    and z = X W + bias [M, V], exact in fp32.  The variations change a few rows and columns of the shape's base case."""
    b = _base(M, V, K)
    c = {"M": M, "V": V, "K": K, "variation": variation, "keras_sparse": variation != "categorical", "clipped_rows": ()}
    Xm, W, bias, t, z = b["X"], b["W"], b["bias"], b["t"], b["z"]
    if variation == "categorical":
        c["w"], c["gs"] = None, float(F32(1.0 / M))
    else:
        c["w"], c["gs"] = b["w"], 1.0
    if variation == "sparse all":                               # one word at -80: below 1e-7 in every row; row 4's target
        bias, z, t = bias.copy(), z.copy(), t.copy()
        z[:, CLIP_COL] += -80.0 - bias[CLIP_COL]
        bias[CLIP_COL] = -80.0
        t[4] = CLIP_COL
        c["clipped_rows"] = tuple(range(M))
    elif variation == "sparse mixed":
        assert K >= MIXED_K
        Xm, W, bias, z, t = Xm.copy(), W.copy(), bias.copy(), z.copy(), t.copy()
        W[:, PAIR[1]] = W[:, PAIR[0]]
        bias[PAIR[1]] = bias[PAIR[0]]
        Xm[HI_ROW] = np.where(W[:, HI_COL] < 0, -1.0, 1.0)      # aligned with one word: p > 1 - 1e-7, everything else below 1e-7
        Xm[LO_ROW] = np.where(W[:, PAIR[0]] < 0, -1.0, 1.0)     # aligned with two equal words: p = 1/2 twice, the rest below 1e-7
        t[HI_ROW], t[LO_ROW] = HI_COL, PAIR[0]                  # a clipped-high target (no gradient through it) and a live one
        z[:, PAIR[1]] = Xm @ W[:, PAIR[1]] + bias[PAIR[1]]
        for r in (HI_ROW, LO_ROW):
            z[r] = Xm[r] @ W + bias
        c["clipped_rows"] = tuple(sorted((HI_ROW, LO_ROW)))
    c.update({"X": Xm, "W": W, "bias": bias, "t": t, "z": P.assert_exact_f32(z, "the logits")})
    for name in ("X", "W"):                                     # exact in bf16 as well: the bf16 routes read the same values
        assert np.array_equal(bf16_of(c[name]).astype(F64), c[name]), name
    return _frozen(c)


@functools.lru_cache(maxsize=4)
def softmax_operands(M, V, K, variation):
    """The unfused fallback's input: the grid logits themselves (the two small shapes' own, and a V % 4 != 0 cut of the second)."""
    if (M, V, K) in SMALL:
        return operands(M, V, K, variation)
    src = operands(130, 1016, K, variation)                     # rows 0 .. M - 1, columns CUT .. CUT + V - 1 of the first small shape
    c = dict(src)
    for name in ("t", "w", "z", "X"):
        if c[name] is not None:
            c[name] = c[name][:M]
    c["z"], c["W"], c["bias"] = c["z"][:, CUT:CUT + V], c["W"][:, CUT:CUT + V], c["bias"][CUT:CUT + V]
    c["t"] = np.where((c["t"] >= CUT) & (c["t"] < CUT + V), c["t"] - CUT, c["t"] % V).astype(np.int32)
    if not c["keras_sparse"]:
        c["gs"] = float(F32(1.0 / M))
    c.update({"M": M, "V": V, "clipped_rows": tuple(r for r in c["clipped_rows"] if r < M)})
    c["z"] = np.ascontiguousarray(c["z"])
    return _frozen(c)


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 reference

def _block(a, rows, cols):
    """a[rows][:, cols] (None: all); a itself when both are None."""
    if rows is None and cols is None:
        return a
    if cols is None:
        return a[rows]
    if rows is None:
        return a[:, cols]
    return a[np.ix_(rows, cols)]


def _targets_in_block(t, rows, cols):
    """(block row, block column) of every target that lies inside the block."""
    tr = t if rows is None else t[rows]
    br = np.arange(len(tr))
    if cols is None:
        return br, tr
    pos = np.searchsorted(cols, tr)
    ok = (pos < len(cols)) & (cols[np.minimum(pos, len(cols) - 1)] == tr)
    return br[ok], pos[ok]


def reference_stats(c, z):
    """The whole rows' statistics of the logits z (float64): what every block of reference_from_logits shares."""
    z = np.asarray(z, F64)
    M, V = z.shape
    t = np.asarray(c["t"]).astype(np.int64)
    e = np.exp(z - z.max(-1, keepdims=True))
    s = e.sum(-1)
    pt = e[np.arange(M), t] / s
    st = {"e": e, "s": s, "pt": pt, "live": (pt >= EPS) & (pt <= 1 - EPS), "qt": np.clip(pt, EPS, 1 - EPS), "pmax": e.max(-1) / s}
    st["needs_clip"] = (e.min(-1) / s < EPS) | (st["pmax"] > 1 - EPS)
    st["edge_lo"] = float((np.abs(e - (EPS * s)[:, None]).min(-1) / (EPS * s)).min())
    S, UP = np.ones(M), np.ones(M)                # no probability of the row is clipped: S = UP = sum p = 1
    if c["keras_sparse"]:
        for n in np.nonzero(st["needs_clip"])[0]:
            pn = e[n] / s[n]
            S[n] = np.clip(pn, EPS, 1 - EPS).sum()
            UP[n] = pn[(pn >= EPS) & (pn <= 1 - EPS)].sum()
    st["S"], st["UP"] = S, UP
    return st


def reference_from_logits(c, z, rows=None, cols=None, stats=None):
    """Loss, gradient, bias gradient and probabilities of the logits z (float64) under c's flavour, each with the UNIT of its bound
    (multiply by the constant and u; add TINY * the `tiny` scale).  The row statistics are those of the whole rows (stats: a
    reference_stats(c, z) to share); rows / cols (sorted index arrays) restrict the [M, V] outputs to a block, and the bias gradient
    to the block's rows and columns.  dict with
      p, g, A_g [block];  tiny_g [block rows];  loss, A_loss, needs_clip, live, pt, pmax [M];  dbias, A_dbias [block columns], tiny_dbias."""
    st = stats if stats is not None else reference_stats(c, z)
    M = len(st["s"])
    t = np.asarray(c["t"]).astype(np.int64)
    s, pt, live, qt, S, UP = st["s"], st["pt"], st["live"], st["qt"], st["S"], st["UP"]
    r = {k: st[k] for k in ("live", "needs_clip", "pt", "pmax", "edge_lo")}
    sel = (lambda v: v) if rows is None else (lambda v: v[rows])
    p = _block(st["e"], rows, cols) / sel(s)[:, None]
    bi, bj = _targets_in_block(t, rows, cols)
    if not c["keras_sparse"]:
        w = np.ones(M)
        gs = sel(c["gs"] * live)
        g = p.copy()
        g[bi, bj] -= 1.0
        A = p.copy()
        A[bi, bj] += 1.0
        r["loss"], r["tiny_g"] = -np.log(qt), gs
    else:
        w = np.asarray(c["w"], F64)
        gs = sel(c["gs"] * w)
        tq = live / qt
        back = UP / S + live * pt / qt
        inside = (p >= EPS) & (p <= 1 - EPS)
        g = inside / sel(S)[:, None]
        A = g.copy()
        del inside
        g[bi, bj] -= sel(tq)[bi]
        g -= sel(UP / S - live * pt / qt)[:, None]
        g *= p
        A[bi, bj] += sel(tq)[bi]
        A += sel(back)[:, None]
        A *= p
        r["tiny_g"] = gs * sel(1.0 / S + tq + back)
        r["loss"] = w * (-np.log(qt) + np.log(S))
        r["S"], r["UP"] = S, UP
    g *= gs[:, None]
    A *= gs[:, None]
    r["p"], r["g"], r["A_g"] = p, g, A
    r["A_loss"] = (1.0 + np.abs(np.log(qt))) * w
    r["dbias"], r["A_dbias"], r["tiny_dbias"] = g.sum(0), np.abs(g).sum(0), float(np.sum(r["tiny_g"]))
    return r


def _case_logits(M, V, K, variation, parked, softmax):
    c = softmax_operands(M, V, K, variation) if softmax else operands(M, V, K, variation)
    return c, (bf16_of(c["z"]).astype(F64) if parked else c["z"])


@functools.lru_cache(maxsize=3)
def reference(M, V, K, variation, parked=False, softmax=False):
    """The reference of one case, shared by the routes that compute it: of the exact logits z, or (parked) of bf16_of(z), what the
    materialised route works with.  Read-only."""
    return _frozen(reference_from_logits(*_case_logits(M, V, K, variation, parked, softmax)))


def host_blocks(M, V):
    """The two blocks on which the host measures the stand-in at the large shapes (the row statistics are always the whole rows'):
    whole rows -- the first 128 (the special rows are among them) and the last 64, the ragged tile's -- for the gradient, and whole
    columns -- the first 16 (the special words), 48 more across the row and the last 8 -- for the bias gradient."""
    rows = np.unique(np.concatenate([np.arange(min(M, 128)), np.arange(max(0, M - 64), M)]))
    cols = np.unique(np.concatenate([np.arange(16), np.arange(16, V - 8, max(1, (V - 24) // 48)), np.arange(V - 8, V)]))
    return rows, cols


def clear_caches():
    """Drop every cached case and reference (float64 [M, V] arrays of 100 MB each at the large shapes): the test modules call it
    when they are done, so that nothing of this stays resident for the rest of a suite run."""
    for fn in (_base, operands, softmax_operands, reference):
        fn.cache_clear()


def edge_distance(ref):
    """(lower, upper): the smallest relative distance of any probability from 1e-7, and of 1 - p from 1e-7 for the rows' largest
    probabilities (only a row's largest can be near the upper edge; fp32 resolves 1 - p in steps of 6e-8 only, so the upper distance
    is asked to be EDGE_MARGIN_HI, half of the edge itself)."""
    return ref["edge_lo"], float(np.abs((1.0 - ref["pmax"]) / EPS - 1.0).min())


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparison

class Verdict(object):
    """worst: the largest ratio |got - want| / (u * unit) (after the TINY allowance); bad: how many entries exceed `const`."""

    def __init__(self, what, worst, bad, size, lines):
        self.what, self.worst, self.bad, self.size, self.lines = what, worst, bad, size, lines

    @property
    def ok(self):
        return self.bad == 0

    def report(self):
        return "\n".join(["%s: %d of %d entries outside the bound, worst ratio %.4g" % (self.what, self.bad, self.size, self.worst)] + self.lines)

    def line(self, case):
        return "vocab-ce-elementwise %s %s: worst ratio %.3g (%d of %d outside)" % (case, self.what, self.worst, self.bad, self.size)


def _tiny_like(tiny, shape):
    tiny = np.asarray(tiny, F64)
    return tiny[:, None] if tiny.ndim == 1 and len(shape) == 2 else tiny


def _where_lines(bad, got, want, ratio, n=6):
    lines = []
    for idx in np.argwhere(bad)[:n]:
        at = tuple(int(i) for i in idx)
        lines.append("  at %s: got %.10g want %.10g (ratio %.4g)" % (at, got[at], want[at], ratio[at]))
    return lines


def _ratio(got, want, A, tiny):
    d = np.abs(np.asarray(got, F64) - want)
    d -= TINY * _tiny_like(tiny, d.shape)
    np.maximum(d, 0.0, out=d)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = d / (U * A)
    ratio[(d == 0.0)] = 0.0                                      # a zero unit (a dead row) wants the exact value
    ratio[~np.isfinite(np.asarray(got, F64))] = np.inf
    return ratio


def compare_f32(got, want, A, tiny, const, what):
    """An fp32 output against the oracle: |got - want| <= const u A + TINY tiny, every entry."""
    got, want = np.asarray(got), np.asarray(want, F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ratio = _ratio(got, want, A, tiny)
    bad = ~(ratio <= const)
    return Verdict(what, float(np.nanmax(np.where(np.isnan(ratio), np.inf, ratio))), int(bad.sum()), bad.size,
                   _where_lines(bad, np.asarray(got, F64), want, ratio))


def compare_bf16(got_bits, want, A, tiny, const, what):
    """A bf16 output (bit patterns) against the oracle: the round-to-nearest of some fp32 value within const u A + TINY tiny of want,
    bf16_round(want - e) <= got <= bf16_round(want + e) in ordered bit patterns.  worst: the distance of want from the nearest fp32
    value that rounds to got, in units of u A."""
    got_bits, want = np.asarray(got_bits), np.asarray(want, F64)
    assert got_bits.dtype == np.uint16 and got_bits.shape == want.shape, (what, got_bits.dtype, got_bits.shape, want.shape)
    with np.errstate(invalid="ignore"):
        e = np.nan_to_num(const * U * A, nan=0.0, posinf=np.inf) + TINY * _tiny_like(tiny, want.shape)
    lo = X._ordered(X.bf16_round((want - e).astype(F32)), 16)
    hi = X._ordered(X.bf16_round((want + e).astype(F32)), 16)
    g = X._ordered(got_bits, 16)
    got = bf16_value(got_bits)
    bad = ~((lo <= g) & (g <= hi)) | ~np.isfinite(got)
    half = np.spacing(np.abs(got)).astype(F64) * 2.0 ** 15      # half a bf16 ulp of the value got
    d = np.maximum(np.abs(got.astype(F64) - want) - half, 0.0)
    ratio = _ratio(want + d, want, A, tiny)
    ratio[~np.isfinite(got)] = np.inf
    lines = []
    for idx in np.argwhere(bad)[:6]:
        at = tuple(int(i) for i in idx)
        lines.append("  at %s: got %.8g (0x%04x) want %.10g, allowed 0x%04x .. 0x%04x" %
                     (at, got[at], int(got_bits[at]), want[at], int(X.bf16_round(F32(want[at] - e[at])).ravel()[0]), int(X.bf16_round(F32(want[at] + e[at])).ravel()[0])))
    return Verdict(what, float(ratio.max()), int(bad.sum()), bad.size, lines)


def compare_outputs(ref, const, loss=None, g=None, g_bits=None, dbias=None, probs=None):
    """Every output given against its reference: {name: Verdict}."""
    out = {}
    if loss is not None:
        out["loss_rows"] = compare_f32(loss, ref["loss"], ref["A_loss"], np.zeros(len(ref["loss"])), const["loss"], "loss_rows")
    if g is not None:
        out["dlogits"] = compare_f32(g, ref["g"], ref["A_g"], ref["tiny_g"], const["g"], "dlogits (fp32)")
    if g_bits is not None:
        out["dlogits bf16"] = compare_bf16(g_bits, ref["g"], ref["A_g"], ref["tiny_g"], const["g"], "dlogits (bf16)")
    if dbias is not None:
        out["dbias"] = compare_f32(dbias, ref["dbias"], ref["A_dbias"], ref["tiny_dbias"], const["dbias"], "dbias")
    if probs is not None:
        out["probs"] = compare_f32(probs, ref["p"], ref["p"], np.ones(len(ref["p"])), const["g"], "probs")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the existing tests' assertions, restated as data (tests/test_gpu_bf16.py): True when the output passes them

def old_close(got, want, tol):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    return bool(np.abs(got - want).max() / max(1.0, float(np.abs(want).max())) < tol)


def old_assertions(c, ref, route, loss=None, g=None, g_bits=None, dbias=None, ref_z=None):
    """test_vocab_ce_categorical / _masked_keras_sparse / _bf16_on_the_256_tile (recomputing routes) and
    test_vocab_ce_bf16_materialised_logits (the parked route) on these outputs.  Gradients are compared times M in the categorical
    flavour, as there.  ref_z: the unrounded logits (the parked route's loss and gradient tolerances scale with the row's largest)."""
    scale = 1.0 if c["keras_sparse"] else 1.0 / c["gs"]
    want = ref["g"] * scale
    ok = True
    if not ROUTES[route][2]:
        if loss is not None:
            ok &= old_close(loss, ref["loss"], 3e-5)
        if g is not None:
            ok &= old_close(np.asarray(g, F64) * scale, want, 3e-5)
        if g_bits is not None:
            got = bf16_value(g_bits).astype(F64) * scale
            ok &= bool(np.abs(got - want).max() <= 2.0 ** -8 * np.abs(want).max() + 1e-6)
        if dbias is not None:
            ok &= old_close(np.asarray(dbias, F64) * scale, want.sum(0), 2e-4)
        return bool(ok)
    zmax = np.abs(ref_z).max(axis=1)
    wrow = c["w"] if c["keras_sparse"] else np.ones(c["M"])
    if loss is not None:
        ok &= bool(np.all(np.abs(np.asarray(loss, F64) - ref["loss"]) <= 2.0 ** -7 * wrow * np.maximum(1.0, zmax) + 3e-5))
    if g_bits is not None:
        got = bf16_value(g_bits).astype(F64) * scale
        gmax = np.abs(want).max()
        err = np.abs(got - want)
        ok &= bool(err.max() <= (2.0 ** -7 * max(1.0, float(zmax.max())) / 2 + 2.0 ** -8) * gmax + 1e-6)
        ok &= bool(np.median(err.max(axis=1)) <= 2.0 ** -8 * gmax + 1e-6)
        if not c["clipped_rows"]:
            ok &= bool(np.abs(got.sum(axis=1)).max() <= 2.0 ** -8 * np.abs(got).sum(axis=1).max() + 1e-6)
        if dbias is not None:                                    # against the column sums of the gradient the kernel itself wrote
            ok &= old_close(np.asarray(dbias, F64) * scale, got.sum(0), 2e-3)
    return bool(ok)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in float32 NumPy, right or wrong on purpose (host only)

def _exp32(x, mode):
    x = np.asarray(x, F32)
    with np.errstate(under="ignore"):
        if mode == "libm":
            return np.exp(x)
        assert mode == "fast"
        return np.exp2(x * LOG2E)


def _tiles(a, fill, width=128):
    """[M, V] -> [M, tiles, width], the last tile padded with `fill`."""
    M, V = a.shape
    n = -(-V // width)
    if n * width != V:
        a = np.concatenate([a, np.full((M, n * width - V), fill, a.dtype)], axis=1)
    return a.reshape(M, n, width)


def _ordered_sum(parts):
    """Float32 partial sums [M, tiles] combined in ce_rows_kernel's fixed order: 64 lanes stride the tiles (lane l adds tiles l,
    l + 64, ... in order), then a butterfly over the lanes (32, 16, ..., 1).  (Tile after tile on ONE accumulator is a fixed order as
    well, but not the kernel's: the 64 partials of 1.28e-5 of the mixed case's row of two halves, added onto 1.0000126, lose the same
    0.37 ulp each -- 42 u on that row's loss from the order alone.)"""
    M, n = parts.shape
    lanes = np.zeros((M, 64), F32)
    for j0 in range(0, n, 64):
        k = min(64, n - j0)
        lanes[:, :k] = lanes[:, :k] + parts[:, j0:j0 + k]
    o = 32
    while o:
        lanes = lanes[:, :o] + lanes[:, o:2 * o]
        o >>= 1
    return lanes[:, 0]


def standin_stats(c, parked=False, exp="fast", tile_rows=128, park_rule="even", neighbours_of=None):
    """The whole rows' part of standin(): the logits as the route reads them, m, 1 / s and the row kernel's constants."""
    # The clip sums below follow the GEMM CLIP pass (128-column partials, then _ordered_sum) on every route.  The parked route's own
    # sums are ce_rows_kernel's walk of the parked logits -- one accumulator per lane, 8 words a step, the words clipped low counted --
    # which is NOT modelled here: for clipped rows the parked route's floor is borrowed from the tile-partial order.
    z = np.asarray(c["z"], F32)
    if parked:
        z = bf16_of(z, park_rule)
    M, V = z.shape
    t = np.asarray(c["t"]).astype(np.int64)
    zt = _tiles(z, F32(-np.inf))
    mj = zt.max(-1)
    sj = _exp32(zt - mj[..., None], exp).sum(-1, dtype=F32)
    del zt
    m = mj.max(-1)
    s = _ordered_sum(sj * _exp32(mj - m[:, None], exp))
    inv_s = F32(1.0) / s
    pt = _exp32(z[np.arange(M), t] - m, exp) * inv_s
    live = (pt >= EPS32_LO) & (pt <= EPS32_HI)
    qt = np.minimum(np.maximum(pt, EPS32_LO), EPS32_HI)
    pmin = _exp32(z.min(-1) - m, exp) * inv_s
    needs = ~((pmin >= EPS32_LO) & (inv_s <= EPS32_HI))
    st = {"z": z, "m": m, "inv_s": inv_s, "pt": pt, "live": live, "qt": qt, "needs_clip": needs, "exp": exp, "tile_rows": tile_rows}
    if not c["keras_sparse"]:
        st["gs"] = np.where(live, F32(c["gs"]), F32(0.0)).astype(F32)
        st["loss"] = -np.log(qt)
        return st
    w = np.asarray(c["w"], F32)
    S, UP = np.ones(M, F32), np.ones(M, F32)
    if needs.any():
        n = np.nonzero(needs)[0]
        pn = _exp32(z[n] - m[n, None], exp) * inv_s[n, None]
        S[n] = _ordered_sum(_tiles(np.minimum(np.maximum(pn, EPS32_LO), EPS32_HI), F32(0)).sum(-1, dtype=F32))
        UP[n] = _ordered_sum(_tiles(np.where((pn >= EPS32_LO) & (pn <= EPS32_HI), pn, F32(0)), F32(0)).sum(-1, dtype=F32))
    if neighbours_of is not None:
        r0 = neighbours_of // tile_rows * tile_rows
        other = np.arange(r0, min(M, r0 + tile_rows))
        other = other[~needs[other]]
        S[other], UP[other] = S[neighbours_of], UP[neighbours_of]
    livef = live.astype(F32)
    st["invS"] = F32(1.0) / S
    st["cc"] = UP * st["invS"] - livef * (pt / qt)
    st["tq"] = livef * (F32(1.0) / qt)
    st["gs"] = (F32(c["gs"]) * w).astype(F32)
    st["loss"] = w * (-np.log(qt) + np.log(S))
    return st


def standin(c, parked=False, exp="fast", tile_rows=128, park_rule="even", neighbours_of=None, rows=None, cols=None, stats=None):
    """dc_vocab_ce's formulas in float32: logits (exact; parked: rounded to bf16 by park_rule) -> per-tile maxima and sums of exp over
    128 columns combined in the row kernel's order (_ordered_sum), 1 / s, p = exp(z - m) * (1 / s), the row kernel's constants, the gradient expression, column sums
    in per-row-tile partials combined in order.  neighbours_of = row: every unclipped row of that row's tile takes ITS S and UP (a
    planted error).  rows / cols / stats: as reference_from_logits (stats: a standin_stats of the same arguments).
    -> dict loss, needs_clip [M]; p, g [block], g_bits (the bf16 copy), dbias [block columns]; all float32."""
    st = stats if stats is not None else standin_stats(c, parked, exp, tile_rows, park_rule, neighbours_of)
    exp, tile_rows = st["exp"], st["tile_rows"]
    M = len(st["m"])
    t = np.asarray(c["t"]).astype(np.int64)
    sel = (lambda v: v) if rows is None else (lambda v: v[rows])
    p = _exp32(_block(st["z"], rows, cols) - sel(st["m"])[:, None], exp) * sel(st["inv_s"])[:, None]
    assert p.dtype == F32
    bi, bj = _targets_in_block(t, rows, cols)
    if not c["keras_sparse"]:
        g = p.copy()
        g[bi, bj] -= F32(1.0)
        g *= sel(st["gs"])[:, None]
    else:
        g = np.where((p >= EPS32_LO) & (p <= EPS32_HI), sel(st["invS"])[:, None], F32(0))
        g[bi, bj] -= sel(st["tq"])[bi]
        g -= sel(st["cc"])[:, None]
        g = sel(st["gs"])[:, None] * p * g
    assert g.dtype == F32 and st["loss"].dtype == F32
    return {"loss": st["loss"], "g": g, "g_bits": X.bf16_round(g), "dbias": column_sums(g, rows, M, tile_rows), "p": p,
            "needs_clip": st["needs_clip"]}


def _tree_sum_rows(a):
    """Float32 sum over the rows by halving (neighbours first): the order of a shuffle reduction, whatever the array's layout."""
    a = np.ascontiguousarray(a, F32)
    while a.shape[0] > 1:
        if a.shape[0] % 2:
            a = np.concatenate([a, np.zeros((1, a.shape[1]), F32)])
        a = a[0::2] + a[1::2]
    return a[0]


def column_sums(g, rows, M, tile_rows):
    """The bias gradient of a float32 gradient block: a tree sum inside every row tile, the tiles' partials combined in order."""
    rsel = np.arange(M) if rows is None else rows
    dbias = np.zeros(g.shape[1], F32)
    for r0 in range(0, M, tile_rows):                           # the block's rows, in the row tiles they belong to
        k0, k1 = np.searchsorted(rsel, [r0, r0 + tile_rows])
        if k1 > k0:
            dbias = dbias + _tree_sum_rows(g[k0:k1])
    return dbias
