"""The instrument of tests/test_gpu_vocab_ce_elementwise.py, proved on the host (no GPU, no library): the cases are what the device
test takes them for -- exact logits, bf16 ties on either side of round-to-even, no probability near a clip edge, exactly the clipped
rows each case names, the two 256-tile routes far enough apart that a call on the wrong one fails --, the asserted constants are 4 x
the float32 stand-in's floor (one digit, rounded up), and each of eight planted errors fails the new comparison while the existing
tests' assertions (restated as data in _vocab_ce_cases.old_assertions) let it pass."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _bf16_exact_cases as X
import _vocab_ce_cases as C

F32, F64 = np.float32, np.float64
NO_BOUND = {"g": np.inf, "loss": np.inf, "dbias": np.inf}


@pytest.fixture(scope="module", autouse=True)
def _release_the_cases():
    """The cached cases and references hold hundreds of megabytes: gone when this module is done."""
    yield
    C.clear_caches()


@functools.lru_cache(maxsize=None)
def sweep():
    """One pass over every case: the facts the device test relies on, and the stand-in's ratios.  At the large shapes the [M, V]
    outputs are measured on C.host_blocks (whole rows for the gradient, whole columns for the bias gradient); the row statistics,
    the losses and the clip decisions are always the whole case's."""
    facts, ratios = {}, {}

    def note(into, key, value):
        into[key] = max(into.get(key, 0.0), value)

    def one(case):
        """-> (the case's facts, its ratios): nothing shared is written from the pool's threads."""
        M, V, K, v = case
        mine = {}
        c = C.operands(M, V, K, v)
        big = (M, V, K) in C.BIG
        rows, cols = C.host_blocks(M, V) if big else (None, None)
        f = {"ties": X.tie_shares(c["z"])}
        held = {}
        for parked in ((False, True) if big else (False,)):
            _, z = C._case_logits(M, V, K, v, parked, False)
            rst = C.reference_stats(c, z)
            sst = C.standin_stats(c, parked, "fast", 256 if big else 128)
            ref = C.reference_from_logits(c, z, rows, None, stats=rst)
            got = C.standin(c, rows=rows, stats=sst)
            out = C.compare_outputs(ref, NO_BOUND, loss=got["loss"], g=got["g"], g_bits=got["g_bits"])
            if big:
                refc = C.reference_from_logits(c, z, None, cols, stats=rst)
                out["dbias"] = C.compare_outputs(refc, NO_BOUND, dbias=C.standin(c, cols=cols, stats=sst)["dbias"])["dbias"]
            else:
                out["dbias"] = C.compare_outputs(ref, NO_BOUND, dbias=got["dbias"])["dbias"]
            note(mine, ("fast", v, "g"), max(out["dlogits"].worst, out["dlogits bf16"].worst))
            note(mine, ("fast", v, "loss"), out["loss_rows"].worst)
            note(mine, ("fast", v, "dbias"), out["dbias"].worst)
            name = "parked" if parked else "plain"
            f[name] = {"edges": C.edge_distance(ref), "clipped": tuple(int(r) for r in np.nonzero(ref["needs_clip"])[0]),
                       "standin clipped": tuple(int(r) for r in np.nonzero(got["needs_clip"])[0]), "pmax": ref["pmax"], "pt": ref["pt"]}
            held[parked] = (ref, got)
        if big:                                                  # a call on the other route, held to this route's reference
            const = C.CONST["fast"][v]["g"]
            (plain, _), (park, _) = held[False], held[True]
            f["references apart"] = float(np.mean(np.abs(park["g"] - plain["g"]) > const * C.U * np.maximum(park["A_g"], plain["A_g"]) +
                                                  C.TINY * plain["tiny_g"][:, None]))
            f["other route's share"] = tuple(
                C.compare_bf16(held[not parked][1]["g_bits"], held[parked][0]["g"], held[parked][0]["A_g"], held[parked][0]["tiny_g"],
                               const, "the other route").bad / held[parked][0]["g"].size for parked in (False, True))
        return f, mine

    # (NumPy releases the interpreter lock inside its loops: the cases run side by side; their results are merged here, on one thread)
    with ThreadPoolExecutor(max_workers=4) as pool:
        for case, (f, mine) in zip(C.all_cases(), pool.map(one, C.all_cases())):
            facts[case] = f
            for key, value in mine.items():
                note(ratios, key, value)
    for (M, V, K) in C.SOFTMAX_SHAPES:                           # dc_softmax_ce_f32: float32 exp
        for v in C.variations(M, V, K):
            c = C.softmax_operands(M, V, K, v)
            ref = C.reference_from_logits(c, c["z"])
            got = C.standin(c, exp="libm", tile_rows=M)
            out = C.compare_outputs(ref, NO_BOUND, loss=got["loss"], g=got["g"], probs=got["p"])
            note(ratios, ("libm", v, "g"), max(out["dlogits"].worst, out["probs"].worst))
            note(ratios, ("libm", v, "loss"), out["loss_rows"].worst)
            facts[("softmax", M, V, K, v)] = {"edges": C.edge_distance(ref), "clipped": tuple(int(r) for r in np.nonzero(ref["needs_clip"])[0])}
    return facts, ratios


@pytest.mark.parametrize("M,V,K,variation", C.all_cases())
def test_case_is_what_the_device_test_takes_it_for(M, V, K, variation):
    facts, _ = sweep()
    c, f = C.operands(M, V, K, variation), facts[(M, V, K, variation)]
    C.P.assert_exact_f32(c["z"], "the logits")                  # (operands() asserted it when it built them)
    assert np.array_equal(c["z"][C.BIAS_ROW], c["bias"]) and not c["X"][C.BIAS_ROW].any()
    up, down = f["ties"]
    assert up >= C.TIE_SHARE and down >= C.TIE_SHARE, (up, down)
    if c["keras_sparse"]:
        assert c["w"][C.ZERO_ROW] == 0.0 and (np.delete(c["w"], C.ZERO_ROW) > 0).all()
    for name in ("plain", "parked"):
        if name not in f:
            continue
        lo, hi = f[name]["edges"]
        assert lo >= C.EDGE_MARGIN and hi >= C.EDGE_MARGIN_HI, (name, lo, hi)
        assert f[name]["clipped"] == c["clipped_rows"] == f[name]["standin clipped"], name
        if variation == "sparse mixed":                          # exactly two rows of the first row tile, one high, one twice 1/2
            assert f[name]["clipped"] == (C.LO_ROW, C.HI_ROW) and C.HI_ROW < 128
            assert f[name]["pmax"][C.HI_ROW] > 1 - C.EPS and c["t"][C.HI_ROW] == C.HI_COL
            assert abs(f[name]["pmax"][C.LO_ROW] - 0.5) < 1e-3 and abs(f[name]["pt"][C.LO_ROW] - 0.5) < 1e-3
        if variation == "sparse all":
            assert f[name]["pt"][4] < C.EPS and c["t"][4] == C.CLIP_COL
    if "other route's share" in f:
        assert f["references apart"] >= C.ROUTE_SHARE and min(f["other route's share"]) >= C.ROUTE_SHARE_BF16, (f["references apart"], f["other route's share"])


def test_softmax_cases_keep_the_edges_and_the_clipped_rows():
    facts, _ = sweep()
    for (M, V, K) in C.SOFTMAX_SHAPES:
        for v in C.variations(M, V, K):
            f, c = facts[("softmax", M, V, K, v)], C.softmax_operands(M, V, K, v)
            assert f["edges"][0] >= C.EDGE_MARGIN and f["edges"][1] >= C.EDGE_MARGIN_HI and f["clipped"] == c["clipped_rows"], (M, V, K, v, f)
    assert C.SOFTMAX_SHAPES[-1][1] % 4 != 0


def test_constants_are_four_times_the_stand_ins_floor():
    """Every asserted constant is 4 x the recorded floor (C.FLOOR), rounded up to one digit, and the recorded
    floor is the largest ratio of the float32 stand-in on the cases of its variation as measured here (to FLOOR_TOLERANCE: a
    float32 exp differs by an ulp between NumPy builds, and a floor just below a digit's edge must not flip the constant)."""
    _, ratios = sweep()
    for (exp, v, kind), floor in sorted(ratios.items()):
        print("vocab-ce-elementwise floor %s / %s / %s: %.3g -> asserted %g" % (exp, v, kind, floor, C.CONST[exp][v][kind]))
    for (exp, v, kind), floor in ratios.items():
        recorded = C.FLOOR[exp][v][kind]
        assert C.CONST[exp][v][kind] == C.one_digit_up(4.0 * recorded), (exp, v, kind)
        assert abs(recorded - floor) <= C.FLOOR_TOLERANCE * recorded, (exp, v, kind, recorded, floor)
    assert {(e, v, k) for e in C.CONST for v in C.CONST[e] for k in C.CONST[e][v]} == set(ratios)


# ---------------------------------------------------------------------------------------------------------------------------------
# planted errors.  Each runs the stand-in of one route on one case, plants the error and returns
#   (the new comparison's verdicts, whether the existing tests' assertions pass, the kind of constant it is measured against, the case)

def _quiet_chunk(c, ref, limit):
    """(row, first column) of sixteen aligned columns without the row's target whose probabilities are all below `limit`."""
    p = ref["p"]
    for r in range(5, p.shape[0]):
        for c0 in range(16, p.shape[1] - 16, 16):
            if p[r, c0:c0 + 16].max() < limit and not (c0 <= c["t"][r] < c0 + 16):
                return r, c0
    raise AssertionError("no quiet chunk")


SMALL_CASE = (130, 1016, 2048, "categorical")
PARKED_CASE = (264, 1000, 256, "categorical")                   # the parked route's FORMULAS at a small shape (the stand-in takes any)


def _small_bf16(plant):
    c, ref = C.operands(*SMALL_CASE), C.reference(*SMALL_CASE)
    got = C.standin(c)
    bits = got["g_bits"].copy()
    r, c0 = _quiet_chunk(c, ref, 1.5e-3)
    plant(bits, got, r, c0)
    new = C.compare_outputs(ref, C.CONST["fast"]["categorical"], g_bits=bits)
    return new, C.old_assertions(c, ref, "bf16 128, bf16 dl", g_bits=bits), "g"


def _swap(bits, got, r, c0):
    bits[r, c0:c0 + 8], bits[r, c0 + 8:c0 + 16] = bits[r, c0 + 8:c0 + 16].copy(), bits[r, c0:c0 + 8].copy()


def _stale(bits, got, r, c0):
    bits[r, c0:c0 + 8] = 0                                       # what a zero-initialised buffer holds (the device test's own sentinel is -3e30)


def _truncate(bits, got, r, c0):
    # below the largest entry's binade, where the existing bound (2^-8 of the LARGEST entry) cannot see one bf16 ulp: every non-target
    below = np.abs(got["g"]) < 0.5 * np.abs(got["g"]).max()
    bits[below] = X.bf16_round(got["g"], "truncate")[below]


def _parked(what):
    c, ref = C.operands(*PARKED_CASE), C.reference(*PARKED_CASE, parked=True)
    const = C.CONST["fast"]["categorical"]
    good = C.standin(c, parked=True)
    assert all(v.ok for v in C.compare_outputs(ref, const, loss=good["loss"], g_bits=good["g_bits"], dbias=good["dbias"]).values())
    if what == "ties away":
        got = C.standin(c, parked=True, park_rule="away")
        new = C.compare_outputs(ref, const, loss=got["loss"], g_bits=got["g_bits"], dbias=got["dbias"])
        kind = "g"
    elif what == "loss unrounded":
        got = dict(good, loss=C.standin(c, parked=False)["loss"])
        new = C.compare_outputs(ref, const, loss=got["loss"], g_bits=got["g_bits"], dbias=got["dbias"])
        kind = "loss"
    else:
        assert what == "dbias of rounded"
        got = dict(good, dbias=C.column_sums(C.bf16_value(good["g_bits"]), None, c["M"], 256))
        new = C.compare_outputs(ref, const, loss=got["loss"], g_bits=got["g_bits"], dbias=got["dbias"])
        kind = "dbias"
    old = C.old_assertions(c, ref, "bf16 256 parked", loss=got["loss"], g_bits=got["g_bits"], dbias=got["dbias"], ref_z=c["z"])
    return new, old, kind


def _doubled():
    M, V, K, v = 1500, 8200, 512, "categorical"
    c = C.operands(M, V, K, v)
    rows, _ = C.host_blocks(M, V)
    ref = C.reference_from_logits(c, c["z"], rows, None)
    got = C.standin(c, tile_rows=256, rows=rows)
    g = got["g"].copy()
    r = 40                                                       # a word below 2e-5: the existing fp32 bound is 3e-5 of the largest entry
    k = int(np.argmin(np.where(np.arange(V) == c["t"][rows][r], np.inf, ref["p"][r])))
    assert 0 < ref["p"][r, k] < 2e-5
    g[r, k] *= F32(2.0)
    new = C.compare_outputs(ref, C.CONST["fast"][v], g=g, g_bits=X.bf16_round(g))
    old = C.old_assertions(c, ref, "bf16 256", g=g) and C.old_assertions(c, ref, "bf16 256, bf16 dl", g_bits=X.bf16_round(g))
    return new, old, "g"


def _neighbours():
    case = (130, 1016, 2048, "sparse mixed")
    c, ref = C.operands(*case), C.reference(*case)
    got = C.standin(c, neighbours_of=C.LO_ROW)
    new = C.compare_outputs(ref, C.CONST["fast"]["sparse mixed"], loss=got["loss"], g=got["g"], dbias=got["dbias"])
    # (1 / S - (UP / S - 1) = 1 + (1 - UP) / S: with UP = 1 the row of two halves leaves the gradient as it was -- the loss shows it)
    return new, C.old_assertions(c, ref, "f32 128", loss=got["loss"], g=got["g"], dbias=got["dbias"]), "loss"


PLANTED = {
    "two 16-byte chunks of a row exchanged": lambda: _small_bf16(_swap),
    "one 8-column store left stale": lambda: _small_bf16(_stale),
    "bf16 gradient truncated": lambda: _small_bf16(_truncate),
    "parked logits rounded with ties away": lambda: _parked("ties away"),
    "one gradient doubled at V = 8200": _doubled,
    "loss from unrounded logits beside a gradient from rounded ones": lambda: _parked("loss unrounded"),
    "a clipped row's S and UP applied to its tile neighbours": _neighbours,
    "dbias summed from the bf16-rounded gradient": lambda: _parked("dbias of rounded"),
}


@functools.lru_cache(maxsize=None)
def planted(name):
    return PLANTED[name]()


@pytest.mark.parametrize("name", list(PLANTED))
def test_planted_error_fails_the_new_comparison_and_passes_the_old(name):
    new, old, kind = planted(name)
    failing = {k: v for k, v in new.items() if not v.ok}
    for v in failing.values():
        print(v.report())
    assert failing, "the new comparison let it pass"
    assert old, "the existing assertions see it too: not a gap they leave"
    if name == "bf16 gradient truncated":                        # about half of the entries: every one whose fp32 value was rounded up
        v = new["dlogits bf16"]
        assert 0.3 < v.bad / v.size < 0.7, v.bad / v.size


def test_the_stale_store_fails_with_the_device_tests_sentinel_too():
    c, ref = C.operands(*SMALL_CASE), C.reference(*SMALL_CASE)
    bits = C.standin(c)["g_bits"].copy()
    bits[9, 64:72] = X.bf16_round(F32(C.P.SENTINEL["bfloat16"]))
    v = C.compare_outputs(ref, C.CONST["fast"]["categorical"], g_bits=bits)["dlogits bf16"]
    assert v.bad == 8


def test_every_constant_is_below_half_of_the_smallest_planted_figure_of_its_kind():
    figures = {}
    for name in PLANTED:
        new, _, kind = planted(name)
        worst = max(v.worst for v in new.values() if not v.ok)
        figures[kind] = min(figures.get(kind, np.inf), worst)
        print("vocab-ce-elementwise planted %s: worst ratio %.3g (%s)" % (name, worst, kind))
    assert set(figures) == {"g", "loss", "dbias"}
    for exp in C.CONST:
        for v in C.CONST[exp]:
            for kind, const in C.CONST[exp][v].items():
                assert const < 0.5 * figures[kind], (exp, v, kind, const, figures[kind])


def test_comparison_counts_and_locates():
    """The report names how many entries fail, the first ones with row, column and both values, and the worst ratio; a NaN and a
    value in a dead row (zero weight: the unit is zero) fail."""
    case = (264, 1000, 256, "sparse none")
    c, ref = C.operands(*case), C.reference(*case)
    got = C.standin(c)
    const = C.CONST["fast"]["sparse none"]
    assert all(v.ok for v in C.compare_outputs(ref, const, loss=got["loss"], g=got["g"], g_bits=got["g_bits"], dbias=got["dbias"]).values())
    g = got["g"].copy()
    g[7, 5] = np.nan
    g[C.ZERO_ROW, 9] = 1e-30
    g[40, 100] *= F32(1.001)
    v = C.compare_outputs(ref, const, g=g)["dlogits"]
    assert v.bad == 3 and not v.ok and v.worst == np.inf
    text = v.report()
    assert "3 of 264000" in text and "(7, 5)" in text and "(2, 9)" in text and "(40, 100)" in text, text
    assert C.one_digit_up(41.2) == 50.0 and C.one_digit_up(4.0) == 4.0 and C.one_digit_up(0.71) == 0.8 and C.one_digit_up(166.4) == 200.0
