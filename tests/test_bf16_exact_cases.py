"""The instrument of tests/_bf16_exact_cases.py, proven on the host (no GPU, no library): every operand is exact in bf16 and every
expected value in fp32, every bf16 output has exact ties on both sides of round-to-even, the tables reach every mechanism of every
kernel, and the equality comparison sees one lost product, one doubled K-tile, truncation, ties-away and half-up.

What the bound of tests/test_gpu_bf16.py on a bf16 output, max|got - want| <= 2^-8 max|want| + 1e-6, makes of the rounding rules is
recorded here too.  The bound lies between half an ulp and one ulp of the largest element's binade.  Ties away from zero and half-up err
by half an ulp of the element at a tie: they pass it on every output (asserted).  Truncation errs by up to an ulp of the element: it
passes on every element below the top binade (asserted), and in the top binade -- under 6 % of each of these outputs, 0.2 % in the
median -- only where the dropped bits happen to be small or max|want| sits high in its binade.  On these grids it does NOT pass there: the emulated truncation exceeds the
older bound on 31 of the 32 outputs of the tables (largest error / bound: 0.0308 / 0.0219 on the 200 x 1024 x 3136 product, 0.0215 /
0.0213 on the "3x3 ragged" convolution; it passes 4096 x 3072 x 72, whose largest element 1.02 has a near-empty binade to itself).  So
what the older assertion cannot see is a truncating kernel's error on the 94 % or more of an output below the largest binade, and a
ties-away or half-up kernel at all."""
import numpy as np
import pytest

import _bf16_exact_cases as X
import _placement_cases as P

from oracle import np_oracle as O

GEMM_SHAPES = sorted({row[:3] for row in X.GEMM_PLAIN})
GEMM_EPILOGUES = [row[:4] for row in X.GEMM_EPILOGUE]


def _on_bf16_grid(a):
    return np.array_equal(O.to_bf16(a), np.asarray(a, np.float64))


def _has_ties(want, what):
    up, down = X.tie_shares(want)
    assert up >= X.TIE_SHARE and down >= X.TIE_SHARE, "%s: %.2f %% of the elements are ties that round up, %.2f %% ties that round down" % (
        what, 100 * up, 100 * down)
    # ... and bf16_of sends them where round-to-nearest-even says: up to the even neighbour above, down to the even one below
    u = X.f32_bits(want)
    tie = (u & 0xFFFF) == 0x8000
    kept = X.bf16_bits(P.bf16_of(want))[tie].astype(np.int64)
    assert np.all(kept & 1 == 0) and np.array_equal(kept, ((u[tie] >> 16).astype(np.int64) + 1) // 2 * 2)


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_case_is_exact_and_has_ties(M, N, K):
    c = X.gemm_plain(M, N, K)
    assert K < X.K_LIMIT and _on_bf16_grid(c["A"]) and _on_bf16_grid(c["B"])
    assert np.array_equal(c["want"], c["A"] @ c["B"])
    P.assert_exact_f32(c["want"], "want")
    _has_ties(c["want"], "A B")


@pytest.mark.parametrize("M,N,K,residual", GEMM_EPILOGUES)
def test_gemm_epilogue_case_is_exact_and_has_ties(M, N, K, residual):
    c = X.gemm_epilogue(M, N, K, residual)
    assert K < X.K_LIMIT and _on_bf16_grid(c["A"]) and _on_bf16_grid(c["B"])
    for name in ("scale", "shift", "residual", "C0", "want", "want_acc"):
        P.assert_exact_f32(c[name], name)
    assert c["relu"] and c["residual"].shape == ((M, N) if residual == "full" else (residual, N))
    assert np.array_equal(c["want_acc"], c["want"] + c["C0"]) and c["want"].min() == 0.0 and (c["want"] == 0).mean() > 0.1      # relu bites
    _has_ties(c["want"], "the bf16-only leg")
    _has_ties(c["want_acc"], "the accumulating legs")


def test_gather_and_strided_cases_are_exact_and_have_ties():
    g, d = X.gather_case(), X.GATHER
    assert _on_bf16_grid(g["table"]) and _on_bf16_grid(g["W"]) and _on_bf16_grid(g["dz"])
    assert not g["table"][:, d["E"]:].any() and not g["W"][d["E"]:].any() and g["table"][:, :d["E"]].any()
    assert len(np.unique(g["ids"])) < d["N"] and len(np.unique(g["ids"])) > d["N"] // 2          # repeated rows, and most of the table
    assert [(leg[1], leg[2], leg[3]) for leg in X.GATHER_LEGS] == [(d["N"], d["U"], d["Ep"]), (d["Ep"], d["U"], d["N"])]
    _has_ties(g["want_rows"], "row gather")
    _has_ties(g["want_k"], "K gather")
    s = X.strided_case()
    assert _on_bf16_grid(s["X"]) and _on_bf16_grid(s["W"])
    _has_ties(s["want"], "strided B")


@pytest.mark.parametrize("name", list(X.CONV_ROWS))
def test_conv_case_is_exact_and_has_ties(name):
    c = X.conv_case(name)
    M, N, K, Ho, Wo = X.conv_geometry(name)
    assert K < X.K_LIMIT and K % 64 == 0 and c["want"].shape[1:] == (Ho, Wo, N) and c["want"].size == M * N
    assert _on_bf16_grid(c["x"]) and _on_bf16_grid(c["w"]) and c["w"].shape == (N, K)
    for name_ in ("scale", "shift", "want"):
        P.assert_exact_f32(c[name_], name_)
    assert (c["residual"] is None) == (c["res_mode"] == 0)
    _has_ties(c["want"], "conv " + name)


def test_conv_rows_cover_the_residual_modes_on_every_tile():
    for tile in (64, 128, 256):
        modes = {X.CONV_ROWS[n][0][7] for n in X.CONV_ROWS if X.conv_granted(n, tile) == tile}
        assert modes == {0, 1, 2}, (tile, modes)
    assert set(X.CONV_OWN_TILE.values()) == {64, 256}


@pytest.mark.parametrize("name", list(X.WGRAD_ROWS))
def test_wgrad_case_is_exact(name):
    c = X.wgrad_case(name)
    (N, H, W, Cin, Cout, k, stride), _, _ = X.WGRAD_ROWS[name]
    assert N * H * W < X.K_LIMIT and Cin % 128 == 0 and Cout % 8 == 0
    assert _on_bf16_grid(c["x"]) and _on_bf16_grid(c["dy"]) and c["want"].shape == (Cout, k * k * Cin)
    P.assert_exact_f32(c["want"], "dw")
    P.assert_exact_f32(c["want_twice"], "2 dw")
    assert np.array_equal(c["want_twice"], 2 * c["want"]) and np.count_nonzero(c["want"]) > 0.5 * c["want"].size
    # the centre tap of the packed gradient is the plain product over the pixels
    centre = (k * k // 2) * Cin
    assert np.array_equal(c["want"][:, centre:centre + Cin], c["dy"].reshape(-1, Cout).T @ c["x"].reshape(-1, Cin))


def test_cases_are_cached_and_read_only():
    c = X.gemm_plain(264, 136, 72)
    assert X.gemm_plain(264, 136, 72) is c and X.conv_case("pw 64-64") is X.conv_case("pw 64-64")
    with pytest.raises(ValueError):
        c["want"][0, 0] = 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# mechanism coverage: a case that loses its edge fails here, not passes on the GPU while testing nothing

def test_every_kernel_is_reached_on_every_mechanism_it_has():
    reached = {k: set() for k in X.KERNELS}
    for what, kernel, mechanisms in X.legs():
        reached[kernel] |= mechanisms
    for kernel, needed in X.KERNELS.items():
        assert needed <= reached[kernel], "%s: no case reaches %s" % (kernel, sorted(needed - reached[kernel]))


def test_the_tables_hold_the_shapes_they_are_meant_to():
    assert {row[:4] for row in X.GEMM_PLAIN if row[:3] == (200, 1024, 3136)} == {(200, 1024, 3136, s) for s in (0, 1, 3, 7)}
    assert {row[4] for row in X.GEMM_PLAIN} == {128, 256} and {row[5] for row in X.GEMM_EPILOGUE} == {128, 256}
    for tile in (128, 256):                      # per tile: the epilogue with and without slabs, both residual forms between them
        rows = [r for r in X.GEMM_EPILOGUE if r[5] == tile]
        assert {r[6] > 1 for r in rows} == {True, False} and {r[3] == "full" for r in rows} == {True, False}
    assert len(X.CONV_ROWS) == 15 and len(X.WGRAD_ROWS) == 10
    assert {row[1] for row in X.WGRAD_ROWS.values()} == {128, 256}
    # the 256-square tile is refused for a sliver only
    assert [n for n in X.CONV_ROWS if X.conv_granted(n, 256) != 256] == ["3x3 ragged", "pw Cout 20"]


# ---------------------------------------------------------------------------------------------------------------------------------
# planted errors: each fails the equality comparison; the two rounding rules pass what test_gpu_bf16.py asserts of a bf16 output

def _old_bf16_assertion(got_bits, want):
    """The two sides of tests/test_gpu_bf16.py's assertion on a bf16 output, max|got - want| <= 2^-8 * max|want| + 1e-6:
    (|got - want| per element, the bound)."""
    got = (got_bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return np.abs(got - want), 2.0 ** -8 * np.abs(want).max() + 1e-6


def _planted(A, B, want, **epilogue):
    want_bf16 = P.bf16_of(want)
    shape = want.shape

    def run(**plant):
        f, b = X.emulate(A, B, **epilogue, **plant)
        return f.reshape(shape), b.reshape(shape)

    f, b = run()                                                       # the intended arithmetic equals the exact result
    assert X.mismatch(f, want, "fp32") is None and X.mismatch(b, want_bf16, "bf16") is None

    f, b = run(drop=X.smallest_product(A, B, want))                    # one product of 2^-11 lost at one output
    report = X.mismatch(f, want, "dropped product")
    assert report is not None and "1 of %d elements differ" % want.size in report, report
    d = np.abs(f.view(np.float32).astype(np.float64) - want).max()
    assert d in (2.0 ** -12, 2.0 ** -11, 2.0 ** -10), d                # the product times the column's scale (1/2, 1 or 2)

    f, b = run(twice=64)                                               # one K-tile of 64 twice in one 128 x 128 block
    report = X.mismatch(f, want, "doubled K-tile")
    assert report is not None
    bad = (f != X.f32_bits(want)).reshape(A.shape[0], -1)
    assert bad[:128, :128].mean() > 0.25 and not bad[128:].any() and not bad[:, 128:].any()
    report = X.mismatch(b, want_bf16, "doubled K-tile")
    assert report is not None and "not a rounding rule" in report, report

    up, down = X.tie_shares(want)
    top = np.abs(want) >= 2.0 ** np.floor(np.log2(np.abs(want).max()))  # the elements in the binade of the largest one
    assert 0 < top.mean() < 0.5
    for rule in ("truncate", "away", "half up"):
        f, b = run(rounding=rule)
        assert X.mismatch(f, want, rule) is None                       # the fp32 output is untouched
        report = X.mismatch(b, want_bf16, rule)
        assert report is not None and "ONE bf16 ulp" in report, report
        wrong = int((b != X.bf16_bits(want_bf16)).sum())
        assert wrong >= (up if rule == "truncate" else down if rule == "away" else (up + down) / 4) * want.size      # the ties it gets wrong, at the least
        err, bound = _old_bf16_assertion(b, want)
        if rule == "truncate":
            # Off by up to a whole ulp of the element.  The older bound lies between half an ulp and one ulp of the LARGEST element's
            # binade, so below that binade (where an ulp is at most half as large) truncation always passes it: the older assertion
            # sees truncation through the top binade alone, a few per cent of the output at the most -- and there only where max|want|
            # sits low in its binade (it does in most of these cases: 0.0308 against 0.0219 on the 200 x 1024 x 3136 product, max|want| = 5.6).
            assert np.all(err[~top] <= bound), rule
        else:
            assert err.max() <= bound, "%s fails the older bound too" % rule      # half an ulp at a tie: passes whatever the output


def test_planted_errors_in_a_gemm():
    M, N, K, residual = X.GEMM_EPILOGUE[0][:4]
    c = X.gemm_epilogue(M, N, K, residual)
    _planted(c["A"], c["B"], c["want"], scale=c["scale"], shift=c["shift"], residual=c["residual"], relu=True)


def test_planted_errors_in_a_plain_gemm():
    c = X.gemm_plain(264, 136, 72)
    _planted(c["A"], c["B"], c["want"])


def test_planted_errors_in_a_convolution():
    c = X.conv_case("3x3 ragged")
    A, B, res = X.conv_as_gemm(c)
    _planted(A, B, c["want"], scale=c["scale"], shift=c["shift"], residual=res, relu=c["relu"])


def test_the_report_counts_unwritten_elements():
    c = X.gemm_plain(264, 136, 72)
    got = X.f32_bits(c["want"]).copy()
    got[3, 4:8] = X.f32_bits(np.float32(P.SENTINEL["float32"]))[0]
    got[9, 1] = X.f32_bits(np.float32(np.nan))[0]
    report = X.mismatch(got, c["want"], "holes", sentinel=P.SENTINEL["float32"])
    assert "5 of %d elements differ" % got.size in report and "5 never written" in report, report
    assert X.mismatch(X.f32_bits(c["want"]), c["want"], "whole") is None
