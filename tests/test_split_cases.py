"""The piece-product projection of tests/_split_cases.py, proven on the emulated arithmetic of every case (no GPU): present products
project to 0, a dropped one to -1, a doubled one to +1, in every stratum -- and a kernel that lost a third-order product would have passed
the 2e-5 max-norm tolerance every split-bf16 test used before."""
import numpy as np
import pytest

import _split_cases as S

PROBLEMS = dict(S.all_problems())


def _scaled_err(got, prob):
    idx = Ellipsis if prob.whole is None else prob.whole
    return float(np.abs(got.astype(np.float64) - prob.want)[idx].max()) / max(1.0, float(np.abs(prob.want[idx]).max()))


def test_the_table_holds_every_family():
    assert len(PROBLEMS) == len(S.CONV) + 2 + len(S.WINO) + 1 + len(S.WINO_LEVELS[1]) + 2 * len(S.CHAIN)
    second = set(S.wino_second_items(S.WINO[S.WINO_MULTI][:3] + S.WINO[S.WINO_MULTI][4:]))
    sampled = {name for name, _ in S.wino_case(S.WINO_MULTI)[1].strata}
    assert second and any("item slice %d group %d" % sg in sampled for sg in second)       # strata on items a block takes second


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_strata_hold_a_thousand_outputs(name):
    prob = PROBLEMS[name]
    assert prob.strata
    for sname, idx in prob.strata:
        assert prob.want[idx].size >= S.MIN_STRATUM, (sname, prob.want[idx].size)


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_projection_separates_right_from_wrong(name):
    prob = PROBLEMS[name]

    def coef(**kw):
        got = prob.emulate(**kw)
        return got, S.coefficients(got, prob.want, prob.D, prob.strata, prob.whole)

    got, c = coef()
    w = S.worst(c, S.KEPT)
    assert w[0] <= 0.03, "intended arithmetic: |c| = %.4f in %s for product %s" % w
    for ij in S.KEPT:
        got, c = coef(drop=ij)
        hi = max((v[ij], s) for s, v in c.items())
        assert hi[0] <= -0.9, "dropped %s: c = %.4f in %s" % (ij, hi[0], hi[1])
        if ij in S.THIRD:
            assert _scaled_err(got, prob) < 2e-5           # ... and the tolerance of the older tests does not see it
        got, c = coef(twice=ij)
        lo = min((v[ij], s) for s, v in c.items())
        assert lo[0] >= 0.9, "doubled %s: c = %.4f in %s" % (ij, lo[0], lo[1])
    got, c = coef(pieces=2)
    assert all(v[ij] <= -0.9 for v in c.values() for ij in S.THIRD), "two pieces: %s" % (c["all"],)
    assert S.worst(c, S.SECOND)[0] <= 0.03
    assert _scaled_err(got, prob) < 2e-5
    got, c = coef(pieces=1)
    assert all(v[ij] <= -0.9 for v in c.values() for ij in S.SECOND), "one piece: %s" % (c["all"],)


def test_split3_pieces_are_bf16_and_sum_to_x():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(4097) * np.exp(rng.uniform(-20, 20, 4097))).astype(np.float32)
    x[:4] = [0.0, 1.0, -2.5, 2.0 ** -120]
    p = S.split3(x)
    assert np.all((p.astype(np.float32).view(np.uint32) & 0xffff) == 0)
    assert np.all(np.abs(p.sum(0) - x.astype(np.float64)) <= np.abs(x.astype(np.float64)) * 2.0 ** -24 + 1e-44)
    assert np.array_equal(S.bf16_bits(p[0]), S.bf16_bits(S.O.to_bf16(x)))


def test_winograd_form_is_the_convolution():
    """sum of all nine D_ij-like products = the float64 convolution: the host's Winograd transforms, checked against im2col."""
    prob = S.wino_case("odd sizes")[1]
    v, u = prob.pieces
    full = prob._output(np.matmul(v.sum(0), u.sum(0))) * prob.scale + prob.shift
    assert np.abs(full - prob.want).max() < 1e-5 * np.abs(prob.want).max()                  # (V and U are rounded to fp32)
    ref = S.O.conv2d_winograd_nhwc(prob.x, prob.w, np.float64) * prob.scale + prob.shift
    assert np.abs(ref - prob.want).max() < 1e-12 * np.abs(prob.want).max()
