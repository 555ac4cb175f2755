"""The float64 restatement of the RoI tag head's focal loss (tests/_roitag_ref.py) against closed forms and central differences (no
GPU).  tests/test_gpu_tag_focal.py holds dc_tag_focal_f32 / dc_tag_scores_f32 to that restatement."""
import numpy as np
import pytest

import _roitag_ref as R


def test_clip_thresholds_on_the_logit():
    assert R.LO == float(np.float32(1e-7)) and R.HI == 1.0 - 2.0 ** -23          # float32(1 - 1e-7) is the second float below 1
    assert abs(R.Z_LO - (-16.1181)) < 5e-5 and abs(R.Z_HI - 15.9424) < 5e-5


@pytest.mark.parametrize("gamma", [0, 1, 2])
@pytest.mark.parametrize("alpha", [0.25, 0.5])
def test_analytic_gradient_equals_central_differences(alpha, gamma):
    """|z| < 15 (inside the clip, where the loss is smooth), h = 1e-6, 1e-4 absolute: 20 000 normal * 4 logits."""
    rng = np.random.RandomState(gamma * 10 + int(alpha * 100))
    z = np.clip(rng.randn(20000) * 4.0, -14.9, 14.9)
    t = (rng.rand(20000) < 0.3).astype(np.int32)
    _, g = R.focal_elements(z, t, alpha, gamma)
    h = 1e-6
    num = (R.focal_elements(z + h, t, alpha, gamma)[0] - R.focal_elements(z - h, t, alpha, gamma)[0]) / (2 * h)
    assert np.abs(g - num).max() < 1e-4, np.abs(g - num).max()


def test_gamma_zero_alpha_half_is_half_the_plain_cross_entropy():
    rng = np.random.RandomState(3)
    z = np.concatenate([rng.randn(5000) * 6.0, [-200.0, -30.0, -17.0, 17.0, 30.0, 200.0]])
    t = (rng.rand(z.size) < 0.5).astype(np.int32)
    L, _ = R.focal_elements(z, t, 0.5, 0)
    want = 0.5 * R.plain_bce(z, t)
    assert np.abs(L - want).max() < 1e-9 * max(1.0, np.abs(want).max())


def test_gradient_jumps_at_the_clip_thresholds():
    """Outside the clip only the focal weight's term is left: t = 1 at z = -16.0 (inside) -0.25, at z = -16.3 (outside) -6.7e-7."""
    g = R.focal_elements(np.array([-16.0, -16.3, 15.9, 16.0]), np.array([1, 1, 0, 0]), 0.25, 2)[1]
    assert abs(g[0] - (-0.25)) < 1e-5 and abs(g[1] - (-6.7e-7)) < 1e-8
    assert abs(g[2] - 0.75) < 1e-5 and 0 < g[3] < 3e-6


def test_everything_is_finite_at_200():
    L, g = R.focal_elements(np.array([200.0, -200.0, 200.0, -200.0]), np.array([1, 1, 0, 0]))
    assert np.isfinite(L).all() and np.isfinite(g).all()
    assert L[0] < 1e-20 and abs(L[1] - 0.25 * -R.Z_LO) < 1e-3 and abs(L[2] - 0.75 * R.Z_HI) < 1e-3 and L[3] < 1e-20


def test_dead_rows_are_zero_whatever_their_logits_hold():
    z = np.array([[1.0, -2.0], [np.nan, np.inf], [0.5, 0.5]])
    t = np.array([[0, 1], [0, 0], [0, 0]])
    rows, dz = R.tag_focal(z, t)
    assert rows[0] > 0 and (rows[1:] == 0).all() and (dz[1:] == 0).all() and np.isfinite(dz).all()


@pytest.mark.parametrize("M,C", R.SHAPES)
def test_direct_cases_keep_their_promises(M, C):
    z, t = R.focal_case(M, C)
    assert z.dtype == np.float32 and t.dtype == np.int32 and z.shape == t.shape == (M, C)
    assert min(np.abs(z - R.Z_LO).min(), np.abs(z - R.Z_HI).min()) >= 0.05
    live = R.live_rows(t)
    assert live[0] and t[0].sum() == 1 and t[0, C - 1] == 1                 # the only 1 in the last column
    if M > 2:
        assert not live[1::2].any() and live[0::2].all()                    # dead rows between live ones
        assert t[np.flatnonzero(live)[-1]].all()                            # one all-ones row
    if M * C >= 20:
        assert set(R.PLANTED) <= set(z.reshape(-1).tolist())


def test_scores_restatement():
    p = np.array([[0.9, 0.8, 0.1], [0.2, 0.3, 0.1], [0.7, 0.71, 0.0]], np.float32)
    s = R.tag_scores(p, 0.7)
    assert s.dtype == np.float32 and s[1] == np.float32(-3.4e38)
    assert abs(s[0] - (np.log(np.float64(p[0, 0])) + np.log(np.float64(p[0, 1])))) < 1e-7
    assert abs(s[2] - np.log(np.float64(p[2, 1]))) < 1e-7                   # float32(0.7) > 0.7 is decided in float32: not above
    assert (R.tag_scores(p, 0.0)[:2] < 0).all()
