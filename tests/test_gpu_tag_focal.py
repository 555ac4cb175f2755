"""dc_tag_focal_f32 and dc_tag_scores_f32 (-m gpu) against the float64 restatement of tests/_roitag_ref.py.

Tolerances are the project's kernel-test ones: loss_rows within 1e-5 * max(1, |want|), dz within 1e-5 * max|want|.  (A float32 NumPy
model of the kernel's formulation is within 2e-7 / 4e-7 of the float64 restatement on these cases; the kernels measured 8.3e-8 / 3.5e-7
on an MI355X, 8.7e-8 on probs and 0 on the scores.)  Every logit is at least 0.05 away
from the clip thresholds -16.1181 / 15.9424, where the gradient jumps (tests/test_roitag_ref.py)."""
import numpy as np
import pytest
import torch

from image_captioning_amd._lib import DcapError

import _roitag_ref as R

pytestmark = pytest.mark.gpu

# strided: ld = C + 3.  Between the two layouts both paths run with ld == C and with ld > C: the 16-byte path at contiguous C = 64, 4100
# and strided C = 5, 257 (ld 8, 260: with a scalar tail), the 4-byte path at every odd or 2-mod-4 stride (contiguous 5, 257, 1023;
# strided 64 -> 67, 1023 -> 1026, 4100 -> 4103).
LAYOUTS = ("contiguous", "strided")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def dev(a, dtype):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().copy()


def place(a, dtype, layout):
    """[M,C] on the device: contiguous, or the leading columns of a [M, C + 3] buffer."""
    if layout == "contiguous":
        return dev(a, dtype)
    return dev(R.strided(a, a.shape[1] + 3), dtype)[:, :a.shape[1]]


def out_like(M, C, layout):
    whole = torch.full((M, C if layout == "contiguous" else C + 3), 123.0, dtype=torch.float32, device="cuda")
    return whole, whole[:, :C]


_CASES = {}


def case(M, C):
    """(z, t) of the shape, computed once."""
    if (M, C) not in _CASES:
        _CASES[(M, C)] = R.focal_case(M, C)
    return _CASES[(M, C)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,C", R.SHAPES)
def test_tag_focal_matches_the_float64_restatement(ops, M, C, layout):
    z, t = case(M, C)
    zd, td = place(z, torch.float32, layout), place(t, torch.int32, layout)
    dead = ~R.live_rows(t)
    for gamma in (0, 1, 2):
        for alpha in (0.25, 0.5):
            want_rows, want_dz = R.tag_focal(z, t, alpha, gamma, grad_scale=0.5)
            whole, dz = out_like(M, C, layout)
            rows = torch.full((M,), 123.0, dtype=torch.float32, device="cuda")
            ops.tag_focal(zd, td, alpha=alpha, gamma=gamma, grad_scale=0.5, loss_rows=rows, dlogits=dz)
            got_rows, got_dz = rows.cpu().numpy().astype(np.float64), dz.cpu().numpy().astype(np.float64)
            assert np.isfinite(got_rows).all() and np.isfinite(got_dz).all()                     # +-200 included
            err_rows = (np.abs(got_rows - want_rows) / np.maximum(1.0, np.abs(want_rows))).max()
            err_dz = np.abs(got_dz - want_dz).max() / max(np.abs(want_dz).max(), 1e-30)
            print("tag_focal M=%d C=%d %s gamma=%d alpha=%.2f: loss_rows %.3e  dz %.3e" % (M, C, layout, gamma, alpha, err_rows, err_dz))
            assert err_rows < 1e-5, (gamma, alpha, err_rows)
            assert err_dz < 1e-5, (gamma, alpha, err_dz)
            assert (bits(rows)[dead] == 0).all() and (bits(dz)[dead] == 0).all()                 # bit-zero, not merely small
            if layout == "strided":
                assert (whole[:, C:] == 123.0).all()                                             # nothing written past C


@pytest.mark.parametrize("layout", LAYOUTS)
def test_dead_rows_are_bit_zero_with_nan_and_inf_in_their_logits(ops, layout):
    M, C = 12, 257
    z, t = case(M, C)
    z = z.copy()
    dead = np.flatnonzero(~R.live_rows(t))
    z[dead[0], :] = np.nan
    z[dead[1], ::3] = np.inf
    z[dead[2], 1::2] = -np.inf
    _, dz = out_like(M, C, layout)
    rows = torch.full((M,), 123.0, dtype=torch.float32, device="cuda")
    ops.tag_focal(place(z, torch.float32, layout), place(t, torch.int32, layout), loss_rows=rows, dlogits=dz)
    assert (bits(rows)[dead] == 0).all() and (bits(dz)[dead] == 0).all()
    live = R.live_rows(t)
    want_rows, want_dz = R.tag_focal(np.where(live[:, None], z, 0.0), t)
    assert np.abs(dz.cpu().numpy() - want_dz).max() < 1e-5 * np.abs(want_dz).max()
    assert np.isfinite(rows.cpu().numpy()).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,C", [(7, 64), (12, 257), (2, 4100)])
def test_tag_focal_is_deterministic_and_a_row_does_not_depend_on_the_batch(ops, M, C, layout):
    z, t = case(M, C)
    zd, td = place(z, torch.float32, layout), place(t, torch.int32, layout)
    outs = []
    for _ in range(2):
        _, dz = out_like(M, C, layout)
        rows = torch.empty((M,), dtype=torch.float32, device="cuda")
        ops.tag_focal(zd, td, loss_rows=rows, dlogits=dz)
        outs.append((bits(rows), bits(dz)))
    assert (outs[0][0] == outs[1][0]).all() and (outs[0][1] == outs[1][1]).all()
    for m in range(M):                                     # the one-row call: another M, and for odd m another base alignment
        dz1 = torch.empty((1, C), dtype=torch.float32, device="cuda")
        rows1 = torch.empty((1,), dtype=torch.float32, device="cuda")
        ops.tag_focal(zd[m:m + 1], td[m:m + 1], loss_rows=rows1, dlogits=dz1)
        assert bits(rows1)[0] == outs[0][0][m] and (bits(dz1)[0] == outs[0][1][m]).all(), m


def test_each_output_is_optional_and_leaves_the_other_unchanged(ops):
    M, C = 7, 64
    z, t = case(M, C)
    zd, td = dev(z, torch.float32), dev(t, torch.int32)
    rows, dz = ops.tag_focal(zd, td, loss_rows=torch.empty((M,), device="cuda"), dlogits=torch.empty((M, C), device="cuda"))
    rows_only, none = ops.tag_focal(zd, td, loss_rows=torch.empty((M,), device="cuda"))
    assert none is None and (bits(rows_only) == bits(rows)).all()
    none, dz_only = ops.tag_focal(zd, td, dlogits=torch.empty((M, C), device="cuda"))
    assert none is None and (bits(dz_only) == bits(dz)).all()
    default_rows, none = ops.tag_focal(zd, td)              # neither given: loss_rows is allocated
    assert none is None and (bits(default_rows) == bits(rows)).all()
    inplace = zd.clone()                                    # dz may alias z
    ops.tag_focal(inplace, td, dlogits=inplace)
    assert (bits(inplace) == bits(dz)).all()


def test_bad_gamma_and_alpha_are_refused_without_a_launch(ops):
    z, t = dev(np.zeros((2, 8)), torch.float32), dev(np.ones((2, 8)), torch.int32)
    dz = torch.full((2, 8), 5.0, device="cuda")
    for kw in (dict(gamma=1.5), dict(alpha=1.5), dict(alpha=-0.1), dict(gamma=3)):
        with pytest.raises(DcapError, match=r"code -1"):
            ops.tag_focal(z, t, dlogits=dz, **kw)
    torch.cuda.synchronize()
    assert (dz == 5.0).all()
    with pytest.raises(DcapError):
        ops.tag_focal(z, t.to(torch.float32))
    with pytest.raises(DcapError):
        ops.tag_focal(z, t[:, :4])


# ---- dc_tag_scores_f32 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,C", R.SHAPES)
def test_tag_scores(ops, M, C, layout):
    z, _ = case(M, C)
    z = z.copy()
    if M > 1:
        z[1] = -np.abs(z[1]) - 1.0                          # a row with nothing above 0.5 / 0.7
    zd = place(z, torch.float32, layout)
    want_p = R.sigmoid(z)[0]
    for thr in (0.0, 0.5, 0.7):
        whole, probs = out_like(M, C, layout)
        scores = torch.empty((M,), dtype=torch.float32, device="cuda")
        ops.tag_scores(zd, thr, probs=probs, scores=scores)
        p, s = probs.cpu().numpy(), scores.cpu().numpy()
        assert np.abs(p.astype(np.float64) - want_p).max() < 2e-7
        want_s = R.tag_scores(p, thr)                       # from the device's own probabilities
        none = want_s == R.NO_SCORE
        assert (s[none] == R.NO_SCORE).all() and (s.view(np.int32)[none] == want_s.view(np.int32)[none]).all()
        err = (np.abs(s.astype(np.float64) - want_s.astype(np.float64)) / np.maximum(1.0, np.abs(want_s.astype(np.float64))))[~none]
        print("tag_scores M=%d C=%d %s thr=%.1f: probs %.3e  scores %.3e" % (M, C, layout, thr, np.abs(p - want_p).max(), err.max() if err.size else 0.0))
        assert err.size == 0 or err.max() < 1e-6
        if M > 1 and thr >= 0.5:
            assert none[1]
        if layout == "strided":
            assert (whole[:, C:] == 123.0).all()
    p2, s2 = ops.tag_scores(zd, 0.5)                        # outputs allocated by the wrapper
    probs, scores = ops.tag_scores(zd, 0.5, probs=torch.empty((M, C), device="cuda"), scores=torch.empty((M,), device="cuda"))
    assert (bits(p2) == bits(probs)).all() and (bits(s2) == bits(scores)).all()
