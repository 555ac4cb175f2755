"""Every instantiation of the fused LSTM step kernels of csrc/lstm.hip against the float64 NumPy oracle (-m gpu).

lstm_step_fused_kernel<RT,NW> (forward), lstm_step_masked_kernel<RT> (forward with recurrent-dropout masks) and
lstm_bwd_step_fused_kernel<RT,NW> (backward) are chosen from (B, U) by fwd_step_tile, fwd_masked_step_tile and bwd_step_tile.  The
sibling tests (test_lstm_seq_forward_backward, test_lstm_recurrent_dropout_matches_oracle, test_lstm_step_matches_sequence) leave
instances and branches that only the model tests reach, at model tolerance: forward <2,4>, backward <2,4>, backward <1,4> with masks,
a wave's K share of 3, 7 or 15 chunks (a partly clamped first prefetch ring, a partial second one), a block whose second row tile lies
wholly past B, both sides of every rule's threshold, the step-by-step decode on 64-row blocks, and the descriptor branches
accumulate_dU, dU_rec = NULL, dh_last without dh_seq and T == 1.  Every case here FIRST asserts the block the library's own rule reports
(info= of the ops wrappers: dc_lstm_step_tile_config), then the values.

Reference: oracle.np_oracle.lstm_forward / lstm_backward in float64 with I = 4U and W = the identity, so that zx = x + b and the
oracle's dx IS dz: dz is compared element for element.  T = 3 gives two fused steps each way (t = 1, 2 forward, t = 0, 1 backward).
Outputs start as NaN and carry 64 sentinel rows behind the [T*B, .] view that is passed in: an element no block stored and a store from
a row tile past B both fail.

The hard-sigmoid derivative jumps from 0.2 to 0 at z = +-2.5; a device pre-activation that differs from the oracle's in the last fp32
bits could sit on the other side and move dz by O(0.1).  The inputs are therefore built so that the ORACLE's gate pre-activations stay
clear of the jump by w = 2e-5 * max(1, max|z|) -- the very bound asserted on the device's z -- by redrawing the x rows that come closer
(case()).  A device z that passes its check is then on the oracle's side of every kink, and no element is excluded anywhere.

Tolerances are the sibling tests' for the same kernels at larger K: 2e-5 of the output scale on h_seq, c_seq and the overwritten z,
5e-5 on dz, dU, dW = x^T dz and db = colsum(dz)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 64, 777.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def close(got, want, tol, what=""):
    got = got.detach().float().cpu().numpy().astype(np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1.0, float(np.abs(want).max()))
    diff = np.abs(got - want)
    diff[np.isnan(diff)] = np.inf                              # an element no block stored
    err = float(diff.max()) / scale
    if not err < tol:                                          # where, and how many: a lone entry reads differently from a spread-out excess
        at = np.unravel_index(int(diff.argmax()), diff.shape)
        raise AssertionError("%s: max err %.3e (scaled) exceeds %.1e at %s: got %.9g want %.9g; %d of %d entries above the tolerance"
                             % (what, err, tol, at, got[at], want[at], int((diff > tol * scale).sum()), diff.size))


def padded(rows, cols, fill=None):
    """[rows + PAD, cols]: NaN (or `fill`) in the rows the kernels own, the sentinel behind them."""
    buf = torch.full((rows + PAD, cols), float("nan"), device="cuda")
    if fill is not None:
        buf[:rows] = fill
    buf[rows:] = SENTINEL
    return buf


def sentinel_intact(buf, rows, what):
    assert bool((buf[rows:] == SENTINEL).all()), "%s: a store landed behind row T*B" % what


def tm(a):
    """[B, T, n] -> time-major [T*B, n]"""
    return np.transpose(a, (1, 0, 2)).reshape(a.shape[0] * a.shape[1], a.shape[2])


def f32(a):
    """rounded to float32 once, so that the device and the oracle read the same numbers"""
    return np.asarray(a, np.float32).astype(np.float64)


VARIANTS = ["plain", "seqmask", "recmasks"]        # no sequence mask / sequence mask / sequence mask + recurrent-dropout masks


class Case:
    pass


@functools.lru_cache(maxsize=3)
def case(B, U, variant, T=3):
    """Inputs and the oracle's forward for one (B, U, variant) -- treat as read-only.  Gradients come from grads()."""
    rng = np.random.default_rng(100000 * VARIANTS.index(variant) + 1000 * B + 10 * U + T)
    c = Case()
    c.B, c.U, c.T = B, U, T
    x = f32(rng.standard_normal((B, T, 4 * U)))
    c.Ur = f32(rng.standard_normal((U, 4 * U)) / np.sqrt(U))
    c.b = f32(0.1 * rng.standard_normal(4 * U))
    c.mask = None
    if variant != "plain":
        c.mask = rng.random((B, T)) > 0.3
        c.mask[0] = False                                   # a fully masked row
        c.mask[1] = True                                    # and a fully live one
    c.rm = O.recurrent_dropout_masks(rng, B, U, 0.2) if variant == "recmasks" else None
    c.dH = rng.standard_normal((B, T, U))
    c.dlast = rng.standard_normal((B, U))
    W = np.eye(4 * U)
    gates = np.r_[0:2 * U, 3 * U:4 * U]                     # i, f, o: the hard-sigmoid gates
    for _ in range(8):
        c.H, c.cache = O.lstm_forward(x, c.mask, W, c.Ur, c.b, rec_masks=c.rm)
        c.Z = np.stack([s[2] for s in c.cache["steps"]], axis=1)            # [B, T, 4U]
        w = 2e-5 * max(1.0, float(np.abs(c.Z).max()))
        near = (np.abs(np.abs(c.Z[:, :, gates]) - 2.5) < w).any(axis=(1, 2))
        if not near.any():
            break
        x[near] = f32(rng.standard_normal((int(near.sum()), T, 4 * U)))
    assert not near.any(), "%d rows still within %.1e of a hard-sigmoid kink after 8 rounds" % (int(near.sum()), w)
    c.x = x
    c.Cs = np.stack([s[1] for s in c.cache["steps"][1:]] + [c.cache["c_last"]], axis=1)      # c after every step [B, T, U]
    c.grads = {}
    return c


def grads(c, use_dh_seq=True, use_dh_last=True):
    """(dz [B,T,4U], dW, dU, db) of the oracle for this case's dH / dlast (W is the identity: dx is dz)."""
    key = (use_dh_seq, use_dh_last)
    if key not in c.grads:
        c.grads[key] = O.lstm_backward(c.dH if use_dh_seq else None, c.cache, dh_last=c.dlast if use_dh_last else None)
    return c.grads[key]


def device_operands(c):
    mk = None if c.mask is None else dev(c.mask.T.reshape(-1), torch.uint8)
    rmd = None if c.rm is None else dev(c.rm)
    return dev(c.Ur), mk, rmd


def forward(ops, c, operands, rec_masks="own"):
    """dc_lstm_seq_fwd_f32 on NaN-filled, sentinel-backed outputs -> (z, h_seq, c_seq, xt, info)."""
    Ud, mk, rmd = operands
    if rec_masks != "own":
        rmd = rec_masks
    n = c.T * c.B
    xt = tm(c.x)
    z = padded(n, 4 * c.U, dev(xt + c.b))                   # zx = x + b  (W is the identity)
    h, cs = padded(n, c.U), padded(n, c.U)
    info = {}
    ops.lstm_seq_fwd(z[:n], Ud, mk, c.B, c.T, h_seq=h[:n], c_seq=cs[:n], rec_masks=rmd, info=info)
    torch.cuda.synchronize()
    for name, buf in (("z", z), ("h_seq", h), ("c_seq", cs)):
        sentinel_intact(buf, n, name)
    return z[:n], h[:n], cs[:n], dev(xt), info


def backward(ops, c, operands, fwd, use_dh_seq=True, use_dh_last=True, **kw):
    """dc_lstm_seq_bwd_f32 on a NaN-filled, sentinel-backed dz -> (dz, dU, info)."""
    Ud, mk, rmd = operands
    z, h, cs = fwd[:3]
    n = c.T * c.B
    dz = padded(n, 4 * c.U)
    info = {}
    kw.setdefault("dU", torch.full((c.U, 4 * c.U), float("nan"), device="cuda"))
    got_dz, got_dU = ops.lstm_seq_bwd(z, Ud, mk, h, cs, c.B, c.T, dh_seq=dev(tm(c.dH)) if use_dh_seq else None,
                                      dh_last=dev(c.dlast) if use_dh_last else None, dz=dz[:n], rec_masks=rmd, info=info, **kw)
    torch.cuda.synchronize()
    sentinel_intact(dz, n, "dz")
    assert got_dz.data_ptr() == dz.data_ptr()
    return got_dz, got_dU, info


def forward_matches(c, fwd, what):
    z, h, cs = fwd[:3]
    close(z, tm(c.Z), 2e-5, what + " z")                    # first: the kink argument rests on it
    close(h, tm(c.H), 2e-5, what + " h_seq")
    close(cs, tm(c.Cs), 2e-5, what + " c_seq")


def backward_matches(ops, c, xt, got_dz, got_dU, want, what):
    dz, dW, dU, db = want
    close(got_dz, tm(dz), 5e-5, what + " dz")
    if got_dU is not None:
        close(got_dU, dU, 5e-5, what + " dU")
    close(ops.gemm(xt, got_dz, a_trans=True), dW, 5e-5, what + " dW")          # dkernel = x^T dz
    close(ops.colsum(got_dz), db, 5e-5, what + " db")


# ------------------------------------------------------------------------------------------------------------------------------------
# A. every instance, both sides of every threshold
# ------------------------------------------------------------------------------------------------------------------------------------
# The rules (kNumCU = 256):
#   forward, plain:      64 rows iff (U/8) * ceil(B/32) > 512; 8 waves iff 64 rows and U % 64 == 0, else 4; unfused iff U % 32 != 0
#   forward, rec_masks:  32 rows iff (U/16) * ceil(B/16) > 256, else 16; always 8 waves;               unfused iff U % 32 != 0
#   backward:            32 rows iff (U/16) * ceil(B/16) > 256, else 16; 8 waves iff U % 32 == 0;      unfused iff U % 16 != 0
# (B, U): (rows, waves) forward plain, forward with rec_masks, backward; (0, 0) = unfused.  K chunks per wave: forward plain U / waves / 8,
# forward with masks U / 2 / 16, backward 4U / waves / 16 -- the 3, 7 and 15 are why those shapes are here.
UNFUSED = (0, 0)
TABLE = [
    (37, 32, (32, 4), (16, 8), (16, 8)),         # 1 chunk everywhere
    (70, 64, (32, 4), (16, 8), (16, 8)),         # 2 chunks
    (37, 48, UNFUSED, UNFUSED, (16, 4)),         # backward <1,4>: 3 chunks
    (37, 96, (32, 4), (16, 8), (16, 8)),         # 3 chunks everywhere
    (256, 256, (32, 4), (16, 8), (16, 8)),       # 16 * 16 = 256: the last below the masked-forward / backward threshold
    (257, 256, (32, 4), (32, 8), (32, 8)),       # 16 * 17: the first above; 1 row in the last block
    (512, 256, (32, 4), (32, 8), (32, 8)),       # 32 * 16 = 512: the last below the forward threshold
    (513, 256, (64, 8), (32, 8), (32, 8)),       # 32 * 17: the first above; forward <2,8>, 4 chunks; the last block holds 1 row, its second tile none
    (576, 112, UNFUSED, UNFUSED, (16, 4)),       # 7 * 36 = 252: backward <1,4>, 7 chunks, the last below
    (577, 112, UNFUSED, UNFUSED, (32, 4)),       # 7 * 37 = 259: backward <2,4>, 7 chunks, the first above
    (280, 240, UNFUSED, UNFUSED, (32, 4)),       # backward <2,4>, 15 chunks
    (580, 224, (64, 4), (32, 8), (32, 8)),       # forward <2,4>, 7 chunks everywhere
    (260, 480, (64, 4), (32, 8), (32, 8)),       # forward <2,4>, 15 chunks everywhere
]
# K chunks per wave the issue names for a shape: (forward plain, forward with masks, backward); None = not the reason the shape is here
CHUNKS = {(37, 32): (1, 1, 1), (70, 64): (2, 2, 2), (37, 48): (None, None, 3), (37, 96): (3, 3, 3), (513, 256): (4, None, None),
          (576, 112): (None, None, 7), (577, 112): (None, None, 7), (280, 240): (None, None, 15), (580, 224): (7, 7, 7),
          (260, 480): (15, 15, 15)}


def tile_of(info):
    return info["rows"], info["waves"]


def ran_on(info, want, what):
    assert tile_of(info) == want, "%s: the library runs %d rows / %d waves, not the %d / %d this case is here for" % ((what,) + tile_of(info) + want)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,U,fwd_plain,fwd_rec,bwd", TABLE, ids=["%dx%d" % t[:2] for t in TABLE])
def test_every_step_instance(ops, B, U, fwd_plain, fwd_rec, bwd, variant):
    c = case(B, U, variant)
    operands = device_operands(c)
    what = "%dx%d %s" % (B, U, variant)
    fwd = forward(ops, c, operands)
    masked = variant == "recmasks"
    ran_on(fwd[4], fwd_rec if masked else fwd_plain, what + " forward")
    ch = CHUNKS.get((B, U), (None, None, None))
    rows, waves = tile_of(fwd[4])
    if ch[1 if masked else 0] is not None:
        assert (U // 2 // 16 if masked else U // waves // 8) == ch[1 if masked else 0]
    forward_matches(c, fwd, what)
    got_dz, got_dU, binfo = backward(ops, c, operands, fwd)
    ran_on(binfo, bwd, what + " backward")
    if ch[2] is not None:
        assert 4 * U // binfo["waves"] // 16 == ch[2]
    backward_matches(ops, c, fwd[3], got_dz, got_dU, grads(c), what)
    if masked:                                              # masks of ones == the plain recurrence
        ones = torch.ones((4, B, U), device="cuda")
        h_a = forward(ops, c, operands, rec_masks=ones)[1]
        h_b = forward(ops, c, operands, rec_masks=None)[1]
        close(h_a, h_b.cpu().numpy(), 1e-5, what + " masks of ones")


# ------------------------------------------------------------------------------------------------------------------------------------
# B. one step at a time equals the sequence, bit for bit, on wide blocks
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "repacked"])
@pytest.mark.parametrize("B,U,want", [(513, 256, (64, 8)), (260, 480, (64, 4))], ids=["513x256", "260x480"])
def test_step_by_step_equals_the_sequence_on_wide_blocks(ops, B, U, want, packed):
    T = 4
    rng = np.random.default_rng(B + U)
    z = (0.5 * rng.standard_normal((T * B, 4 * U))).astype(np.float32)
    Ur = (rng.standard_normal((U, 4 * U)) / np.sqrt(U)).astype(np.float32)
    mask = np.ones((T, B), np.uint8)
    mask[1:3, ::3] = 0                                 # holes in the middle of rows
    mask[0, 1::5] = 0                                  # and masked first steps (state stays zero)
    assert mask[:, 0].tolist() == [1, 0, 0, 1]
    Ud = dev(Ur)
    sinfo = {}
    h_seq, c_seq = ops.lstm_seq_fwd(dev(z), Ud, dev(mask.reshape(-1), torch.uint8), B, T, info=sinfo)
    ran_on(sinfo, want, "sequence")
    pk = ops.lstm_pack_urec(Ud) if packed else None
    h = c = None
    for t in range(T):
        info = {}
        h, c = ops.lstm_step(dev(z[t * B:(t + 1) * B]), Ud, h, c, dev(mask[t], torch.uint8), U_packed=pk, info=info)
        assert info == sinfo, (t, info, sinfo)
        assert torch.equal(h, h_seq[t * B:(t + 1) * B]), "h differs at step %d" % t
        assert torch.equal(c, c_seq[t * B:(t + 1) * B]), "c differs at step %d" % t
    hm = h_seq.view(T, B, U)
    assert torch.equal(hm[2, 0], hm[0, 0]) and not torch.equal(hm[3, 0], hm[2, 0])      # the carry over the hole


# ------------------------------------------------------------------------------------------------------------------------------------
# C. descriptor branches, on both dU paths: one GEMM (37 x 96), four per-gate GEMMs (577 x 112 with rec_masks)
# ------------------------------------------------------------------------------------------------------------------------------------
BRANCH_CASES = [(37, 96, "seqmask"), (577, 112, "recmasks")]
BRANCH_IDS = ["37x96", "577x112-recmasks"]


@functools.lru_cache(maxsize=2)
def normal_run(ops, B, U, variant):
    """The forward and the plain backward (dh_seq + dh_last, dU written) the branch tests compare with -- treat as read-only."""
    c = case(B, U, variant)
    operands = device_operands(c)
    fwd = forward(ops, c, operands)
    got_dz, got_dU, _ = backward(ops, c, operands, fwd)
    return c, operands, fwd, got_dz, got_dU


@pytest.mark.parametrize("B,U,variant", BRANCH_CASES, ids=BRANCH_IDS)
def test_accumulate_dU(ops, B, U, variant):
    c, operands, fwd, dz0, _ = normal_run(ops, B, U, variant)
    dU0 = np.random.default_rng(5).standard_normal((U, 4 * U)).astype(np.float32)
    got_dz, got_dU, _ = backward(ops, c, operands, fwd, dU=dev(dU0), accumulate_dU=True)
    close(got_dU, dU0.astype(np.float64) + grads(c)[2], 5e-5, "dU0 + dU")
    assert torch.equal(got_dz, dz0)


@pytest.mark.parametrize("B,U,variant", BRANCH_CASES, ids=BRANCH_IDS)
def test_dU_left_to_the_caller(ops, B, U, variant):
    c, operands, fwd, dz0, _ = normal_run(ops, B, U, variant)
    got_dz, got_dU, _ = backward(ops, c, operands, fwd, dU=False)
    assert got_dU is None
    assert torch.equal(got_dz, dz0)


@pytest.mark.parametrize("use_dh_seq,use_dh_last", [(False, True), (True, False)], ids=["dh_last-only", "dh_seq-only"])
@pytest.mark.parametrize("B,U,variant", BRANCH_CASES, ids=BRANCH_IDS)
def test_one_gradient_input(ops, B, U, variant, use_dh_seq, use_dh_last):
    c, operands, fwd, _, _ = normal_run(ops, B, U, variant)
    got_dz, got_dU, _ = backward(ops, c, operands, fwd, use_dh_seq=use_dh_seq, use_dh_last=use_dh_last)
    backward_matches(ops, c, fwd[3], got_dz, got_dU, grads(c, use_dh_seq, use_dh_last), "one gradient input")


@pytest.mark.parametrize("variant", ["seqmask", "recmasks"])
@pytest.mark.parametrize("B,U", [t[:2] for t in BRANCH_CASES], ids=["37x96", "577x112"])
def test_a_single_timestep(ops, B, U, variant):
    """T == 1: no recurrent product anywhere, so dU is all zeros -- written, or with accumulate_dU left alone."""
    c = case(B, U, variant, T=1)
    operands = device_operands(c)
    what = "%dx%d %s T=1" % (B, U, variant)
    fwd = forward(ops, c, operands)
    forward_matches(c, fwd, what)
    got_dz, got_dU, _ = backward(ops, c, operands, fwd)                        # dU starts as NaN
    assert bool((got_dU == 0).all()), "a NaN-filled dU must come back all zeros"
    assert not np.any(grads(c)[2])
    backward_matches(ops, c, fwd[3], got_dz, got_dU, grads(c), what)
    dU0 = torch.randn((U, 4 * U), device="cuda")
    acc_dz, acc_dU, _ = backward(ops, c, operands, fwd, dU=dU0.clone(), accumulate_dU=True)
    assert torch.equal(acc_dU, dU0), "accumulate_dU at T == 1 must leave dU alone"
    assert torch.equal(acc_dz, got_dz)


# ------------------------------------------------------------------------------------------------------------------------------------
# D. refusals of the query
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_query_refuses_bad_arguments(ops):
    from image_captioning_amd import _lib
    query = _lib.load().dc_lstm_step_tile_config
    rows, waves = C.c_int(-7), C.c_int(-7)
    for B, U in ((0, 64), (-3, 64), (37, 0), (37, -32), (37, 30), (37, 34)):
        for direction in (0, 1):
            assert query(B, U, direction, 0, C.byref(rows), C.byref(waves)) == _lib.EINVAL, (B, U, direction)
    assert query(37, 64, 0, 0, None, C.byref(waves)) == _lib.EINVAL
    assert query(37, 64, 1, 1, C.byref(rows), None) == _lib.EINVAL
    assert query(37, 64, 2, 0, C.byref(rows), C.byref(waves)) == _lib.EINVAL
    assert (rows.value, waves.value) == (-7, -7)           # a refusal writes nothing
    assert query(37, 36, 0, 0, C.byref(rows), C.byref(waves)) == _lib.OK and (rows.value, waves.value) == UNFUSED       # U % 4 == 0: unfused
    assert query(37, 36, 1, 0, C.byref(rows), C.byref(waves)) == _lib.OK and (rows.value, waves.value) == UNFUSED
    assert query(37, 64, 0, 1, C.byref(rows), C.byref(waves)) == _lib.OK and (rows.value, waves.value) == (16, 8)
