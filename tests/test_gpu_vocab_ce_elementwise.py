"""dc_vocab_ce (every route) and dc_softmax_ce_f32 held PER ELEMENT on exact logits (-m gpu).  tests/_vocab_ce_cases.py has the
cases, the float64 reference, the bounds and their constants; tests/test_vocab_ce_cases.py proves on the host that the cases are
what this file takes them for and that the comparison sees what the max-norm assertions of tests/test_gpu_bf16.py let pass.

Every output starts as a sentinel inside a sentinel ring; the pad columns V .. lddl - 1 of a bf16 gradient must be zero.  The route
shows in the result itself: the parked (materialised) route is held to the reference of bf16_of(z), the recomputing routes to the
reference of z, and the two lie further apart than the bound on most entries (asserted on the host) -- a call that silently took the
other route fails.  One reference per case, shared by the routes that compute it.  Each test prints its worst ratios
("vocab-ce-elementwise ...": run with -s to see them)."""
import numpy as np
import pytest
import torch

import _placement_cases as P
import _vocab_ce_cases as C

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PAD = 8                                                          # bf16 gradient: lddl = V + 8 (rows stay 16-byte aligned)


@pytest.fixture(scope="module", autouse=True)
def _release_the_cases():
    """The cached cases and references hold hundreds of megabytes: gone when this module is done."""
    yield
    C.clear_caches()


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def _out(shape, dtype=torch.float32, ld=None):
    return P.carve(P.sentinel_like(shape, dtype), 0, ld)


def _f32(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.detach().view(torch.int16).cpu().numpy().view(np.uint16)


def _settle(verdicts, case):
    for v in verdicts.values():
        print(v.line(case))
    failing = [v.report() for v in verdicts.values() if not v.ok]
    assert not failing, "%s\n%s" % (case, "\n".join(failing))


# (case, route), the routes of one case side by side: they share its reference
CASE_ROUTES = [(M, V, K, v, route) for (M, V, K, v) in C.all_cases() for route, spec in C.ROUTES.items() if (M, V, K) in spec[3]]


@pytest.mark.parametrize("M,V,K,variation,route", CASE_ROUTES)
def test_vocab_ce_elementwise(ops, M, V, K, variation, route):
    """loss_rows, dlogits (fp32 or bf16) and dbias of one route on one case against the float64 reference of the EXACT logits, entry by
    entry; a loss-only call returns the same loss bit for bit (on the parked route it has no buffer to park in and recomputes: it is
    held to the reference of the unrounded logits instead)."""
    operand, grad, parked, _, _ = C.ROUTES[route]
    c = C.operands(M, V, K, variation)
    case = "%s %s [%s]" % ((M, V, K), variation, route)
    Xd, Wd = P.dev(c["X"]), P.dev(c["W"])
    if operand == "bf16":
        Xd, Wd = ops.to_bf16(Xd), ops.to_bf16(Wd)
        assert torch.equal(Xd.float(), P.dev(c["X"])) and torch.equal(Wd.float(), P.dev(c["W"]))          # the grids are exact in bf16
    bias, t = P.dev(c["bias"]), P.dev(c["t"], torch.int32)
    kw = dict(grad_scale=c["gs"], keras_sparse=c["keras_sparse"], row_weights=None if c["w"] is None else P.dev(c["w"]))
    loss, db = _out((M,)), _out((V,))
    dl = _out((M, V), ld=V + 4) if grad == "f32" else _out((M, V + PAD), BF)
    assert dl.data_ptr() % 16 == 0 and (dl.stride(0) * dl.element_size()) % 16 == 0
    ops.vocab_ce(Xd, Wd, bias, t, loss_rows=loss, dlogits=dl, dbias=db, materialize_bf16=parked, **kw)
    only = _out((M,))
    ops.vocab_ce(Xd, Wd, bias, t, loss_rows=only, materialize_bf16=parked, **kw)
    torch.cuda.synchronize()
    for name, o in (("loss_rows", loss), ("dbias", db), ("dlogits", dl), ("loss_rows of the loss-only call", only)):
        assert P.untouched_outside(o), "%s: written outside %s" % (case, name)
    ref = C.reference(M, V, K, variation, parked)
    const = C.CONST["fast"][variation]
    if grad == "f32":
        verdicts = C.compare_outputs(ref, const, loss=_f32(loss), g=_f32(dl), dbias=_f32(db))
    else:
        bits = _bits(dl)
        assert not bits[:, V:].any(), "%s: the pad columns V .. lddl - 1 must be zero" % case
        verdicts = C.compare_outputs(ref, const, loss=_f32(loss), g_bits=bits[:, :V], dbias=_f32(db))
    if parked:
        plain = C.reference(M, V, K, variation, False)
        verdicts["loss-only"] = C.compare_f32(_f32(only), plain["loss"], plain["A_loss"], np.zeros(M), const["loss"], "loss_rows (loss-only call)")
    else:
        assert torch.equal(only, loss), "%s: the loss-only call's loss differs from the full call's" % case
    _settle(verdicts, case)


SOFTMAX = [(M, V, K, v, inplace) for (M, V, K) in C.SOFTMAX_SHAPES for v in C.variations(M, V, K) for inplace in (False, True)]


@pytest.mark.parametrize("M,V,K,variation,inplace", SOFTMAX)
def test_softmax_ce_elementwise(ops, M, V, K, variation, inplace):
    """The unfused fallback (dc_softmax_ce_f32, one block per row) on the grid logits themselves: probs, loss_rows and dlogits, the
    gradient written beside the logits or over them; V % 4 != 0 runs the scalar loops."""
    c = C.softmax_operands(M, V, K, variation)
    ref = C.reference(M, V, K, variation, False, True)
    case = "%s %s [softmax_ce%s]" % ((M, V, K), variation, ", in place" if inplace else "")
    t = P.dev(c["t"], torch.int32)
    kw = dict(grad_scale=c["gs"], keras_sparse=c["keras_sparse"], row_weights=None if c["w"] is None else P.dev(c["w"]))
    z = P.carve(P.dev(c["z"]), 0)
    loss, probs = _out((M,)), _out((M, V))
    dl = z if inplace else _out((M, V))
    ops.softmax_ce(z, t, probs=probs, loss_rows=loss, dlogits=dl, **kw)
    only = _out((M,))
    ops.softmax_ce(P.dev(c["z"]), t, loss_rows=only, **kw)
    torch.cuda.synchronize()
    for name, o in (("loss_rows", loss), ("probs", probs), ("dlogits", dl), ("loss_rows of the loss-only call", only)):
        assert P.untouched_outside(o), "%s: written outside %s" % (case, name)
    if not inplace:
        assert torch.equal(z, P.dev(c["z"])), "%s: the logits changed" % case
    assert torch.equal(only, loss), "%s: the loss-only call's loss differs from the full call's" % case
    _settle(C.compare_outputs(ref, C.CONST["libm"][variation], loss=_f32(loss), g=_f32(dl), probs=_f32(probs)), case)
