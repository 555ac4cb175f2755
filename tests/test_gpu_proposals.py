"""Non-maximum suppression of the ProposalLayer, bit for bit against the oracle at production sizes (-m gpu).

The anchors are the boxes (see _proposal_cases.py): one level, one anchor per location, zero box logits, so the decode is exact and the
device's `order`, `keep` and `proposals` must EQUAL O.proposal_layer's, started from the device's own scores.  The cases reach what the
pyramid tests of test_gpu_kernels.py do not: kept boxes that suppress candidates in words 64 and above of the wave scan's removed-set
(its second register, the `lane + 64` row loads, the hand-over between the two), the last groups, `kept < count` after a full scan,
chunks that keep more rows than one fetch holds, IoU exactly at the threshold, `count > k`, the 64 / 65 and 128 / 129 word boundaries,
and every word of the serial scan above 8192 candidates.  Each case first asserts, on the oracle's answer, the property it exists for
(test_proposal_cases.py does the same without a GPU)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _proposal_cases as P
from oracle import np_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.0                                       # what `out=` holds before the call: every row has to be written


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


class Inputs:
    """A case's tensors on the device (made once; the calls under test only launch)."""

    def __init__(self, case):
        self.case = case
        self.heads, self.anchors = [dev(case.heads())], dev(case.anchors)

    def run(self, ops):
        c = self.case
        out = torch.full((c.B, c.count, 4), SENTINEL, dtype=torch.float32, device="cuda")
        props, (scores, order, keep) = ops.rpn_proposals(self.heads, self.anchors, c.image_hw, c.count, c.thr, pre_nms_limit=c.k,
                                                         anchors_per_loc=1, out=out, debug=True)
        assert props.data_ptr() == out.data_ptr()
        return {"scores": scores.cpu().numpy(), "order": order.cpu().numpy(), "keep": keep.cpu().numpy(), "proposals": props.cpu().numpy()}


def guarded_reference(case, scores):
    refs = P.reference(case, scores)
    print(case.name, "words %d:" % case.words, P.check_guards(case, refs, P.kernel_constants(ROOT)))
    return refs


def assert_equals_oracle(case, got, refs):
    k = min(case.k, case.N)
    assert got["order"].shape == (case.B, k) and got["keep"].shape == (case.B, case.count) and got["proposals"].shape == (case.B, case.count, 4)
    for b, r in enumerate(refs):
        n = len(r["keep"])
        print("  image %d: oracle keeps %d, device keeps %d" % (b, n, int((got["keep"][b] >= 0).sum())))
        np.testing.assert_array_equal(got["order"][b], np.argsort(-got["scores"][b].astype(np.float64), kind="stable")[:k])
        np.testing.assert_array_equal(got["order"][b], r["order"])
        np.testing.assert_array_equal(got["keep"][b][:n], r["keep"])
        assert np.all(got["keep"][b][n:] == -1)
        np.testing.assert_array_equal(got["proposals"][b][:n], r["proposals"][:n])          # zero box logits: bit for bit
        assert np.all(got["proposals"][b][n:] == 0)


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_nms_equals_the_oracle(ops, name):
    case = P.build(name)
    got = Inputs(case).run(ops)
    assert np.abs(got["scores"] - P.host_scores(case.logits)).max() < 1e-6
    assert_equals_oracle(case, got, guarded_reference(case, got["scores"]))


def _workspace(ops, inp):
    """The scratch buffer the next rpn_proposals call of these inputs is handed (the size query rpn_proposals makes)."""
    from image_captioning_amd import _lib
    c = inp.case
    d = _lib.ProposalDesc()
    d.B, d.levels, d.anchors_per_loc, d.A_total = c.B, 1, 1, c.N
    d.heads[0], d.Hs[0], d.Ws[0] = inp.heads[0].data_ptr(), 1, c.N
    d.anchors = d.proposals = inp.anchors.data_ptr()                     # (validated for null and alignment only)
    d.pre_nms_limit, d.proposal_count = c.k, c.count
    nbytes = _lib.load().dc_proposals_workspace_bytes(C.byref(d))
    assert nbytes > c.B * c.k * c.words * 8
    ws, _ = ops.WORKSPACE.get(nbytes, "cuda")
    return ws


@pytest.mark.parametrize("name", ["clustered300_6000", "clustered100_4097", "clustered300_4097"])
def test_nms_ignores_what_the_workspace_held(ops, name):
    """nms_mask_kernel writes no word left of the diagonal and the wave scan reads whole rows: what the scratch buffer held before
    (all ones, all zeros) must not reach the result.  (The planted k = 4097 cases are here too: a scan that took the removed-word of
    rank 4096 from the wrong register would read such a stale word, and could pass or fail by what an earlier test left there.)"""
    case = P.build(name)
    inp = Inputs(case)
    runs = []
    for fill in (0xFF, 0x00):
        ws = _workspace(ops, inp)
        ws.fill_(fill)
        runs.append(inp.run(ops))
        assert _workspace(ops, inp).data_ptr() == ws.data_ptr()          # the call did use the buffer that was filled
    refs = guarded_reference(case, runs[0]["scores"])
    for got in runs:
        assert_equals_oracle(case, got, refs)
    for key in runs[0]:
        np.testing.assert_array_equal(runs[0][key], runs[1][key])


@pytest.mark.parametrize("name", ["clustered1500_6000", "clustered500_12000"])
def test_nms_is_identical_from_call_to_call(ops, name):
    """Five calls, bit-equal outputs (the wave scan passes keep masks, removed-words and its stop flag between waves through LDS)."""
    case = P.build(name)
    inp = Inputs(case)
    runs = [inp.run(ops) for _ in range(5)]
    assert_equals_oracle(case, runs[0], guarded_reference(case, runs[0]["scores"]))
    for got in runs[1:]:
        for key in got:
            np.testing.assert_array_equal(got[key], runs[0][key])


def test_both_scan_kernels_on_the_same_boxes(ops):
    """k = 8192 (the wave scan's largest) and k = 8193 (the serial scan's smallest) over the same boxes and rankings, each against the
    oracle; the survivors among the first 8192 candidates are the same, so the two kernels are held to one answer."""
    results = []
    for name in ("clustered40_8192", "clustered40_8193"):
        case = P.build(name)
        got = Inputs(case).run(ops)
        assert_equals_oracle(case, got, guarded_reference(case, got["scores"]))
        results.append((case, got))
    (wave_case, wave), (serial_case, serial) = results
    np.testing.assert_array_equal(wave_case.anchors, serial_case.anchors)
    np.testing.assert_array_equal(wave_case.logits, serial_case.logits)
    for b in range(wave_case.B):
        w, s = wave["keep"][b], serial["keep"][b]
        np.testing.assert_array_equal(w[w >= 0], s[(s >= 0) & (s < wave_case.k)])


def test_pyramid_at_the_production_shape_scans_past_rank_4096(ops):
    """512 x 512, five levels, three anchors, 65 472 -> 6000 -> 2000 at 0.7, with heads for which the 2000th survivor lies beyond rank
    4096: `order` and `keep` exact, the boxes to the last bit of expf()."""
    heads, anchors, cls, box = P.pyramid_inputs(0)
    S, count, pre, thr = P.PYRAMID["S"], P.PYRAMID["count"], P.PYRAMID["k"], P.PYRAMID["thr"]
    B = cls.shape[0]
    out = torch.full((B, count, 4), SENTINEL, dtype=torch.float32, device="cuda")
    props, (scores, order, keep) = ops.rpn_proposals([dev(h) for h in heads], dev(anchors), (S, S), count, thr, pre_nms_limit=pre, out=out,
                                                     debug=True)
    scores, order, keep, props = scores.cpu().numpy(), order.cpu().numpy(), keep.cpu().numpy(), props.cpu().numpy()
    assert np.abs(scores - O.softmax(cls)[:, :, 1]).max() < 1e-6
    refs = P.pyramid_reference(scores, box, anchors)
    print("last kept ranks:", [int(kp[-1]) for _, _, kp in refs])
    for b, (want, ix, kp) in enumerate(refs):
        np.testing.assert_array_equal(order[b], ix)
        np.testing.assert_array_equal(keep[b][:len(kp)], kp)
        assert np.all(keep[b][len(kp):] == -1)
        # box values: the device's expf and numpy's float32 exp may differ in the last bit
        np.testing.assert_allclose(props[b], want, rtol=3e-7, atol=1e-7)
