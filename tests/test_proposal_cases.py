"""The inputs of test_gpu_proposals.py have the properties they exist for (CPU: the oracle alone, no library loaded).

Every case of _proposal_cases.py names its guards: a kept box of the first group that suppresses a candidate in the second removed-set
register of the wave scan, `kept < count` after a full scan, `count` reached in the middle of a chunk, a chunk that keeps more rows than
the scan fetches at a time, an IoU that equals the threshold in float32, ...  The guards are evaluated on the oracle's answer, here from
host-computed scores and in the GPU test from the device's own, so a case that has lost its property is red wherever the suite runs.
The kernel constants the guards use are parsed from proposal.hip."""
import numpy as np
import pytest

import _proposal_cases as P
from oracle import np_oracle as O


def test_the_kernel_constants_are_read_from_the_source(repo_root):
    c = P.kernel_constants(repo_root)
    assert c["G"] >= 2 and c["ROWS"] >= 1 and c["MAX_WORDS"] > P.LANES and c["MAX_K"] == c["MAX_WORDS"] * P.LANES
    # the cases were sized for these values: a retuned kernel has to revisit them
    assert (c["G"], c["ROWS"], c["MAX_WORDS"]) == (8, 24, 128)


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_case_has_the_property_it_exists_for(repo_root, name):
    case = P.build(name)
    assert case.B >= 2 and case.logits.shape == (case.B, case.N) and case.anchors.shape == (case.N, 4)
    assert not np.array_equal(case.logits[0], case.logits[1])                        # the images rank the boxes differently
    assert case.heads().shape == (case.B, 1, case.N, 6) and not case.heads()[..., 2:].any()
    scores = P.host_scores(case.logits)
    refs = P.reference(case, scores)
    print(name, "N %d k %d words %d count %d thr %g:" % (case.N, case.k, case.words, case.count, case.thr), P.check_guards(case, refs, P.kernel_constants(repo_root)))
    for b, r in enumerate(refs):                                                     # the ranking is the intended one, ties by anchor index
        np.testing.assert_array_equal(r["order"], np.lexsort((np.arange(case.N), -case.logits[b].astype(np.float64)))[:min(case.k, case.N)])


def test_the_cases_cover_both_scan_kernels_and_the_register_boundary(repo_root):
    c = P.kernel_constants(repo_root)
    words = {n: P.build(n).words for n in P.CASE_NAMES}
    assert {P.LANES, P.LANES + 1, c["MAX_WORDS"], c["MAX_WORDS"] + 1, c["G"], c["G"] + 1, 1} <= set(words.values())
    assert sum(w > c["MAX_WORDS"] for w in words.values()) >= 3


def test_a_guard_fails_on_a_case_without_its_property(repo_root):
    """The guards can fail: sparse boxes reach `count` early, with more than one survivor, in the wave scan."""
    case = P.build("sparse_6000")
    refs = P.reference(case, P.host_scores(case.logits))
    for wrong in ({"wave": None, "one_kept": (0,)}, {"wave": None, "kept_lt_count": None}, {"wave": None, "last_group": (1,)}, {"serial": None}):
        case.guards = wrong
        with pytest.raises(AssertionError):
            P.check_guards(case, refs, P.kernel_constants(repo_root))


def test_the_pyramid_inputs_keep_their_last_box_beyond_rank_4096():
    heads, anchors, cls, box = P.pyramid_inputs(0)
    assert anchors.shape == (65472, 4)
    scores = O.softmax(cls)[:, :, 1].astype(np.float32)
    print([int(kp[-1]) for _, _, kp in P.pyramid_reference(scores, box, anchors)])
