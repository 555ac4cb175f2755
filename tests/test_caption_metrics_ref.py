"""The host path of caption_metrics.py against vectors recorded from the reference's own Bleu(4), Rouge() and Cider() and from its
evaluate loop (tests/golden/make_caption_metric_vectors.py wrote tests/golden/caption_metrics_reference.npz).  CPU-only.

BLEU and ROUGE (rouge="reference") must EQUAL the recorded float64 values: the host path performs the scorers' operations in their
order.  CIDEr within rtol 1e-12 (its sums over dictionaries have no fixed order).  The integer statistics are exact."""
import os
import sys

import numpy as np
import pytest

from image_captioning_amd import caption_metrics as cm
from image_captioning_amd.score_dense_captions import DenseCaptioningEvaluator

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def vec():
    return dict(np.load(os.path.join(GOLDEN, "caption_metrics_reference.npz")))


@pytest.fixture(scope="module")
def batch(vec):
    return cm.CaptionBatch(*(vec[k] for k in cm.CaptionBatch.FIELDS))


@pytest.fixture(scope="module")
def host(batch):
    return cm.score(batch)


def test_the_fixture_holds_the_cases_it_is_for(vec):
    sys.path.insert(0, GOLDEN)
    try:
        from make_caption_metric_vectors import check_conditions
    finally:
        sys.path.remove(GOLDEN)
    check_conditions(vec)
    assert os.path.getsize(os.path.join(GOLDEN, "caption_metrics_reference.npz")) < 200 * 1024
    assert vec["cand"].shape[0] == 67 and vec["cand"].dtype == np.int32


def test_bleu_equals_the_reference(vec, host):
    assert host["BLEU"].dtype == np.float64 and host["BLEU"].shape == vec["BLEU"].shape
    assert (host["BLEU"] == vec["BLEU"]).all()
    assert (host["BLEU_corpus"] == vec["BLEU_corpus"]).all()
    assert (vec["BLEU"] == 0.0).any() and (vec["BLEU"] > 0.5).any()          # the brevity factor underflows for an empty candidate


def test_rouge_reference_mode_equals_the_reference(vec, host):
    assert (host["ROUGE"] == vec["ROUGE"]).all() and host["ROUGE_mean"] == vec["ROUGE_mean"]
    assert (vec["ROUGE"] == 0.0).any()


def test_cider_matches_the_reference(vec, host):
    np.testing.assert_allclose(host["CIDER"], vec["CIDER"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(host["CIDER_mean"], vec["CIDER_mean"], rtol=1e-12, atol=0)
    assert host["CIDER"][0] == 0.0                                           # the group of one record
    assert vec["CIDER"].max() > 1.0


def test_statistics_are_exact(vec, host):
    assert host["stats"].dtype == np.int32 and (host["stats"] == vec["stats"]).all()
    assert (host["stats"][:, 11] == 0).all()


def test_one_metric_alone_gives_the_same_values(batch, host):
    for m in cm.METRICS:
        alone = cm.score(batch, metrics=m)
        assert (alone[m] == host[m]).all() and not (set(cm.METRICS) - {m}) & set(alone)


def test_pack_captions_round_trips_the_fixture(vec, host):
    C = [vec["cand"][i, :n].tolist() for i, n in enumerate(vec["cand_len"])]
    R = [[vec["refs"][j, :vec["ref_len"][j]].tolist() for j in range(a, b)] for a, b in zip(vec["ref_start"][:-1], vec["ref_start"][1:])]
    packed = cm.pack_captions(C, R, groups=vec["group_start"])
    assert (packed.ref_start == vec["ref_start"]).all() and (packed.cand_len == vec["cand_len"]).all()
    again = cm.score(packed)                                                 # zero padding here, word-like padding in the fixture
    for m in cm.METRICS + ("stats",):
        assert (again[m] == host[m]).all()


def test_evaluate_from_equals_the_recorded_dictionary(vec):
    records, at = [], 0
    for c in vec["ev_per_image"]:
        records.append([{"ok": int(vec["ev_ok"][i]), "ov": float(vec["ev_ov"][i]), "references": [["y"]] if vec["ev_has_ref"][i] else []}
                        for i in range(at, at + c)])
        at += c
    got = DenseCaptioningEvaluator.evaluate_from(records, vec["ev_scores"], int(vec["ev_npos"]))
    assert list(got["ap_breakdown"]) == vec["ev_ap_keys"].tolist() and list(got["det_breakdown"]) == vec["ev_det_keys"].tolist()
    assert len(got["ap_breakdown"]) == 30 and len(got["det_breakdown"]) == 5
    assert (np.array(list(got["ap_breakdown"].values())) == vec["ev_ap_values"]).all()
    assert (np.array(list(got["det_breakdown"].values())) == vec["ev_det_values"]).all()
    assert got["map"] == vec["ev_map"] and got["detmap"] == vec["ev_detmap"]
    assert len(set(vec["ev_ap_values"].tolist())) > 5 and vec["ev_map"] > 0
    flat = [r for image in records for r in image]
    assert DenseCaptioningEvaluator.evaluate_from(flat, vec["ev_scores"], int(vec["ev_npos"]))["map"] == got["map"]


def _textbook_lcs(a, b):
    table = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            table[i][j] = table[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(table[i - 1][j], table[i][j - 1])
    return table[len(a)][len(b)]


def _rouge_from(lcs, lc, lrs):
    p = max(l / max(lc, 1) for l in lcs)
    r = max(l / max(lr, 1) for l, lr in zip(lcs, lrs))
    return (1 + 1.2 ** 2) * p * r / (r + 1.2 ** 2 * p) if p != 0 and r != 0 else 0.0


def test_rouge_lcs_mode_is_the_textbook_dp(vec, batch, host):
    got = cm.score(batch, metrics="ROUGE", rouge="lcs")
    differs = 0
    for i in range(batch.N):
        c = vec["cand"][i, :vec["cand_len"][i]].tolist()
        rs = [vec["refs"][j, :vec["ref_len"][j]].tolist() for j in range(vec["ref_start"][i], vec["ref_start"][i + 1])]
        lcs = [_textbook_lcs(r, c) for r in rs]
        assert got["stats"][i, cm.STAT_LCS_MAX] == max(lcs)
        assert got["ROUGE"][i] == pytest.approx(_rouge_from(lcs, len(c), [len(r) for r in rs]), rel=1e-15, abs=0)
        differs += got["ROUGE"][i] != host["ROUGE"][i]
    assert differs >= 10                                                     # the fork's value is not the LCS


def test_the_my_lcs_quirk_is_pinned_in_both_modes():
    """my_lcs("a b c d e", "e d c") returns 3 in the reference's fork (every token of the shorter sentence occurs in the longer one);
    the longest common subsequence has length 1."""
    a, b, c, d, e = range(5)
    one = cm.pack_captions([[e, d, c]], [[[a, b, c, d, e]]])
    quirk, true = cm.score(one, metrics="ROUGE"), cm.score(one, metrics="ROUGE", rouge="lcs")
    assert quirk["stats"][0, cm.STAT_LCS_MAX] == 3 and true["stats"][0, cm.STAT_LCS_MAX] == 1
    assert quirk["ROUGE"][0] == _rouge_from([3], 3, [5]) and true["ROUGE"][0] == _rouge_from([1], 3, [5])
    swapped = cm.pack_captions([[a, b, c, d, e]], [[[e, d, c]]])             # the shorter sentence is the reference
    assert cm.score(swapped, metrics="ROUGE")["stats"][0, cm.STAT_LCS_MAX] == 3
    equal = cm.pack_captions([[a, a, b]], [[[a, c, c]]])                     # equal lengths: the candidate's positions count (2, not 1)
    assert cm.score(equal, metrics="ROUGE")["stats"][0, cm.STAT_LCS_MAX] == 2


def test_score_predictions_and_the_default_tokenizer():
    gens = {"a": ["A man rides a horse."], "b": ["two dogs, playing"]}
    refs = {"a": ["a man rides a horse", "A person on a horse!"], "b": ["Two dogs play."]}
    keys, cands, rlists, word_to_id = cm.encode_strings(gens, refs)
    assert keys == ["a", "b"] and "." not in word_to_id and "," not in word_to_id and "man" in word_to_id
    assert cands[0] == rlists[0][0]                                          # case and the final period are gone
    out = cm.score_predictions(gens, refs)
    assert sorted(out) == ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "CIDEr", "ROUGE_L"]
    assert 0.5 < out["Bleu_1"] <= 1.0 and 0.5 < out["ROUGE_L"] <= 1.0 and np.isfinite(out["CIDEr"])
    ids = cm.score_predictions(gens, refs, tokenizer=str.split)
    assert ids["Bleu_1"] < out["Bleu_1"]                                     # "horse." is not "horse" for a whitespace tokenizer


def test_score_captions_aligns_with_the_records_and_marks_the_reference_less():
    ev = DenseCaptioningEvaluator(None, None, "CIDER", None, None, None, None, "t")
    records = [[{"ok": 1, "ov": 0.8, "candidate": "a red car", "references": [["a red car"], ["the car is red"]]},
                {"ok": 0, "ov": 0.0, "candidate": "a tree", "references": []}],
               [{"ok": 1, "ov": 0.6, "candidate": "a tall tree", "references": ["a tall green tree"]}]]
    for method, shape in (("ROUGE", (3,)), ("CIDER", (3,)), ("BLEU", (4, 3))):
        s = ev.score_captions(records, method)
        assert s.shape == shape and np.isnan(s[..., 1]).all() and np.isfinite(s[..., [0, 2]]).all()
    assert ev.score_captions(records, "ROUGE")[0] == 1.0
