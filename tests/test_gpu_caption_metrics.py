"""The device path of the caption metrics (csrc/caption_metrics.hip: dc_caption_metrics_f64, dc_caption_cider_f64) against the vectors
recorded from the reference's scorers and against the package's host path.

Tolerances are derived, not measured.  The integer statistics are exact.  A BLEU / ROUGE value is a few dozen float64 roundings (the
products, one pow, one exp, the divisions): <= 1e-14 relative, held to rtol 1e-9, and exactly 0.0 where the reference is (an
underflowed brevity factor, a ROUGE without a common word).  CIDEr adds the cancellation in log N - log df: at df = N - 1 the
difference is about 1 / N, so 2 ulp of log N (2.2e-16 * log N) are amplified by about N log N -- below 1e-11 for N <= 2048 -- held to
rtol 1e-9 with atol 1e-12 for the scores that cancel to (almost) nothing.  A missed or doubled n-gram moves a score by >= 1e-3."""
import os

import numpy as np
import pytest
import torch

from image_captioning_amd import caption_metrics as cm

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "caption_metrics_reference.npz")
VOCAB = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 2 ** 31 - 1], np.int64)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def vec():
    return dict(np.load(GOLDEN))


def _to_device(batch):
    return cm.CaptionBatch(*(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in batch.host()))


def _np(res):
    return {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in res.items()}


def _compare(got, want, note):
    """got: a device result (as NumPy), want: the reference or the host path."""
    assert got["stats"].dtype == np.int32 and (got["stats"] == want["stats"]).all(), note
    worst = 0.0
    for m in ("BLEU", "ROUGE", "BLEU_corpus", "ROUGE_mean"):
        g, w = np.asarray(got[m]), np.asarray(want[m])
        assert g.dtype == np.float64 and g.shape == w.shape, (note, m)
        assert ((g == 0.0) == (w == 0.0)).all(), (note, m)
        np.testing.assert_allclose(g, w, rtol=1e-9, atol=0, err_msg="%s %s" % (note, m))
        worst = max(worst, float(np.max(np.abs(g - w) / np.where(w == 0, 1.0, np.abs(w)), initial=0.0)))
    for m in ("CIDER", "CIDER_mean"):
        g, w = np.asarray(got[m]), np.asarray(want[m])
        np.testing.assert_allclose(g, w, rtol=1e-9, atol=1e-12, err_msg="%s %s" % (note, m))
        worst = max(worst, float(np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-3), initial=0.0)))
    print("%s: largest relative error %.3e" % (note, worst))
    return worst


def _random_batch(seed, N, nrefs, groups=None, max_len=15):
    rng = np.random.RandomState(seed)
    cands, refs = [], []
    for i in range(N):
        rs = [VOCAB[rng.randint(0, len(VOCAB), size=rng.randint(0 if j else 1, max_len + 1))].tolist() for j in range(nrefs[i % len(nrefs)])]
        base = rs[0]
        c = [int(VOCAB[rng.randint(len(VOCAB))]) if rng.rand() < 0.15 else t for t in (base * 3)[:rng.randint(1, max_len + 1)]]
        cands.append(c)
        refs.append(rs)
    return cm.pack_captions(cands, refs, groups=groups)


def test_device_matches_the_reference_vectors(ops, vec):
    batch = cm.CaptionBatch(*(vec[k] for k in cm.CaptionBatch.FIELDS))
    got = _np(cm.score(_to_device(batch), backend="device"))
    assert got["CIDER"][0] == 0.0                                            # the group of one record
    _compare(got, vec, "fixture")


def test_the_kernels_through_their_ops_wrappers(ops, vec):
    """ops.caption_metrics / ops.caption_cider called directly: shapes, dtypes and the statistics of the fixture."""
    t = [torch.from_numpy(vec[k]).cuda() for k in cm.CaptionBatch.FIELDS]
    stats, bleu, rouge = ops.caption_metrics(*t[:5])
    assert stats.shape == (67, 12) and bleu.shape == (4, 67) and rouge.shape == (67,) and bleu.dtype == torch.float64
    assert (stats.cpu().numpy() == vec["stats"]).all()
    grams, df, df_off, group_n = cm.cider_gram_tables(t)
    assert grams.shape[0] == 4 and grams.shape[1] == 67 + vec["refs"].shape[0] and df_off[0] == 0 and int(df.max()) <= 41
    cider = ops.caption_cider(grams, torch.cat([t[1], t[3]]), t[4], df, df_off, group_n)
    np.testing.assert_allclose(cider.cpu().numpy(), vec["CIDER"], rtol=1e-9, atol=1e-12)
    strided = torch.zeros((67, 80), dtype=torch.int32, device="cuda")       # a row stride that is not the width, an odd base offset
    strided[:, 1:1 + t[0].shape[1]] = t[0]
    s2, b2, r2 = ops.caption_metrics(strided[:, 1:1 + t[0].shape[1]], *t[1:5])
    assert torch.equal(s2, stats) and torch.equal(b2, bleu) and torch.equal(r2, rouge)


@pytest.mark.parametrize("N,nrefs,groups", [(1, (1,), None), (2, (2,), None), (67, (1, 2, 9), None),
                                            (67, (2, 1, 9), [0, 1, 3, 30, 67]), (67, (9,), [0, 40, 67])])
def test_device_matches_the_host_path(ops, N, nrefs, groups):
    batch = _random_batch(100 + N + len(nrefs), N, nrefs, groups)
    for rouge in ("reference", "lcs"):
        want = cm.score(batch, rouge=rouge)
        got = _np(cm.score(_to_device(batch), backend="device", rouge=rouge))
        _compare(got, want, "N=%d refs=%s groups=%s rouge=%s" % (N, nrefs, groups, rouge))


def test_full_length_sentences_and_the_lcs_dp(ops):
    """64-token sentences on every lane, repeated words (long common subsequences), both ROUGE modes."""
    batch = _random_batch(7, 12, (1, 3), max_len=64)
    assert int(batch.cand_len.max()) > 48 and int(batch.ref_len.max()) > 48
    for rouge in ("reference", "lcs"):
        _compare(_np(cm.score(_to_device(batch), backend="device", rouge=rouge)), cm.score(batch, rouge=rouge), "long " + rouge)


def test_the_same_call_twice_is_bit_identical(ops, vec):
    batch = _to_device(cm.CaptionBatch(*(vec[k] for k in cm.CaptionBatch.FIELDS)))
    a, b = cm.score(batch, backend="device"), cm.score(batch, backend="device")
    for k in ("stats", "BLEU", "ROUGE", "CIDER"):
        assert torch.equal(a[k], b[k]), k
    assert (a["BLEU_corpus"] == b["BLEU_corpus"]).all() and a["CIDER_mean"] == b["CIDER_mean"]


def test_no_records_give_empty_results(ops):
    res = cm.score(cm.pack_captions([], [], device="cuda"), backend="device")
    assert res["stats"].shape == (0, 12) and res["BLEU"].shape == (4, 0) and res["ROUGE"].shape == (0,) and res["CIDER"].shape == (0,)
    empty = torch.zeros((0, 1), dtype=torch.int32, device="cuda")
    none = torch.zeros((0,), dtype=torch.int32, device="cuda")
    stats, bleu, rouge = ops.caption_metrics(empty, none, empty, none, torch.zeros((1,), dtype=torch.int32, device="cuda"))
    assert stats.shape == (0, 12) and bleu.shape == (4, 0) and rouge.shape == (0,)
    host = cm.score(cm.pack_captions([], []))
    assert host["BLEU"].shape == (4, 0) and host["stats"].shape == (0, 12)


def test_the_evaluator_end_to_end_on_the_device(ops):
    """score_captions(backend="device") and evaluate() on synthetic records: the host backend's dictionary."""
    from image_captioning_amd.score_dense_captions import DenseCaptioningEvaluator
    rng = np.random.RandomState(5)
    words = "a the red blue car tree on road tall man".split()

    def phrase():
        return " ".join(words[i] for i in rng.randint(0, len(words), size=rng.randint(2, 8)))

    records = []
    for _ in range(4):
        image = []
        for _ in range(rng.randint(3, 12)):
            refs = [[phrase()] for _ in range(rng.randint(0, 4))]
            cand = refs[0][0] + " car" if refs and rng.rand() < 0.5 else phrase()
            image.append({"ok": int(rng.randint(0, 2)), "ov": float(rng.uniform(0.2, 0.9)), "candidate": cand, "references": refs})
        records.append(image)

    class Evaluator(DenseCaptioningEvaluator):
        def get_gt_captions(self, image_ids):
            return [None] * 4, [np.zeros((6, 4))] * 4, None

        def get_generated_captions(self, num_images, images):
            return None, None, None

        def assign_detections_to_ground_truth(self, *args):
            return records

    class Dataset:
        num_images, _image_ids = 4, [0, 1, 2, 3]

    ev = Evaluator(None, None, "CIDER", Dataset(), None, None, None, "t")
    n = sum(len(image) for image in records)
    for method in ("BLEU", "ROUGE", "CIDER"):
        host, dev = ev.score_captions(records, method), ev.score_captions(records, method, backend="device")
        assert dev.shape == host.shape == ((4, n) if method == "BLEU" else (n,)) and (np.isnan(dev) == np.isnan(host)).all()
        np.testing.assert_allclose(dev, host, rtol=1e-9, atol=1e-12, equal_nan=True)
        away = np.abs(host[..., None] - np.array([0.05, 0.1, 0.15, 0.2, 0.25]))
        assert np.nanmin(away) > 1e-6                                        # no score sits on a threshold: the sweeps must agree exactly
        a, b = ev.evaluate(method, backend="host"), ev.evaluate(method, backend="device")
        assert a["ap_breakdown"] == b["ap_breakdown"] and a["det_breakdown"] == b["det_breakdown"] and a["map"] == b["map"] and a["detmap"] == b["detmap"]
        assert a["detmap"] > 0
