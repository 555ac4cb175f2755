"""dc_refine_detections_f32 through ops.refine_detections on the device (-m gpu): all seven outputs, tails included, equal the
reference's recorded vectors (tests/golden/maskrcnn_reference.npz) and, on every case of tests/_refine_det_ref.py's table, the NumPy
restatement of the contract -- exactly (np.array_equal; scores by their bits).  Every table case is decided (tests/test_refine_det_ref.py
holds that on the CPU with a cap of 0): the one thing that separates the device's float64 exp from np.exp cannot move these results.
The table: N = 1, 2, 63, 64, 65, 200, 1000, 1025 and the limit (a thread owns two RoIs, the rank loop makes a second pass), B = 1 and 3
with a window and an image shape per image, C = 2 and 81, all background, one class, twins of two classes, tied scores, a confidence
floor of 0 and 0.7 with a score exactly at it, max_instances 3 and 100 below the number of survivors, boxes the unmolding empties,
boxes outside the window and with negative extent, zero-padded proposals, an IoU between the float64 and the float32 threshold."""
import os

import numpy as np
import pytest
import torch

import _refine_det_ref as RD

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maskrcnn_reference.npz")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def upload(case, dev):
    return dict(rois=torch.tensor(case["rois"], device=dev), class_ids=torch.tensor(case["class_ids"], device=dev),
                scores=torch.tensor(case["scores"], device=dev), deltas=torch.tensor(case["deltas"], device=dev),
                image_consts=torch.tensor(case["consts"], device=dev), std=case["std"], min_confidence=case["min_confidence"],
                threshold=case["threshold"], max_instances=case["max_instances"], image_hw=case["hw"])


def run(case, dev):
    from image_captioning_amd import ops
    out = ops.refine_detections(**upload(case, dev))
    return {k: t.cpu().numpy() for k, t in zip(RD.OUTPUTS, out)}


def explain(got, want):
    return "; ".join("%s differs in %d places" % (k, int((got[k].view(np.int32) != want[k].view(np.int32)).sum()))
                     for k in RD.OUTPUTS if not np.array_equal(got[k].view(np.int32), want[k].view(np.int32)))


@pytest.mark.parametrize("tag", ["conf", "all"])
def test_the_golden_vectors_give_the_references_detections(gpu, tag):
    with np.load(GOLDEN) as z:
        golden = {k: z[k] for k in z.files}
    case, det, final_boxes, final_ids, final_scores = RD.golden_case(golden, tag)
    got = run(case, gpu)
    n = int(got["count"][0])
    from image_captioning_amd import dense_model
    _, ok = dense_model.unmold_generations(det[:, :4].astype(np.int32), case["image_shapes"][0], case["windows"][0])
    assert n == len(final_boxes) == int(ok.sum())
    assert np.array_equal(got["boxes"][0, :n].astype(np.float64), det[ok, :4]) and np.array_equal(got["class_ids"][0, :n].astype(np.float64), det[ok, 4])
    assert np.array_equal(got["scores"][0, :n].astype(np.float64), det[ok, 5])
    assert np.array_equal(got["rois"][0, :n], final_boxes) and np.array_equal(got["class_ids"][0, :n], final_ids)
    assert np.array_equal(got["scores"][0, :n], final_scores)
    want = RD.refine(case)
    assert RD.same(got, want), explain(got, want)                        # the normalised boxes, the kept indices and the tails as well


@pytest.mark.parametrize("name", sorted(RD.cases()))
def test_the_table_cases_equal_the_restatement(gpu, name):
    from image_captioning_amd import _lib
    assert RD.LIMIT == _lib.REFINE_DET_MAX_ROIS
    case = RD.cases()[name]
    got, want = run(case, gpu), RD.refine(case)
    print("%s: counts %s" % (name, got["count"].tolist()))
    assert all(got[k].dtype == want[k].dtype and got[k].shape == want[k].shape for k in RD.OUTPUTS)
    assert RD.same(got, want), explain(got, want)


def test_the_limit_plus_one_is_refused_and_nothing_is_launched(gpu):
    from image_captioning_amd import _lib, ops
    N = _lib.REFINE_DET_MAX_ROIS + 1
    case = RD.make_case("over", 1, N, 2)
    with pytest.raises(_lib.DcapError, match="N = %d exceeds the limit of %d" % (N, _lib.REFINE_DET_MAX_ROIS)):
        ops.refine_detections(**upload(case, gpu))
    out = ops.refine_detections(**dict(upload(case, gpu), rois=torch.zeros(0, 5, 4, device=gpu), class_ids=torch.zeros(0, 5, dtype=torch.int32, device=gpu),
                                       scores=torch.zeros(0, 5, device=gpu), deltas=torch.zeros(0, 5, 4, device=gpu),
                                       image_consts=torch.zeros(0, _lib.REFINE_CONSTS, dtype=torch.float64, device=gpu)))
    assert [tuple(t.shape) for t in out] == [(0,), (0, 100, 4), (0, 100, 4), (0, 100, 4), (0, 100), (0, 100), (0, 100)]


def test_two_calls_and_a_graph_replay_on_another_stream_give_identical_bits(gpu):
    from image_captioning_amd import ops
    case = RD.cases()["n1000-b3-conf"]
    args = upload(case, gpu)
    first = [t.cpu().numpy() for t in ops.refine_detections(**args)]
    second = [t.cpu().numpy() for t in ops.refine_detections(**args)]
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(first, second))
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with ops.no_gc_during_capture(), torch.cuda.graph(g, stream=side):
        assert torch.cuda.current_stream() == side and torch.cuda.current_stream() != torch.cuda.default_stream()
        out = ops.refine_detections(**args)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(a.view(np.int32), t.cpu().numpy().view(np.int32)) for a, t in zip(first, out))
        for t in out:
            t.fill_(7)                                                   # the next replay writes every word again, tails included
