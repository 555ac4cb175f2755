"""The restatement of dc_refine_detections_f32's contract (tests/_refine_det_ref.py) on the CPU (no GPU): it equals the host path --
mask_rcnn_model.refine_detections + unmold_boxes -- exactly on the reference's recorded vectors and on every table case whose scores
are pairwise distinct; every table case is decided (an exp one ulp off either way changes nothing: none may be skipped); each planted
error moves the result; and the refusals of ops.refine_detections and of detect(refine=...) come before the library is loaded."""
import os

import numpy as np
import pytest
import torch

import _refine_det_ref as RD

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maskrcnn_reference.npz")
MAX_UNDECIDED = 0


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag", ["conf", "all"])
def test_the_restatement_equals_the_host_path_and_the_reference_on_the_golden_vectors(golden, tag):
    case, det, final_boxes, final_ids, final_scores = RD.golden_case(golden, tag)
    got = RD.refine(case)
    assert RD.same(got, RD.host_path(case))
    n = int(got["count"][0])
    assert n == len(final_boxes) and n < len(det)                        # (the vectors hold a box that the unmolding empties)
    assert np.array_equal(got["rois"][0, :n], final_boxes) and np.array_equal(got["class_ids"][0, :n], final_ids)
    assert np.array_equal(got["scores"][0, :n], final_scores)
    from image_captioning_amd import dense_model
    _, ok = dense_model.unmold_generations(det[:, :4].astype(np.int32), case["image_shapes"][0], case["windows"][0])
    assert np.array_equal(got["boxes"][0, :n].astype(np.float64), det[ok, :4]) and np.array_equal(got["scores"][0, :n].astype(np.float64), det[ok, 5])
    assert (got["keep"][0, n:] == -1).all() and (got["class_ids"][0, n:] == -1).all() and not got["boxes"][0, n:].any()
    assert RD.decided(case)


def test_the_table_holds_the_cases_it_promises():
    T = RD.cases()
    sizes = {c["rois"].shape[1] for c in T.values()}
    assert {1, 63, 64, 65, 1000, 1025, RD.LIMIT} <= sizes
    assert {c["rois"].shape[0] for c in T.values()} == {1, 3}
    assert {int(c["class_ids"].max()) + 1 for c in T.values()} >= {2, 81}
    assert {c["min_confidence"] for c in T.values()} == {0.0, 0.7} and {c["max_instances"] for c in T.values()} == {3, 100}
    out = {k: RD.refine(c) for k, c in T.items()}
    assert out["n1"]["count"].tolist() == [1]
    assert out["n2-iou-between-thresholds"]["count"].tolist() == [2]     # float32 IoU == (float) 0.3: nothing is suppressed
    assert out["n65-all-background"]["count"].tolist() == [0] and (out["n65-all-background"]["keep"] == -1).all()
    assert (out["n64-single-class"]["class_ids"][0, :out["n64-single-class"]["count"][0]] == 1).all()
    tw = out["n64-twins"]
    assert tw["keep"][0, :2].tolist() == [0, 1] and np.array_equal(tw["boxes"][0, 0], tw["boxes"][0, 1])     # both classes' copies survive
    assert 2 not in tw["keep"][0] and 3 not in tw["keep"][0]
    assert not RD.distinct_scores(T["n65-ties"]) and not RD.distinct_scores(T["limit-ties-c81"])
    fl = out["n65-floor-0.7"]
    assert 0 in fl["keep"][0] and 1 not in fl["keep"][0]                  # a score of (float32) 0.7 passes the floor, the next below does not
    assert out["n63-m3-more-survivors"]["count"].tolist() == [3] and out["n1025-c81"]["count"].tolist() == [100]
    assert out["limit-c2"]["count"][0] >= 20
    # the edge rows of n200-edges-b3: candidates among them, none of them in the output where the box is empty
    e, eo = T["n200-edges-b3"], out["n200-edges-b3"]
    for b in range(3):
        boxes = RD.refined_boxes(e["rois"][b], e["deltas"][b], e["consts"][b][:4], e["std"], e["hw"], np.exp)
        cand = e["class_ids"][b] > 0
        flat = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) <= 0) & cand
        assert flat[100:].sum() >= 20 and not np.isin(np.nonzero(flat)[0], eo["keep"][b]).any()
        assert (boxes[cand, 2] < boxes[cand, 0]).any() or (boxes[cand, 3] < boxes[cand, 1]).any()            # inverted boxes exist
    n = eo["count"]
    assert (n >= 5).all() and len({tuple(e["consts"][b]) for b in range(3)}) == 3
    # a box the unmolding empties although it has area in the molded image (scale < 1 in image 2)
    one = RD.refine_image(e["rois"][2], e["class_ids"][2], e["scores"][2], e["deltas"][2], e["consts"][2], e["std"], 0.0, 2.0, 200, e["hw"])
    two = RD.refined_boxes(e["rois"][2], e["deltas"][2], e["consts"][2][:4], e["std"], e["hw"], np.exp)
    area = ((two[:, 2] - two[:, 0]) * (two[:, 3] - two[:, 1]) > 0) & (e["class_ids"][2] > 0)
    assert one["count"] < area.sum()


@pytest.mark.parametrize("name", sorted(RD.cases()))
def test_the_restatement_equals_the_host_path_where_the_scores_are_distinct(name):
    case = RD.cases()[name]
    if not RD.distinct_scores(case):
        assert "ties" in name                                            # the host path's default sort promises no order: nothing to hold
        return
    assert RD.same(RD.refine(case), RD.host_path(case))


def test_every_table_case_is_decided():
    undecided = [k for k, c in RD.cases().items() if not RD.decided(c)]
    print("undecided table cases: %r" % (undecided,))
    assert len(undecided) <= MAX_UNDECIDED


@pytest.mark.parametrize("plant", RD.PLANTS)
def test_a_planted_error_is_seen(plant):
    T = RD.cases()
    moved = [k for k, c in T.items() if not RD.same(RD.refine(c), RD.refine(c, plant=plant))]
    print("%s moves %r" % (plant, moved))
    assert moved
    if plant in ("cross_class", "no_conf"):                              # and the host path sees it too where it is defined
        k = [k for k in moved if RD.distinct_scores(T[k])][0]
        assert not RD.same(RD.host_path(T[k]), RD.refine(T[k], plant=plant))


# ---- refusals (everything here is refused before the library is loaded) ----------------------------------------------------------------
def _no_library(monkeypatch):
    from image_captioning_amd import _lib

    def boom():
        raise AssertionError("the wrapper loaded the library before refusing")
    monkeypatch.setattr(_lib, "load", boom)
    return _lib.DcapError


def _good(B=2, N=5):
    from image_captioning_amd import _lib
    return dict(rois=torch.zeros(B, N, 4), class_ids=torch.zeros(B, N, dtype=torch.int32), scores=torch.zeros(B, N), deltas=torch.zeros(B, N, 4),
                image_consts=torch.zeros(B, _lib.REFINE_CONSTS, dtype=torch.float64), std=RD.STD, min_confidence=0.7, threshold=0.3,
                max_instances=100, image_hw=(256, 256))


def test_refine_detections_refusals(monkeypatch):
    from image_captioning_amd import _lib, ops
    E = _no_library(monkeypatch)
    B, N = 2, 5
    for key, bad, what in (("rois", torch.zeros(B, N, 5), "rois must be a float32 \\[B,N,4\\]"), ("rois", torch.zeros(B * N, 4), "rois must be"),
                           ("rois", torch.zeros(B, N, 4).double(), "rois must be torch.float32"),
                           ("rois", torch.zeros(B, N, 8)[:, :, ::2], "rois must be a contiguous"),
                           ("class_ids", torch.zeros(B, N, dtype=torch.int64), "class_ids must be torch.int32"),
                           ("class_ids", torch.zeros(B * N, dtype=torch.int32), "class_ids must be a contiguous"),
                           ("scores", torch.zeros(B, N).double(), "scores must be torch.float32"),
                           ("scores", torch.zeros(N, B).t(), "scores must be a contiguous"),
                           ("deltas", torch.zeros(B, N, 4).half(), "deltas must be torch.float32"),
                           ("deltas", torch.zeros(B, N + 1, 4), "deltas must be a contiguous"),
                           ("image_consts", torch.zeros(B, _lib.REFINE_CONSTS), "image_consts must be torch.float64"),
                           ("image_consts", torch.zeros(B, _lib.REFINE_CONSTS + 1, dtype=torch.float64), "image_consts must be a contiguous"),
                           ("max_instances", 0, "max_instances must be a positive integer"), ("max_instances", 2.5, "max_instances must be"),
                           ("max_instances", True, "max_instances must be"), ("std", (0.1, 0.2), "std must hold four"),
                           ("image_hw", (256,), "image_hw two")):
        with pytest.raises(E, match=what):
            ops.refine_detections(**dict(_good(B, N), **{key: bad}))
    over = _good(1, _lib.REFINE_DET_MAX_ROIS + 1)
    with pytest.raises(E, match="N = %d exceeds the limit of %d" % (_lib.REFINE_DET_MAX_ROIS + 1, _lib.REFINE_DET_MAX_ROIS)):
        ops.refine_detections(**over)
    assert 1024 <= _lib.REFINE_DET_MAX_ROIS == RD.LIMIT
    with pytest.raises(E, match="refine_detections: rois must live on the GPU"):                 # after the shape checks, before the library
        ops.refine_detections(**_good())


def test_detect_refuses_an_unknown_refine_by_name():
    from image_captioning_amd.mask_rcnn_model import MaskRCNN, MaskRCNNConfig
    stub = object.__new__(MaskRCNN)                                      # the refusal reads no model state
    stub.config = MaskRCNNConfig(9)
    with pytest.raises(ValueError, match="refine must be 'host' or 'device', got 'gpu'"):
        stub.detect([], refine="gpu")
    with pytest.raises(ValueError, match="device_masks"):                # the earlier refusals keep their place
        stub.detect([], device_masks=True, refine="device")


def test_detection_constants_is_the_row_the_kernel_reads():
    from image_captioning_amd import _lib
    from image_captioning_amd.mask_rcnn_model import MaskRCNNConfig, detection_constants
    cfg = MaskRCNNConfig(9)
    window, shape = (43, 0, 213, 256), (100, 150, 3)
    row = detection_constants(window, cfg, shape)
    assert row.dtype == np.float64 and row.shape == (_lib.REFINE_CONSTS,)
    want = RD.consts_row(window, cfg.IMAGE_SHAPE[:2], shape)
    assert np.array_equal(row[:4], want[:4]) and np.array_equal(row[6:9], want[6:9])
