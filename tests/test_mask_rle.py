"""COCO run-length masks on the host (no GPU): mask_rle's encode / decode / area / string form, the refusals of decode and from_string,
detect's two new refusals and ops.mask_rle's refusals on CPU tensors (checked before the library is loaded).

pycocotools is not a dependency, so the string form is pinned by vectors derived by hand from its rleToString:
  [5]        5 = 00101: no more groups                                   -> chr(5 + 48)                    "5"
  [3,2,4]    three single groups                                         -> "324"
  [3,2,4,2]  the fourth count goes out as 2 - counts[1] = 0              -> "3240"
  [40]       40 = 1|01000: low group 8 with the more bit, 8 + 32 + 48 = 88 "X"; then 1                     "X1"
  [16]       16 = 10000: bit 0x10 is set and what is left (0) is not -1, so one more group: 16 + 32 + 48 = 96 "`"; then 0   "`0"
  [3,5,4,2]  the fourth is 2 - 5 = -3 = ...11101: group 29, what is left is -1 and bit 0x10 is set: done, 29 + 48 = 77       "354M"
"""
import numpy as np
import pytest
import torch

from image_captioning_amd import mask_rle as R

VECTORS = (([5], "5"), ([3, 2, 4], "324"), ([3, 2, 4, 2], "3240"), ([40], "X1"), ([16], "`0"), ([3, 5, 4, 2], "354M"))


def _by_definition(mask):
    """The counts from the definition, pixel by pixel: column-major runs, starting with a run of zeros."""
    H, W = mask.shape
    counts, cur, run = [], 0, 0
    for x in range(W):
        for y in range(H):
            b = 1 if mask[y, x] else 0
            if b != cur:
                counts.append(run)
                cur, run = b, 0
            run += 1
    counts.append(run)
    return counts


def _masks():
    rng = np.random.RandomState(0)
    out = {"random_13x17": rng.rand(13, 17) < 0.5, "sparse_31x9": rng.rand(31, 9) < 0.1, "zeros": np.zeros((6, 5), bool), "ones": np.ones((6, 5), bool),
           "first_pixel": np.zeros((6, 5), bool), "last_pixel": np.zeros((6, 5), bool), "row_1xW": rng.rand(1, 23) < 0.5,
           "column_Hx1": rng.rand(23, 1) < 0.5, "uint8_values": (rng.rand(7, 8) < 0.5).astype(np.uint8) * 255}
    out["first_pixel"][0, 0] = True
    out["last_pixel"][-1, -1] = True
    return out


@pytest.mark.parametrize("name", sorted(_masks()))
def test_encode_is_the_definition_and_decode_inverts_it(name):
    mask = _masks()[name]
    rle = R.encode(mask)
    H, W = mask.shape
    assert rle["size"] == [H, W] and rle["counts"].dtype == np.uint32
    assert rle["counts"].tolist() == _by_definition(mask)
    assert int(rle["counts"].sum()) == H * W
    back = R.decode(rle)
    assert back.dtype == np.uint8 and back.shape == (H, W) and np.array_equal(back, (mask != 0).astype(np.uint8))
    assert R.area(rle) == int((mask != 0).sum())


def test_the_edges_of_the_rule():
    m = _masks()
    assert R.encode(m["zeros"])["counts"].tolist() == [30]
    assert R.encode(m["ones"])["counts"].tolist() == [0, 30]                 # T = 1 transition, T + 1 counts: the last run is of ones
    assert R.encode(m["first_pixel"])["counts"].tolist() == [0, 1, 29]
    assert R.encode(m["last_pixel"])["counts"].tolist() == [29, 1]          # no zero-length run of zeros is appended
    two = np.zeros((3, 2), bool)
    two[2, 0] = two[0, 1] = True                                             # a run crosses the column boundary: indices 2 and 3
    assert R.encode(two)["counts"].tolist() == [2, 2, 2]


def test_the_string_vectors():
    for counts, s in VECTORS:
        assert R.to_string(counts) == s, counts
        assert R.from_string(s).tolist() == counts and R.from_string(s).dtype == np.uint32
        assert R.from_string(s.encode()).tolist() == counts


def test_string_round_trips():
    rng = np.random.RandomState(1)
    cases = [[0, 5, 3], [1 << 20], [7, 1 << 20, 3, 2, 1 << 25, 1], [100, 3, 1, 900, 5, 2, 70000, 1, 1, 65536, 31, 32, 33, 15, 16, 17],
             [0, (1 << 31) - 1], rng.randint(0, 1 << 18, 200).tolist()]
    assert any(c[i] < c[i - 2] for c in cases for i in range(3, len(c)))     # negative differences from counts[i-2] are in there
    for c in cases:
        assert R.from_string(R.to_string(c)).tolist() == c
    for name, mask in _masks().items():
        coco = R.to_coco(R.encode(mask))
        assert coco["size"] == list(mask.shape) and isinstance(coco["counts"], str)
        assert np.array_equal(R.decode(coco), (mask != 0).astype(np.uint8)), name
        assert R.area(coco) == int((mask != 0).sum())


def test_inconsistent_input_is_refused_by_name():
    with pytest.raises(ValueError, match="counts sum to 29, the mask of size 6 x 5 has 30 pixels"):
        R.decode({"size": [6, 5], "counts": np.array([10, 19], np.uint32)})
    with pytest.raises(ValueError, match="counts sum to 31"):
        R.decode({"size": [6, 5], "counts": [31]})
    with pytest.raises(ValueError, match="non-empty list"):
        R.decode({"size": [6, 5], "counts": np.zeros((0,), np.uint32)})
    with pytest.raises(ValueError, match="counts sum to 40"):
        R.to_coco({"size": [6, 5], "counts": [40]})
    with pytest.raises(ValueError, match="truncated: it ends inside count 0"):
        R.from_string("X")                                                   # "X1" without its second group
    with pytest.raises(ValueError, match="truncated: it ends inside count 3"):
        R.from_string("324" + "`")
    with pytest.raises(ValueError, match="not part of an RLE string"):
        R.from_string("3 4")
    with pytest.raises(ValueError, match="no run length"):
        R.from_string("M")                                                   # -3 as a first count
    with pytest.raises(ValueError, match="bool or uint8"):
        R.encode(np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="bool or uint8"):
        R.encode(np.zeros((3,), bool))


# ---- detect's new refusals ----------------------------------------------------------------------------------------------------------
def test_detect_refuses_the_new_keyword_by_name():
    from image_captioning_amd.mask_rcnn_model import MaskRCNN, MaskRCNNConfig

    class Cfg(MaskRCNNConfig):
        IMAGES_PER_GPU = 1
        IMAGE_MIN_DIM = 128
        IMAGE_MAX_DIM = 128
    stub = object.__new__(MaskRCNN)                                          # the refusals read no model state but the configuration
    stub.config = Cfg(9)
    with pytest.raises(ValueError, match="mask_format must be 'dense' or 'rle', got 'coco'"):
        stub.detect([], mask_format="coco")
    with pytest.raises(ValueError, match="mask_format='rle'.*device_masks=True is not available"):
        stub.detect([], postprocess="device", device_masks=True, mask_format="rle")
    with pytest.raises(ValueError, match="device_masks=True needs postprocess='device'"):      # the older check still comes first
        stub.detect([], device_masks=True, mask_format="rle")


# ---- ops.mask_rle's refusals (everything here is refused before the library is loaded) ----------------------------------------------
def _no_library(monkeypatch):
    from image_captioning_amd import _lib

    def boom():
        raise AssertionError("the wrapper loaded the library before refusing")
    monkeypatch.setattr(_lib, "load", boom)
    return _lib.DcapError


def test_mask_rle_refusals(monkeypatch):
    from image_captioning_amd import ops
    E = _no_library(monkeypatch)
    m, b = torch.zeros(3, 28, 28), torch.zeros(3, 4, dtype=torch.int32)
    for bad_m, bad_b, H, W, what in ((torch.zeros(3, 65, 28), b, 97, 131, "h, w in 1..64"), (torch.zeros(28, 28), b, 97, 131, "masks must be"),
                                     (m, b, 0, 131, "at least 1 x 1"), (m, b, 1 << 16, 1 << 15, "below 2\\^31"),
                                     (m, b, 1 << 15, 1 << 15, "M \\* \\(H \\* W \\+ 1\\) below 2\\^31"),
                                     (m.double(), b, 97, 131, "masks must be torch.float32"), (m, b.long(), 97, 131, "boxes must be torch.int32"),
                                     (m, torch.zeros(2, 4, dtype=torch.int32), 97, 131, "boxes must be a contiguous"),
                                     (torch.zeros(3, 28, 56)[:, :, ::2], b, 97, 131, "masks must be a contiguous")):
        with pytest.raises(E, match=what):
            ops.mask_rle(bad_m, bad_b, H, W)
    for capacity in (-1, 2.5, True, 1 << 31):
        with pytest.raises(E, match="capacity must be an integer"):
            ops.mask_rle(m, b, 97, 131, capacity=capacity)
    with pytest.raises(E, match="mask_rle: masks must live on the GPU"):
        ops.mask_rle(m, b, 97, 131)
    with pytest.raises(E, match="mask_rle: masks must live on the GPU"):
        ops.mask_rle(m, b, 97, 131, capacity=0)


def test_the_default_capacity_grows_with_the_detections_and_the_width():
    from image_captioning_amd import ops
    assert ops.mask_rle_capacity(0, 97, 131) == 4096 and ops.mask_rle_capacity(100, 768, 1024) == 102400
