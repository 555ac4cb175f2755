"""ops.rle_iou / ops.box_iou / ops.detection_ap (csrc/detect_eval.hip) and MaskRCNN.evaluate on the device (-m gpu).  Every comparison
is an equality of bits: the oracles are mask_rle.iou, utils.compute_overlaps and detection_eval.ap_from_overlaps on the host.

rle_iou: 70 x 45 masks (H no multiple of 64): the planes of test_mask_rle_iou.py -- empty, full, pixel (0, 0) set, one pixel, a
checkerboard patch -- and dotted masks of 100 and 150 one-pixel runs, which the lanes walk in two and three passes of 64 runs of ones;
a disjoint and an identical pair; 3 x 5, 1 x 1, 130 x 67, 0 x 4 and 4 x 0; an n_det below D; crowd flags; a capacity one word short;
counts that do not sum to H W; the refusals of the header.
detection_ap: D in {0, 1, 63, 64, 65, 130} x G in {0, 1, 64, 65, 100}, three images of different counts a launch, the ten default
thresholds; scores, IoUs and classes are drawn from small sets, so score ties, IoU ties and IoUs equal to a threshold are everywhere; a
NaN row.
evaluate: the smallest synthetic MaskRCNN of test_gpu_maskrcnn_model.py, two images of different sizes with ground truth taken from a
first detect call and perturbed, and one image without ground truth."""
import ctypes as C

import numpy as np
import pytest
import torch

from _detect_device import dev
from test_mask_rle_iou import H, W, planes

pytestmark = pytest.mark.gpu
GUARD = 1024


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def dotted(n, step, start=2):
    """n one-pixel runs of ones at column-major indices start, start + step, ..."""
    flat = np.zeros(H * W, np.uint8)
    flat[start + step * np.arange(n)] = 1
    return flat.reshape(W, H).T.copy()


_MASKS = {}


def masks():
    """name -> uint8 [H,W]: built once, never changed."""
    if not _MASKS:
        _MASKS.update(planes())
        _MASKS["dots100"] = dotted(100, 7)
        _MASKS["dots150"] = dotted(150, 5, start=1)
        yy, xx = np.mgrid[0:H, 0:W]
        _MASKS["left"], _MASKS["right"] = (xx < 10).astype(np.uint8), (xx > 30).astype(np.uint8)       # a disjoint pair
        rng = np.random.RandomState(23)
        for i in range(130):
            cy, cx, r = rng.randint(0, H), rng.randint(0, W), rng.randint(2, 14)
            _MASKS["disc%d" % i] = (np.hypot(yy - cy, xx - cx) < r).astype(np.uint8)
    return _MASKS


def pack(rles):
    """A list of encodings as ops.mask_rle packs them: (offsets int32 [n+1], counts int32 of uint32 bits) on the host."""
    lengths = [len(r["counts"]) for r in rles]
    counts = np.concatenate([r["counts"] for r in rles]).astype(np.uint32) if rles else np.zeros(0, np.uint32)
    return np.cumsum([0] + lengths).astype(np.int32), counts.view(np.int32)


def encoded(names):
    from image_captioning_amd import mask_rle
    return [mask_rle.encode(masks()[k]) for k in names]


SETS = {
    "3x5": (["board", "dots150", "corner"], ["dots100", "board", "blob0", "full", "dots150"]),
    "1x1": (["corner"], ["full"]),
    "130x67": (["disc%d" % i for i in range(120)] + ["empty", "full", "corner", "pixel", "board", "dots100", "dots150", "left", "right", "last"],
               ["disc%d" % i for i in range(60, 120)] + ["right", "left", "pixel", "empty", "dots150", "board", "full"]),
    "0x4": ([], ["blob0", "blob1", "empty", "full"]),
    "4x0": (["blob0", "blob1", "empty", "full"], []),
}
_ORACLE = {}


def oracle(name, crowd=None):
    """(dt, gt encodings, mask_rle.iou's matrix, the intersections, the areas): computed once per case."""
    key = (name, None if crowd is None else tuple(crowd))
    if key not in _ORACLE:
        from image_captioning_amd import mask_rle
        dt, gt = encoded(SETS[name][0]), encoded(SETS[name][1])
        area = np.array([mask_rle.area(r) for r in dt + gt], np.int32)
        inter = np.array([[mask_rle._intersection([int(v) for v in a["counts"]], [int(v) for v in b["counts"]]) for b in gt] for a in dt],
                         np.int32).reshape(len(dt), len(gt))
        _ORACLE[key] = (dt, gt, mask_rle.iou(dt, gt, crowd), inter, area)
    return _ORACLE[key]


def run_rle_iou(ops, dt, gt, **kw):
    (od, cd), (og, cg) = pack(dt), pack(gt)
    iou, inter, area, status = ops.rle_iou(dev(od, torch.int32), dev(cd, torch.int32), dev(og, torch.int32), dev(cg, torch.int32), H, W, **kw)
    torch.cuda.synchronize()
    return iou.cpu().numpy(), inter.cpu().numpy(), area.cpu().numpy(), status.cpu().numpy()


def test_the_masks_hold_what_they_claim():
    m = masks()
    enc = {k: r for k, r in zip(m, encoded(list(m)))}
    assert len(enc["dots100"]["counts"]) == 201 and len(enc["dots150"]["counts"]) == 301      # 100 and 150 runs of ones: two and three passes
    assert len(enc["board"]["counts"]) > 301                                                    # longer than both: they are the walked side
    assert enc["corner"]["counts"][0] == 0 and enc["full"]["counts"].tolist() == [0, H * W] and enc["empty"]["counts"].tolist() == [H * W]
    assert len(enc["pixel"]["counts"]) == 3 and not (m["left"] & m["right"]).any() and H % 64
    _, _, want, inter, _ = oracle("3x5")
    assert want[0, 1] == 1.0 and inter[0, 0] > 0 and inter[1, 0] > 0 and want[1, 4] == 1.0 and inter[1, 4] == 150   # (board: identical pair)


@pytest.mark.parametrize("name", sorted(SETS))
def test_rle_iou_equals_the_host_bit_for_bit(ops, name):
    dt, gt, want, inter_w, area_w = oracle(name)
    iou, inter, area, status = run_rle_iou(ops, dt, gt)
    D, G = len(dt), len(gt)
    assert iou.shape == (D, G) and iou.dtype == np.float64 and inter.shape == (D, G) and area.shape == (D + G,)
    assert status.tolist() == [0, 0, 0, D]
    assert np.array_equal(_bits(iou), _bits(want)), np.argwhere(_bits(iou) != _bits(want))[:5]
    if D and G:
        assert np.array_equal(inter, inter_w) and np.array_equal(area, area_w)
        assert 0 < np.count_nonzero(want) and (name == "1x1" or np.count_nonzero(want) < want.size)
    else:
        assert (area == -1).all()
    if name == "3x5":                                                                           # the intersections against the dense planes
        m = masks()
        for i, a in enumerate(SETS[name][0]):
            for j, b in enumerate(SETS[name][1]):
                assert inter[i, j] == int((m[a] & m[b]).sum()), (a, b)


def test_rle_iou_n_det_below_d_and_crowd_flags(ops):
    crowd = [0, 1, 0, 1, 1]
    dt, gt, want, inter_w, _ = oracle("3x5", crowd)
    assert not np.array_equal(want, oracle("3x5")[2])                                           # the flags change something
    iou, inter, _, status = run_rle_iou(ops, dt, gt, iscrowd=dev(crowd, torch.uint8))
    assert np.array_equal(_bits(iou), _bits(want)) and status.tolist() == [0, 0, 0, 3]
    for n in (2, 0, 3, 7):
        iou, inter, area, status = run_rle_iou(ops, dt, gt, iscrowd=dev(crowd, torch.uint8), n_det=dev([n], torch.int32))
        cut = want.copy()
        cut[n:] = 0.0
        assert np.array_equal(_bits(iou), _bits(cut)) and (inter[n:] == 0).all() and np.array_equal(inter[:n], inter_w[:n]), n
        assert status.tolist() == [0, 0, 0, min(n, 3)] and (area >= 0).all()


def test_rle_iou_into_a_view_with_its_own_row_stride(ops):
    dt, gt, want, inter_w, _ = oracle("3x5")
    (od, cd), (og, cg) = pack(dt), pack(gt)
    big = torch.full((3, 9), 7.0, dtype=torch.float64, device="cuda")
    iou, inter, _, _ = ops.rle_iou(dev(od, torch.int32), dev(cd, torch.int32), dev(og, torch.int32), dev(cg, torch.int32), H, W, out=big[:, :5])
    host = big.cpu().numpy()
    assert np.array_equal(_bits(host[:, :5]), _bits(want)) and (host[:, 5:] == 7.0).all() and np.array_equal(inter.cpu().numpy(), inter_w)


def raw_rle_iou(dt, gt, cap_d=None, cap_g=None, workspace="exact", fill=0x5A5A5A5A, **over):
    """dc_rle_iou_f64 itself, on patterned buffers with guard words behind counts and the workspace.
    Returns (return code, iou, inter, area, status, counts_d's guard intact, the workspace's guard intact, bytes needed)."""
    from image_captioning_amd import _lib
    lib = _lib.load()
    (od, cd), (og, cg) = pack(dt), pack(gt)
    D, G = len(dt), len(gt)
    cap_d = len(cd) if cap_d is None else cap_d
    cap_g = len(cg) if cap_g is None else cap_g
    buf_d = torch.full((cap_d + GUARD,), fill, dtype=torch.int32, device="cuda")
    buf_g = torch.full((cap_g + GUARD,), fill, dtype=torch.int32, device="cuda")
    buf_d[:min(cap_d, len(cd))] = dev(cd[:cap_d], torch.int32)
    buf_g[:min(cap_g, len(cg))] = dev(cg[:cap_g], torch.int32)
    od_t, og_t = dev(od, torch.int32), dev(og, torch.int32)
    iou = torch.full((max(D * G, 1),), 5.0, dtype=torch.float64, device="cuda")
    inter = torch.full((max(D * G, 1),), 55, dtype=torch.int32, device="cuda")
    area = torch.full((D + G + 1,), 55, dtype=torch.int32, device="cuda")
    status = torch.full((4 + GUARD,), 55, dtype=torch.int32, device="cuda")
    d = _lib.RleIouDesc()
    d.D, d.G, d.H, d.W, d.capacity_d, d.capacity_g, d.ld = D, G, H, W, cap_d, cap_g, G
    d.offsets_d, d.counts_d, d.offsets_g, d.counts_g = od_t.data_ptr(), buf_d.data_ptr(), og_t.data_ptr(), buf_g.data_ptr()
    d.iou, d.inter, d.area, d.status = iou.data_ptr(), inter.data_ptr(), area.data_ptr(), status.data_ptr()
    for k, v in over.items():
        setattr(d, k, v)
    need = lib.dc_rle_iou_workspace_bytes(C.byref(d))
    ws = torch.full((need + 4 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    if workspace == "exact":
        d.workspace, d.workspace_bytes = ws.data_ptr(), need
    elif workspace == "short":
        d.workspace, d.workspace_bytes = ws.data_ptr(), need - 1
    elif workspace == "misaligned":
        d.workspace, d.workspace_bytes = ws.data_ptr() + 4, need + 64
    rc = lib.dc_rle_iou_f64(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert (st[4:] == 55).all(), "words behind status were written"
    return (rc, iou.cpu().numpy()[:D * G].reshape(D, G), inter.cpu().numpy()[:D * G].reshape(D, G), area.cpu().numpy(), st[:4],
            bool((buf_d[cap_d:] == fill).all()), bool((ws[need:] == 0xA5).all()), need)


def test_rle_iou_on_an_exact_workspace_and_a_capacity_one_word_short(ops):
    dt, gt, want, inter_w, area_w = oracle("3x5")
    total_d, total_g = (sum(len(r["counts"]) for r in s) for s in (dt, gt))
    rc, iou, inter, area, status, counts_ok, ws_ok, need = raw_rle_iou(dt, gt)
    assert rc == 0 and need == ((total_d + total_g) * 8 + 15) // 16 * 16 + (3 + 5) * 16
    assert np.array_equal(_bits(iou), _bits(want)) and np.array_equal(inter, inter_w) and np.array_equal(area[:-1], area_w) and area[-1] == 55
    assert status.tolist() == [0, 0, 0, 3] and counts_ok and ws_ok
    rc, iou, inter, area, status, counts_ok, ws_ok, _ = raw_rle_iou(dt, gt, cap_d=total_d - 1)
    assert rc == 0 and status.tolist() == [total_d, 0, 0, 3] and np.isnan(iou).all() and (inter == -1).all() and (area[:-1] == -1).all()
    assert counts_ok and ws_ok
    rc, iou, inter, area, status, counts_ok, ws_ok, _ = raw_rle_iou(dt, gt, cap_g=total_g - 1)
    assert rc == 0 and status.tolist() == [0, total_g, 0, 3] and np.isnan(iou).all() and (inter == -1).all() and counts_ok and ws_ok


def test_rle_iou_counts_that_do_not_sum_to_the_image(ops):
    from image_captioning_amd import mask_rle
    dt, gt, want, _, _ = oracle("3x5")
    bad_d = [dict(r, counts=r["counts"].copy()) for r in dt]
    bad_d[1]["counts"][3] += 1
    bad_g = [dict(r, counts=r["counts"].copy()) for r in gt]
    bad_g[2]["counts"][0] -= 1
    bad_g[4]["counts"][-1] += 2
    iou, inter, area, status = run_rle_iou(ops, bad_d, bad_g)
    assert status.tolist() == [0, 0, 3, 3]
    good = np.ones((3, 5), bool)
    good[1, :] = good[:, 2] = good[:, 4] = False
    assert np.isnan(iou[~good]).all() and (inter[~good] == -1).all() and np.array_equal(_bits(iou[good]), _bits(want[good]))
    assert area[[1, 3 + 2, 3 + 4]].tolist() == [-1, -1, -1] and area[0] == mask_rle.area(dt[0])


def test_rle_iou_two_calls_give_identical_bytes(ops):
    dt, gt, _, _, _ = oracle("130x67")
    a, b = run_rle_iou(ops, dt, gt), run_rle_iou(ops, dt, gt)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_rle_iou_refuses_what_the_header_says(ops):
    from image_captioning_amd import _lib
    dt, gt, _, _, _ = oracle("3x5")
    for mode in ("null", "short", "misaligned"):
        rc, iou, _, _, status, _, ws_ok, _ = raw_rle_iou(dt, gt, workspace=mode)
        assert rc == _lib.EWORKSPACE and (iou == 5.0).all() and (status == 55).all() and ws_ok, mode
    keep = torch.zeros((64,), dtype=torch.int32, device="cuda")
    for over in (dict(offsets_d=None), dict(offsets_g=None), dict(status=None), dict(iou=None), dict(counts_d=None), dict(counts_g=None),
                 dict(D=1025), dict(G=1025), dict(D=-1), dict(G=-1), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15), dict(capacity_d=-1),
                 dict(capacity_g=-1), dict(ld=4), dict(offsets_d=keep.data_ptr() + 2), dict(iou=keep.data_ptr() + 4),
                 dict(status=keep.data_ptr() + 1), dict(n_det=keep.data_ptr() + 2)):
        rc, iou, _, _, status, _, _, need = raw_rle_iou(dt, gt, **over)
        assert rc == _lib.EINVAL and need == 0 and (iou == 5.0).all() and (status == 55).all(), over


# ---- box_iou -------------------------------------------------------------------------------------------------------------------------
def test_box_iou_equals_compute_overlaps_bit_for_bit(ops):
    from image_captioning_amd import utils
    rng = np.random.RandomState(4)
    B, Dmax, Gmax = 3, 70, 33

    def boxes(n):
        y1, x1 = rng.randint(0, 600, n), rng.randint(0, 900, n)
        return np.stack([y1, x1, y1 + rng.randint(1, 200, n), x1 + rng.randint(1, 200, n)], 1).astype(np.int32)
    a, g = np.stack([boxes(Dmax) for _ in range(B)]), np.stack([boxes(Gmax) for _ in range(B)])
    a[0, :Gmax] = g[0]                                                           # identical boxes: IoU 1 on a diagonal
    a[1, 5:12] = g[1, 5:12] + np.array([0, 3, 0, 3], np.int32)                   # shifted copies
    a[1, 20], g[1, 20] = (10, 10, 20, 20), (20, 20, 30, 30)                      # touching: 0
    a[2, 60:] = 0                                                                # zero padding on both sides: 0 / 0 is NaN
    g[2, 30:] = 0
    got = ops.box_iou(dev(a, torch.int32), dev(g, torch.int32)).cpu().numpy()
    assert got.shape == (B, Dmax, Gmax) and got.dtype == np.float64
    for b in range(B):
        with np.errstate(divide="ignore", invalid="ignore"):
            want = utils.compute_overlaps(a[b], g[b])
        assert want.dtype == np.float64 and np.array_equal(np.isnan(got[b]), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(_bits(got[b][ok]), _bits(want[ok])), b
    assert (got[0, np.arange(Gmax), np.arange(Gmax)] == 1.0).all() and got[1, 20, 20] == 0.0 and np.isnan(got[2, 60:, 30:]).all()
    assert 0 < np.count_nonzero(np.nan_to_num(got)) < got.size
    wide = torch.full((B, Dmax, Gmax + 3), -2.0, dtype=torch.float64, device="cuda")                # a view with its own row stride
    with pytest.raises(ops._lib.DcapError, match="one behind the other"):
        ops.box_iou(dev(a, torch.int32), dev(g, torch.int32), out=wide[:1].expand(B, Dmax, Gmax + 3)[:, :, :Gmax])
    ops.box_iou(dev(a, torch.int32), dev(g, torch.int32), out=wide[:, :, :Gmax])
    host = wide.cpu().numpy()
    assert host[:, :, :Gmax].tobytes() == got.tobytes() and (host[:, :, Gmax:] == -2.0).all()
    assert ops.box_iou(dev(a[:, :0], torch.int32), dev(g, torch.int32)).shape == (B, 0, Gmax)


def test_box_iou_refuses_what_the_header_says(ops):
    from image_captioning_amd import _lib
    lib = _lib.load()
    a, g = torch.zeros((2, 8, 4), dtype=torch.int32, device="cuda"), torch.zeros((2, 4, 4), dtype=torch.int32, device="cuda")
    out = torch.full((2 * 8 * 4 + 2,), 3.0, dtype=torch.float64, device="cuda")

    def call(boxes=a.data_ptr(), gt=g.data_ptr(), B=2, Dmax=8, Gmax=4, ld=4, o=out.data_ptr()):
        return lib.dc_box_iou_f64(boxes, gt, B, Dmax, Gmax, ld, o, None)
    for over in (dict(boxes=None), dict(gt=None), dict(o=None), dict(B=-1), dict(B=65536), dict(Dmax=1025), dict(Gmax=1025), dict(Dmax=-1),
                 dict(ld=3), dict(boxes=a.data_ptr() + 4), dict(gt=g.data_ptr() + 8), dict(o=out.data_ptr() + 4)):
        assert call(**over) == _lib.EINVAL, over
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 3.0).all()
    assert call(B=0, boxes=None, gt=None, o=None) == 0 and call(Dmax=0, boxes=None) == 0


# ---- detection_ap --------------------------------------------------------------------------------------------------------------------
def ap_case(D, G, seed):
    """Three images in one launch: counts (D, G), (D - 1, G - 3) and (D // 2, G // 2), clipped at 0.  IoUs, scores and classes come from
    small sets -- ties and threshold-equal IoUs everywhere --, image 0 carries a NaN row."""
    from image_captioning_amd import detection_eval
    rng = np.random.RandomState(seed)
    thr = detection_eval.DEFAULT_THRESHOLDS
    values = np.concatenate([[0.0, 0.2, 0.45, 0.5, 0.55, 0.75, 1.0], thr[[2, 4, 7, 9]], np.nextafter(thr[[3, 6]], 0.0), rng.rand(6)])
    ov = values[rng.randint(0, len(values), (3, D, G))]
    ov[rng.rand(3, D, G) < 0.5] = 0.0                                            # (half the pairs do not overlap)
    if D > 5:
        ov[0, 5] = np.nan
    n_det = np.array([D, max(D - 1, 0), D // 2], np.int32)
    n_gt = np.array([G, max(G - 3, 0), G // 2], np.int32)
    scores = (rng.randint(0, max(D // 3, 2), (3, D)) / np.float32(max(D // 3, 2))).astype(np.float32)
    return ov, n_det, n_gt, rng.randint(1, 4, (3, D)).astype(np.int32), scores, rng.randint(1, 4, (3, G)).astype(np.int32), thr


@pytest.mark.parametrize("D", [0, 1, 63, 64, 65, 130])
def test_detection_ap_equals_the_host_bit_for_bit(ops, D):
    from image_captioning_amd import detection_eval
    matched = ties = 0
    for G in (0, 1, 64, 65, 100):
        ov, n_det, n_gt, pcls, psc, gcls, thr = ap_case(D, G, 100 * D + G)
        ap, pm, gm, od = ops.detection_ap(dev(ov, torch.float64), dev(n_det, torch.int32), dev(n_gt, torch.int32), dev(pcls, torch.int32), dev(psc),
                                          dev(gcls, torch.int32), dev(thr, torch.float64))
        ap, pm, gm, od = ap.cpu().numpy(), pm.cpu().numpy(), gm.cpu().numpy(), od.cpu().numpy()
        assert ap.shape == (3, 10) and pm.shape == (3, 10, D) and gm.shape == (3, 10, G) and od.shape == (3, D)
        for b in range(3):
            n, g = n_det[b], n_gt[b]
            w_ap, w_pm, w_gm, w_od = detection_eval.ap_from_overlaps(ov[b, :n, :g], gcls[b, :g], pcls[b, :n], psc[b, :n], thr)
            assert np.array_equal(od[b, :n], w_od) and (od[b, n:] == -1).all(), (G, b)
            assert np.array_equal(pm[b, :, :n], w_pm) and (pm[b, :, n:] == -1).all(), (G, b)
            assert np.array_equal(gm[b, :, :g], w_gm) and (gm[b, :, g:] == -1).all(), (G, b)
            assert np.array_equal(np.isnan(ap[b]), np.isnan(w_ap)) and np.isnan(w_ap).all() == (g == 0), (G, b)
            assert g == 0 or np.array_equal(_bits(ap[b]), _bits(w_ap)), (G, b, ap[b], w_ap)
            matched += int((w_pm >= 0).sum())
            ties += int(len(np.unique(psc[b, :n])) < n)
    if D >= 63:
        assert matched > 100 and ties >= 10                                      # (the cases match, and their scores tie)


def test_detection_ap_planted_rules(ops):
    """The rules of test_detection_eval_ref.py, on the device: score ties, IoU ties, an IoU equal to the threshold, a wrong-class best."""
    from image_captioning_amd import detection_eval
    thr = np.array([0.5, 0.75, np.nextafter(0.75, 1.0)])
    ov = np.zeros((4, 3, 3))
    ov[0, :, 0] = [0.9, 0.8, 0.7]                                                # equal scores on one ground truth
    ov[1, :2] = 0.6                                                              # equal IoUs
    ov[2, 0, 0], ov[2, 1, 1] = 0.5, 0.75                                         # IoUs equal to thresholds
    ov[3, 0] = [0.9, 0.6, 0.2]                                                   # the best IoU has the wrong class
    n_det, n_gt = np.array([3, 2, 2, 1], np.int32), np.array([1, 3, 2, 3], np.int32)
    pcls = np.ones((4, 3), np.int32)
    gcls = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 1], [2, 1, 1]], np.int32)
    psc = np.array([[0.5, 0.5, 0.9], [0.9, 0.8, 0], [0.9, 0.8, 0], [0.9, 0, 0]], np.float32)
    ap, pm, gm, od = (t.cpu().numpy() for t in ops.detection_ap(dev(ov, torch.float64), dev(n_det, torch.int32), dev(n_gt, torch.int32),
                                                                dev(pcls, torch.int32), dev(psc), dev(gcls, torch.int32), dev(thr, torch.float64)))
    assert od[0].tolist() == [2, 1, 0] and pm[0, 0].tolist() == [0, -1, -1] and gm[0, 0].tolist() == [0, -1, -1]
    assert pm[1, 0].tolist() == [2, 1, -1] and gm[1, 0].tolist() == [-1, 1, 0]
    assert pm[2, :, :2].tolist() == [[0, 1], [-1, 1], [-1, -1]] and ap[2].tolist() == [1.0, 0.25, 0.0]
    assert pm[3, :2, 0].tolist() == [1, -1]
    for b in range(4):
        w_ap, w_pm, w_gm, w_od = detection_eval.ap_from_overlaps(ov[b, :n_det[b], :n_gt[b]], gcls[b, :n_gt[b]], pcls[b, :n_det[b]],
                                                                 psc[b, :n_det[b]], thr)
        assert np.array_equal(_bits(ap[b]), _bits(w_ap)) and np.array_equal(pm[b, :, :n_det[b]], w_pm) and np.array_equal(gm[b, :, :n_gt[b]], w_gm)


def test_detection_ap_two_calls_give_identical_bytes_and_outputs_may_be_given(ops):
    ov, n_det, n_gt, pcls, psc, gcls, thr = ap_case(130, 100, 9)
    args = (dev(ov, torch.float64), dev(n_det, torch.int32), dev(n_gt, torch.int32), dev(pcls, torch.int32), dev(psc), dev(gcls, torch.int32),
            dev(thr, torch.float64))
    a = [t.cpu().numpy() for t in ops.detection_ap(*args)]
    given = dict(ap=torch.empty((3, 10), dtype=torch.float64, device="cuda"), pred_match=torch.empty((3, 10, 130), dtype=torch.int32, device="cuda"),
                 gt_match=torch.empty((3, 10, 100), dtype=torch.int32, device="cuda"), order=torch.empty((3, 130), dtype=torch.int32, device="cuda"))
    out = ops.detection_ap(*args, **given)
    assert all(o is given[k] for o, k in zip(out, ("ap", "pred_match", "gt_match", "order")))
    for x, y in zip(a, out):
        assert x.tobytes() == y.cpu().numpy().tobytes()
    with pytest.raises(ops._lib.DcapError, match="thresholds"):
        ops.detection_ap(*args[:-1], dev(np.linspace(0.1, 0.9, 17), torch.float64))


def test_detection_ap_refuses_what_the_header_says(ops):
    from image_captioning_amd import _lib
    lib = _lib.load()
    ov, n_det, n_gt, pcls, psc, gcls, thr = ap_case(8, 4, 1)
    t = dict(overlaps=dev(ov, torch.float64), n_det=dev(n_det, torch.int32), n_gt=dev(n_gt, torch.int32), pred_class=dev(pcls, torch.int32),
             pred_score=dev(psc), gt_class=dev(gcls, torch.int32), thresholds=dev(thr, torch.float64),
             ap=torch.full((3 * 10 + 1,), 3.0, dtype=torch.float64, device="cuda"))

    def call(**over):
        d = _lib.DetectionApDesc()
        d.B, d.Dmax, d.Gmax, d.ld, d.T = 3, 8, 4, 4, 10
        for k, v in t.items():
            setattr(d, k, v.data_ptr())
        for k, v in over.items():
            setattr(d, k, v)
        return lib.dc_detection_ap_f64(C.byref(d), None)
    for over in ([{k: None} for k in t] +
                 [dict(B=-1), dict(B=65536), dict(Dmax=1025), dict(Gmax=1025), dict(Dmax=-1), dict(Gmax=-1), dict(T=0), dict(T=17), dict(ld=3),
                  dict(overlaps=t["overlaps"].data_ptr() + 4), dict(ap=t["ap"].data_ptr() + 4), dict(n_det=t["n_det"].data_ptr() + 2),
                  dict(order=t["n_det"].data_ptr() + 1)]):
        assert call(**over) == _lib.EINVAL, over
    torch.cuda.synchronize()
    assert (t["ap"].cpu().numpy() == 3.0).all()
    assert call(B=0) == 0


# ---- MaskRCNN.evaluate ---------------------------------------------------------------------------------------------------------------
_EVAL = {}


def eval_run():
    """The model (three images a batch), the images, one detect call's results and the ground truth made from them: once."""
    if not _EVAL:
        from image_captioning_amd import mask_rle
        from test_gpu_maskrcnn_model import S, image, make_model
        model, cfg, _ = make_model(images=3)
        imgs = [image(7, 96, S), image(8, S, 80), image(9, 96, S)]
        found = model.detect(imgs, postprocess="device", refine="device", mask_format="rle")
        exact, perturbed = [], []
        for b, r in enumerate(found):
            n = len(r["rois"])
            dense = np.stack([mask_rle.decode(m) for m in r["masks"]], 2) if n else np.zeros(imgs[b].shape[:2] + (0,), np.uint8)
            exact.append({"class_ids": r["class_ids"].copy(), "masks": list(r["masks"]), "rois": r["rois"].copy()})
            moved = np.roll(dense, (2, -3), (0, 1))                               # shifted masks: IoUs on both sides of the thresholds
            moved[:, :, ::3] = dense[:, :, ::3]                                   # every third one exact
            ids = r["class_ids"].copy()
            ids[1::4] = ids[1::4] % (cfg.NUM_CLASSES - 1) + 1                     # some of another class
            keep = np.arange(n) % 5 != 4                                          # some detections without a ground truth
            perturbed.append({"class_ids": ids[keep], "masks": moved[:, :, keep]})
        none = {"class_ids": np.zeros(0, np.int32), "masks": np.zeros(imgs[2].shape[:2] + (0,), np.uint8)}
        _EVAL.update(model=model, imgs=imgs, found=found, exact=exact[:2] + [none], perturbed=perturbed[:2] + [none])
    return _EVAL


def _same_results(a, b):
    assert set(a) == set(b) == {"AP", "mAP", "gt_match", "n_det", "n_gt", "order", "pred_match", "skipped", "thresholds"}
    for k in ("AP", "mAP", "thresholds"):
        assert a[k].dtype == np.float64 and a[k].tobytes() == b[k].tobytes(), (k, a[k], b[k])
    for k in ("n_det", "n_gt"):
        assert a[k].dtype == b[k].dtype == np.int32 and np.array_equal(a[k], b[k]), k
    assert a["skipped"] == b["skipped"]
    for k in ("pred_match", "gt_match", "order"):
        assert len(a[k]) == len(b[k])
        for x, y in zip(a[k], b[k]):
            assert x.dtype == y.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y), k


@pytest.mark.parametrize("overlap", ["mask", "box"])
def test_evaluate_on_the_device_equals_the_host(ops, overlap, monkeypatch):
    from _decode_cases import record_host_syncs
    run = eval_run()
    model, imgs = run["model"], run["imgs"]
    host = model.evaluate(imgs, run["perturbed"], overlap=overlap, backend="host")
    with monkeypatch.context() as mp:
        mp.setattr(model, "EVAL_RLE_CAPACITY", 1 << 18)                          # (more words than the three images have pixels)
        calls = record_host_syncs(mp)
        device = model.evaluate(imgs, run["perturbed"], overlap=overlap, backend="device")
    assert calls == ["cpu", "numpy"], calls                                      # ONE device-to-host copy a batch
    _same_results(device, host)
    n_det = np.array([len(r["rois"]) for r in run["found"]], np.int32)
    print("overlap=%s: n_det %s, n_gt %s, AP@0.5 %s, mAP %s" % (overlap, n_det, host["n_gt"], host["AP"][:, 0], host["mAP"]))
    assert np.array_equal(host["n_det"], n_det) and n_det[:2].min() >= 2 and host["n_gt"][2] == 0 and host["skipped"] == 1
    assert host["AP"].shape == (3, 10) and np.isnan(host["AP"][2]).all() and not np.isnan(host["AP"][:2]).any()
    assert np.array_equal(_bits(host["mAP"]), _bits(host["AP"][:2].mean(axis=0)))
    assert (host["AP"][:2, 0] > 0).all() and (host["AP"][:2] < 1).any()          # the perturbation matches some and misses some
    assert [m.shape for m in host["pred_match"]] == [(10, n) for n in n_det] and model.last_eval_relaunched == []


@pytest.mark.parametrize("overlap", ["mask", "box"])
def test_evaluate_against_the_detections_themselves_is_one(ops, overlap):
    from image_captioning_amd import mask_rle
    run = eval_run()
    out = run["model"].evaluate(run["imgs"], run["exact"], overlap=overlap, backend="device")
    _same_results(out, run["model"].evaluate(run["imgs"], run["exact"], overlap=overlap, backend="host"))
    for b in range(2):
        assert all(mask_rle.area(m) for m in run["found"][b]["masks"])           # (an empty mask has IoU 0 with itself: pycocotools' 0 / 0)
        assert (out["AP"][b] == 1.0).all() and (out["pred_match"][b] >= 0).all(), (b, out["AP"][b])


def test_evaluate_with_a_small_rle_capacity_takes_the_second_launch(ops, monkeypatch):
    from _decode_cases import record_host_syncs
    run = eval_run()
    model = run["model"]
    want = model.evaluate(run["imgs"], run["perturbed"], backend="host")
    with monkeypatch.context() as mp:
        mp.setattr(model, "EVAL_RLE_CAPACITY", 8)
        calls = record_host_syncs(mp)
        got = model.evaluate(run["imgs"], run["perturbed"], backend="device")
    assert model.last_eval_relaunched == [0, 1] and calls == ["cpu", "numpy"] * 2        # a second copy for the batch, no more
    _same_results(got, want)


def test_evaluate_reads_dense_and_rle_ground_truth_alike_and_refuses_by_name(ops):
    from image_captioning_amd import mask_rle
    run = eval_run()
    model, imgs, gt = run["model"], run["imgs"], run["perturbed"]
    as_rle = [{"class_ids": g["class_ids"], "masks": [mask_rle.to_coco(mask_rle.encode(g["masks"][:, :, i])) for i in range(g["masks"].shape[2])],
               "iscrowd": np.arange(len(g["class_ids"])) % 2} for g in gt]
    crowd = [dict(g, iscrowd=np.arange(len(g["class_ids"])) % 2) for g in gt]
    a = model.evaluate(imgs, as_rle, iou_thresholds=[0.5, 0.6], backend="device")
    _same_results(a, model.evaluate(imgs, crowd, iou_thresholds=[0.5, 0.6], backend="host"))
    assert a["AP"].shape == (3, 2)
    with pytest.raises(ValueError, match="device_masks"):
        model.evaluate(imgs, gt, device_masks=True)
    with pytest.raises(ValueError, match="another size"):
        model.evaluate(imgs, [dict(gt[0], masks=gt[0]["masks"][:-1])] + gt[1:])
    with pytest.raises(ValueError, match="more than 1024 ground truths"):
        model.evaluate(imgs, [{"class_ids": np.ones(1025, np.int32), "masks": np.zeros(imgs[0].shape[:2] + (1025,), np.uint8)}] + gt[1:])
    with pytest.raises(ValueError, match="overlap"):
        model.evaluate(imgs, gt, overlap="polygon")
    with pytest.raises(ValueError, match="backend"):
        model.evaluate(imgs, gt, backend="numpy")
    with pytest.raises(ValueError, match="needs \"rois\""):
        model.evaluate(imgs, [{"class_ids": g["class_ids"]} for g in gt], overlap="box")
    with pytest.raises(ValueError, match="crowd"):
        model.evaluate(imgs, crowd, overlap="box")
    with pytest.raises(ValueError, match="thresholds"):
        model.evaluate(imgs, gt, iou_thresholds=np.linspace(0.1, 0.9, 17))
