"""The top of the pyramid driven by the RoI tile lists (EncoderPlan.forward_rois): the level-2 lateral tile list of
dc_roi_tile_groups_lateral against a host restatement, the list-driven pointwise convolution (dc_conv2d_nhwc_tiles_f32: fpn_c2p2 on the
tiles fpn_p2 reads) against the dense launch, the one launch for fpn_p2..p5 (dc_conv2d_winograd_levels_f32) against dense
convolutions, and forward_rois end to end.  Every comparison is torch.equal: no tolerances.  Helpers, maps and box sets are those of
test_gpu_fpn_rois.py."""
import numpy as np
import pytest
import torch

import test_gpu_fpn_rois as FR
from image_captioning_amd import _lib, ops

pytestmark = pytest.mark.gpu

F = np.float32
GH, GW = FR.GH, FR.GW
HW, HW1024 = FR.HW, [(256, 256), (128, 128), (64, 64), (32, 32)]
NAN = float("nan")


def _edge_set():
    """[2,4,4]: image 0 holds level-2 boxes in the last group row (bottom right: group 31 of the 8 x 4 grid, bottom left: group 28) and
    a zero box (pixel (0, 0)); image 1 holds one level-2 box in the middle and zero boxes -- its first group row is listed in column 0
    only, so a neighbour that leaked from image 0's last row into groups 34 / 35 would show."""
    img0 = [(0.9, 0.85, 1.0, 0.97), (0.9, 0.0, 1.0, 0.12), (0, 0, 0, 0), (0, 0, 0, 0)]
    img1 = [(0.5, 0.5, 0.62, 0.62), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
    return np.array([img0, img1], F)


def _dilate(listed, nb, hw):
    """Tiles of the level-2 map that hold a pixel within one pixel of a listed group, inside the same image -- pixel by pixel."""
    H, W = hw[0]
    gy, gx = -(-H // GH), -(-W // GW)
    tiles = set()
    for g in listed:
        i, r = divmod(g, gy * gx)
        a, b = divmod(r, gx)
        assert 0 <= i < nb
        for y in range(max(GH * a - 1, 0), min(GH * a + GH + 1, H)):
            for x in range(max(GW * b - 1, 0), min(GW * b + GW + 1, W)):
                tiles.add(FR._group_of(0, i, y, x, hw=hw))
    return tiles


def _host_lateral(boxes, hw):
    listed = {FR._group_of(0, *p, hw=hw) for p in FR._host_pixels(boxes, hw)[0]}
    return listed, _dilate(listed, boxes.shape[0], hw)


def test_edge_set_holds_the_cases_it_claims():
    listed, tiles = _host_lateral(_edge_set(), HW)
    gy, gx = 8, 4                                        # 64 x 64: 8 x 4 groups per image
    assert 31 in listed and 31 // gx == gy - 1           # last group row of image 0; its lower neighbour would be image 1's first row:
    assert not {34, 35} & tiles and {26, 27, 30, 31} <= tiles
    assert 28 in listed and 28 % gx == 0                 # column 0: its left neighbour would be the end of the row above
    assert 23 not in tiles and {24, 25, 28, 29} <= tiles
    assert 0 in listed and {0, 1, 4, 5} <= tiles         # the corner group of pixel (0, 0)
    assert 32 in listed and {32, 33, 36, 37} <= tiles     # image 1's own zero boxes


def _run_lists(boxes, hw, size):
    nb = boxes.shape[0]
    g = ops.RoiTileGroups(nb, hw, "cuda")
    g.lat_list.fill_(-7)                                 # entries behind the count must not matter
    g.lat_count.fill_(-7)
    g.marks.fill_(1)                                     # ... nor what the scratch held
    ops.roi_tile_groups(torch.tensor(boxes, device="cuda"), g, float(size * size), FR.POOL, lateral=True)
    n = int(g.lat_count.item())
    cap = nb * g.per_image[0]
    assert 0 <= n <= cap
    lst = g.lat_list.cpu().numpy()
    assert (lst[n:] == -7).all()                         # nothing behind the count is written
    lst = lst[:n].tolist()
    assert lst == sorted(set(lst)) and all(0 <= v < cap for v in lst), lst
    listed = g.lists[0].cpu().numpy()[:int(g.counts[0].item())].tolist()
    return lst, listed, cap


@pytest.mark.parametrize("which", ["all_levels", "empty_p4", "seeded", "edges", "benchmark", "scratch_marks"])
def test_lateral_list_matches_the_host_restatement(which):
    if which in ("benchmark", "scratch_marks"):
        boxes, hw, size = (FR._seeded_1024(2, 32, 1235) if which == "benchmark" else FR._seeded_1024(13, 6, 77)), HW1024, 1024
    else:
        boxes, hw, size = (dict(zip(("all_levels", "empty_p4", "seeded"), FR._box_sets()), edges=_edge_set())[which]), HW, FR.S
    lst, listed, _ = _run_lists(boxes, hw, size)
    want_listed, want = _host_lateral(boxes, hw)
    assert set(listed) == want_listed
    assert set(lst) == want, (sorted(want - set(lst)), sorted(set(lst) - want))


def test_lateral_list_is_empty_without_a_level_2_roi():
    boxes = np.array([[(0.02, 0.03, 0.98, 0.99), (0.3, 0.3, 0.74, 0.74)]] * 2, F)          # levels 4 and 3
    assert {FR._level(b) for b in boxes.reshape(-1, 4)} == {3, 4}
    lst, listed, _ = _run_lists(boxes, HW, FR.S)
    assert lst == [] and listed == []


def test_lateral_list_of_the_benchmark_boxes_covers_a_quarter_of_p2_at_most():
    """The benchmark's own boxes, unfiltered (the host restatement gives 178 of 1024 tiles, 17.4 %): the list is the one-pixel dilation
    of the device's own level-2 list, and short enough to be worth a list-driven launch."""
    from image_captioning_amd import synth
    boxes = (synth.rois(1235, 2, 32, 1024, 1024) / F(1024)).astype(F)
    lst, listed, cap = _run_lists(boxes, HW1024, 1024)
    assert set(lst) == _dilate(listed, 2, HW1024)
    H, W = HW1024[0]
    pixels = len(lst) * GH * GW                          # (256 x 256: no ragged tile)
    print("benchmark boxes: %d level-2 groups listed, %d lateral tiles of %d, %.1f %% of P2's pixels" % (len(listed), len(lst), cap, 100.0 * pixels / (2 * H * W)))
    assert pixels <= 0.25 * 2 * H * W


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pointwise_case():
    """N = 2, 42 x 56 (6 x 4 groups per image, last row and column ragged), 256 -> 256, upsample-add of a 21 x 28 map, scale and shift;
    the dense launch in the arithmetic the plan uses for fpn_c2p2: split-bf16, 128 x 128 tiles, no split-K."""
    N, H, W, Cc = 2, 42, 56, 256
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(N, H, W, Cc, device="cuda", generator=g)
    w = torch.randn(Cc, Cc, device="cuda", generator=g) / Cc ** 0.5
    sc = torch.rand(Cc, device="cuda", generator=g) + 0.5
    sh = torch.randn(Cc, device="cuda", generator=g)
    res = torch.randn(N, H // 2, W // 2, Cc, device="cuda", generator=g)
    assert ops.conv2d_kernel_name(x, w, 1, 1, 1, 0, 0, H, W, sc, sh, res, 2, False, split_k=1, math=_lib.MATH_BF16X3).startswith("igemm_bs_kernel<128, 128>")
    dense = ops.conv2d(x, w, 1, 1, 1, 0, 0, H, W, sc, sh, res, 2, False, out=torch.full((N, H, W, Cc), NAN, device="cuda"), split_k=1,
                       math=_lib.MATH_BF16X3)
    assert bool(torch.isfinite(dense).all())
    return x, w, sc, sh, res, dense


@pytest.mark.parametrize("count", [6, 3, 0])
def test_list_driven_pointwise_convolution_is_the_dense_one_on_the_listed_tiles(pointwise_case, count):
    x, w, sc, sh, res, dense = pointwise_case
    N, H, W, Cc = dense.shape
    groups = [0, 5, 10, 23, 24 + 7, 47]                  # the first group, interior ones, image 0's and image 1's ragged corner groups
    lst = torch.tensor(groups + [3] * (48 - len(groups)), dtype=torch.int32, device="cuda")
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    out = torch.full((N, H, W, Cc), NAN, device="cuda")
    ops.conv2d_tiles(x, w, lst, cnt, out, scale=sc, shift=sh, residual=res, res_mode=2)
    mask = torch.zeros(N, H, W, dtype=torch.bool, device="cuda")
    for gi in groups[:count]:
        n, r = divmod(gi, 24)
        gy, gx = divmod(r, 4)
        mask[n, GH * gy:GH * gy + GH, GW * gx:GW * gx + GW] = True
    assert torch.equal(out[mask], dense[mask])
    assert bool(torch.isnan(out[~mask]).all())


def test_list_driven_pointwise_convolution_without_an_add_operand(pointwise_case):
    x, w, sc, sh, _, _ = pointwise_case
    N, H, W, Cc = x.shape
    dense = ops.conv2d(x, w, 1, 1, 1, 0, 0, H, W, None, sh, None, 0, True, split_k=1, math=_lib.MATH_BF16X3)
    lst = torch.arange(48, dtype=torch.int32, device="cuda")
    out = torch.full((N, H, W, Cc), NAN, device="cuda")
    ops.conv2d_tiles(x, w, lst, torch.tensor([48], dtype=torch.int32, device="cuda"), out, shift=sh, relu=True)
    assert torch.equal(out, dense)                       # every tile listed: the whole map, ragged tiles included


def test_list_driven_pointwise_convolution_refuses_other_layers(pointwise_case):
    x, w, sc, sh, res, _ = pointwise_case
    N, H, W, Cc = x.shape
    lst, cnt = torch.zeros(48, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(N, H, W, Cc, device="cuda")
    with pytest.raises(_lib.DcapError):                  # split-K
        ops.conv2d_tiles(x, w, lst, cnt, out, scale=sc, shift=sh, residual=res, res_mode=2, split_k=2)
    with pytest.raises(_lib.DcapError):                  # where the dense rule would split (74 blocks), split_k = 0 is split-K too
        ops.conv2d_tiles(x, w, lst, cnt, out, scale=sc, shift=sh, residual=res, res_mode=2, split_k=0)
    for math in (_lib.MATH_F32, _lib.MATH_BF16X2, _lib.MATH_BF16):
        with pytest.raises(_lib.DcapError):              # another arithmetic
            ops.conv2d_tiles(x, w, lst, cnt, out, scale=sc, shift=sh, residual=res, res_mode=2, math=math)
    with pytest.raises(_lib.DcapError):                  # a plain residual
        ops.conv2d_tiles(x, w, lst, cnt, out, scale=sc, shift=sh, residual=torch.zeros_like(out), res_mode=1)
    with pytest.raises(_lib.DcapError):                  # 64 output channels: the dense launch runs 128 x 64 tiles
        ops.conv2d_tiles(x, w[:64].contiguous(), lst, cnt, torch.zeros(N, H, W, 64, device="cuda"), shift=sh[:64].contiguous())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def level_layers():
    """Four 3x3 layers, 64 -> 64, on the small plan's maps (the last a single ragged group per image) and their dense outputs."""
    Cc = 64
    g = torch.Generator(device="cuda").manual_seed(17)
    xs = [torch.randn(FR.B, h, w, Cc, device="cuda", generator=g) for h, w in HW]
    ws = [torch.randn(Cc, 9 * Cc, device="cuda", generator=g) / (9 * Cc) ** 0.5 for _ in HW]
    scs = [torch.rand(Cc, device="cuda", generator=g) + 0.5 for _ in HW]
    shs = [torch.randn(Cc, device="cuda", generator=g) for _ in HW]
    us = [ops.winograd_pack_b3(w, Cc, Cc) for w in ws]
    dense = [ops.conv2d(x, w, 3, 3, 1, 1, 1, x.shape[1], x.shape[2], sc, sh, None, 0, False, w_wino_b3=u) for x, w, sc, sh, u in zip(xs, ws, scs, shs, us)]
    assert all(bool(torch.isfinite(d).all()) for d in dense)
    return xs, ws, scs, shs, us, dense


@pytest.mark.parametrize("which", ["all_levels", "empty_p4", "all_empty"])
def test_one_launch_for_the_four_outputs_is_the_dense_convolutions_on_the_listed_groups(level_layers, which):
    xs, ws, scs, shs, us, dense = level_layers
    a, b, _ = FR._box_sets()
    g = ops.RoiTileGroups(FR.B, HW, "cuda")
    ops.roi_tile_groups(torch.tensor(a if which == "all_levels" else b, device="cuda"), g, float(FR.S * FR.S), FR.POOL)
    if which == "all_empty":
        g.counts.zero_()
    counts = g.counts.cpu().numpy().tolist()
    assert (all(counts) if which == "all_levels" else counts[2] == 0 and (any(counts) != (which == "all_empty")))
    outs = [torch.full_like(d, NAN) for d in dense]
    ops.conv2d_winograd_levels(xs, ws, us, g.lists, g.counts, outs, scales=scs, shifts=shs)
    for l, (out, want) in enumerate(zip(outs, dense)):
        H, W = HW[l]
        gx = -(-W // GW)
        mask = torch.zeros(FR.B, H, W, dtype=torch.bool, device="cuda")
        for gi in g.lists[l].cpu().numpy()[:counts[l]].tolist():
            n, r = divmod(gi, g.per_image[l])
            mask[n, GH * (r // gx):GH * (r // gx) + GH, GW * (r % gx):GW * (r % gx) + GW] = True
        assert torch.equal(out[mask], want[mask]), l
        assert bool(torch.isnan(out[~mask]).all()), l


def test_one_launch_for_the_four_outputs_refuses_unequal_layers(level_layers):
    xs, ws, scs, shs, us, dense = level_layers
    g = ops.RoiTileGroups(FR.B, HW, "cuda")
    outs = [torch.zeros_like(d) for d in dense]
    w32 = torch.zeros(32, 9 * 64, device="cuda")         # level 1 with 32 output channels
    with pytest.raises(_lib.DcapError):
        ops.conv2d_winograd_levels(xs, [ws[0], w32] + ws[2:], [us[0], ops.winograd_pack_b3(w32, 64, 32)] + us[2:], g.lists, g.counts,
                                   [outs[0], torch.zeros(FR.B, 32, 32, 32, device="cuda")] + outs[2:])
    with pytest.raises(_lib.DcapError):                  # relu on one level only
        ops.conv2d_winograd_levels(xs, ws, us, g.lists, g.counts, outs, relu=[True, False, False, False])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
# size 256: the small plan of test_gpu_fpn_rois.py -- its dense fpn_c2p2 splits K (128 blocks), so forward_rois keeps that launch dense and
# runs the list kernel and the one output launch; size 512: the smallest plan whose fpn_c2p2 is the 128 x 128 kernel without split-K
# (32 768 P2 pixels), where forward_rois runs the lateral on the listed tiles as it does at the benchmark's size.
@pytest.mark.parametrize("size", [256, 512])
def test_forward_rois_equals_the_dense_pass_and_leaves_no_stale_tile_behind(size):
    from image_captioning_amd import synth
    from image_captioning_amd.encoder import EncoderPlan
    plan = EncoderPlan(synth.encoder_weights(0, 2), FR.B, size, size, "cuda", stage4_blocks=2)
    img = torch.tensor(synth.images(7, FR.B, size, size), device="cuda")
    assert plan.sparse_rois and plan._lat_tiles == (size == 512)
    sets = [torch.tensor(b, device="cuda") for b in FR._box_sets()]
    plan.forward(img)
    dense = [plan.roi_features(boxes_norm=b).clone() for b in sets]
    assert all(bool(torch.isfinite(d).all()) for d in dense)
    did = []
    for b, want in zip(sets, dense):
        for p in plan.P + (plan.pre[0],):
            p.fill_(NAN)                                 # a value left by an earlier pass must not hide a missed group or tile
        got = plan.forward_rois(img, b.clone())          # (a fresh tensor every call: nothing captured may hold its address)
        did.append(plan._steps["rois%d" % FR.R].last)
        assert torch.equal(got, want), "call %d (%s): max |diff| %.3e" % (len(did), did[-1], float((got - want).abs().nan_to_num(1e30).max()))
    assert did == ["eager", "capture", "replay"]
    if plan._lat_tiles:                                  # t2 was written on the listed tiles only
        assert bool(torch.isnan(plan.pre[0]).any()) and bool(torch.isfinite(plan.pre[0]).any())
    plan.forward(img)                                    # the dense pass rewrites the maps whole: other boxes read no stale tile
    assert bool(torch.isfinite(plan.pre[0]).all())
    assert torch.equal(plan.roi_features(boxes_norm=sets[0]), dense[0])
    torch.cuda.synchronize()
