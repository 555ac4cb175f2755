"""The FPN output convolutions computed only where RoIAlign reads (EncoderPlan.forward_rois): the device-side list of tile groups
(dc_roi_tile_groups) against a float32 NumPy restatement of RoIAlign's routing and sampling, the list-driven Winograd launch
(dc_conv2d_winograd_groups_f32) against the dense one bit for bit, the plan's sparse pass against its dense pass through an eager, a
capturing and a replaying call, and the training pipeline with the sparse path on and off.  Seeded inputs only."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from image_captioning_amd import ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
S, B, R, POOL = 256, 2, 12, 7
HW = [(64, 64), (32, 32), (16, 16), (8, 8)]             # P2..P5 of a 256 x 256 image; P5 is one ragged tile group per image
GH, GW = 8, 16                                          # output pixels per tile group of the 32-tile Winograd items


def _box_sets():
    """Three [B,R,4] sets of normalised (y1, x1, y2, x2).  A holds every special case; B is A with the P4 boxes zero-padded away (an
    empty P4 list); C is seeded.  Side lengths keep log2(sqrt(h w) / 0.875) at least 0.1 away from a routing boundary (x.5)."""
    rng = np.random.default_rng(20)

    def seeded(n):
        out = []
        for _ in range(n):
            s = rng.choice([0.12, 0.2, 0.45, 0.5])
            y, x = rng.uniform(0.0, 1.0 - s, 2)
            out.append((y, x, y + s, x + s))
        return out

    img0 = [(0, 0, 0, 0),                               # zero-padded: level 2, every sample on pixel (0, 0)
            (0, 0, 1, 1),                               # level 4: step 15 / 6 = 2.5, the last sample lands exactly on H - 1 = 15
            (-0.2, -0.2, 1.2, 1.2),                     # level 5, partly outside: the first and last sample rows / columns are out of range
            (0.6, 0.2, 0.3, 0.5),                       # flipped in y: h w < 0, sqrt = NaN -> level 2, samples run upwards
            (0.7, 0.8, 0.45, 0.55),                     # flipped in both: level 2
            (0.1, 0.55, 0.25, 0.7),                     # level 2
            (0.3, 0.3, 0.74, 0.74),                     # level 3
            (0.05, 0.1, 0.9, 0.95),                     # level 4
            (0.5, 0.2, 0.5, 0.6)] + seeded(3)           # zero height: log(0) -> level 2, one sample row
    img1 = [(1.1, 1.1, 1.3, 1.3),                       # wholly outside: marks nothing
            (-0.05, 0.9, 0.1, 1.05),                    # level 2, partly outside
            (0.02, 0.03, 0.98, 0.99),                   # level 4
            (-0.15, -0.1, 1.25, 1.2),                   # level 5
            (0, 0, 0, 0)] + seeded(7)
    a = np.array([img0, img1], F)
    b = a.copy()
    for i in range(B):
        for j in range(R):
            if _level(b[i, j]) == 4:
                b[i, j] = 0
    c = np.array([seeded(R), seeded(R)], F)
    return a, b, c


def _level_f(box, size=S):
    y1, x1, y2, x2 = [F(v) for v in box]
    h, w = F(y2 - y1), F(x2 - x1)
    with np.errstate(all="ignore"):
        ratio = F(np.sqrt(F(h * w)) / F(F(224.0) / np.sqrt(F(size * size))))
        return F(np.log(ratio) / np.log(F(2.0)))


def _level(box, size=S):
    lvl = _level_f(box, size)
    if not lvl > -100:
        return 2
    return int(min(5, max(2, 4 + int(np.rint(lvl)))))


def _sample(lo, hi, p, n):
    lo, hi = F(lo), F(hi)
    step = F(F(F(hi - lo) * F(n - 1)) / F(POOL - 1))
    return F(F(lo * F(n - 1)) + F(F(p) * step))


def _host_pixels(boxes, hw=HW):
    """{level index: set of (image, y, x)}: the pixels RoIAlign reads, operation by operation in float32."""
    px = {l: set() for l in range(4)}
    for i in range(boxes.shape[0]):
        for j in range(boxes.shape[1]):
            li = _level(boxes[i, j], 4 * hw[0][0]) - 2
            H, W = hw[li]
            y1, x1, y2, x2 = boxes[i, j]
            for py in range(POOL):
                iy = _sample(y1, y2, py, H)
                if not (iy >= 0 and iy <= F(H - 1)):
                    continue
                for qx in range(POOL):
                    ix = _sample(x1, x2, qx, W)
                    if not (ix >= 0 and ix <= F(W - 1)):
                        continue
                    for y in (int(np.floor(iy)), int(np.ceil(iy))):
                        for x in (int(np.floor(ix)), int(np.ceil(ix))):
                            px[li].add((i, y, x))
    return px


def _group_of(li, i, y, x, hw=HW):
    H, W = hw[li]
    gy, gx = -(-H // GH), -(-W // GW)
    return (i * gy + y // GH) * gx + x // GW


def test_box_set_holds_the_cases_it_claims():
    a, b, _ = _box_sets()
    assert _sample(0, 1, POOL - 1, 16) == F(15) and _level(a[0, 1]) == 4          # lands exactly on H - 1
    assert {_level(x) for x in a.reshape(-1, 4)} == {2, 3, 4, 5}
    assert 4 not in {_level(x) for x in b.reshape(-1, 4)}
    assert any(not (_sample(-0.2, 1.2, p, 8) >= 0) for p in range(POOL)) and any(_sample(-0.2, 1.2, p, 8) >= 0 for p in range(POOL))
    pa = _host_pixels(a)
    assert all(pa[l] for l in range(4)) and (0, 0, 0) in pa[0]


def _seeded_1024(nb, nr, seed):
    """synth.rois on 1024 x 1024 images, normalised; boxes within 0.02 of a routing boundary are zero-padded away."""
    from image_captioning_amd import synth
    boxes = (synth.rois(seed, nb, nr, 1024, 1024) / F(1024)).astype(F)
    for i in range(nb):
        for j in range(nr):
            lvl = _level_f(boxes[i, j], 1024)
            if abs(float(lvl) - np.floor(float(lvl)) - 0.5) < 0.02:
                boxes[i, j] = 0
    return boxes


# which: the special boxes on the small maps (one scan chunk, marks in LDS); the benchmark's geometry (1360 groups: two scan chunks, the
# first ending exactly where P3's marks begin); 13 images of it (8840 groups: the marks in the caller's scratch, nine chunks)
@pytest.mark.parametrize("which", ["all_levels", "empty_p4", "benchmark", "scratch_marks"])
def test_tile_group_lists_match_the_host_restatement(which):
    if which in ("all_levels", "empty_p4"):
        a, b, _ = _box_sets()
        boxes, hw, size = (a if which == "all_levels" else b), HW, S
    else:
        boxes, hw, size = (_seeded_1024(2, 32, 1235) if which == "benchmark" else _seeded_1024(13, 6, 77)), [(256, 256), (128, 128), (64, 64), (32, 32)], 1024
    nb = boxes.shape[0]
    g = ops.RoiTileGroups(nb, hw, "cuda")
    assert g.per_image == [-(-h // GH) * -(-w // GW) for h, w in hw]
    assert g.per_image[3] == 1 or size == 1024
    for l in g.lists:
        l.fill_(-7)                                      # entries behind the count must not matter
    g.marks.fill_(1)                                     # ... nor what the scratch held
    ops.roi_tile_groups(torch.tensor(boxes, device="cuda"), g, float(size * size), POOL)
    counts = g.counts.cpu().numpy()
    want = _host_pixels(boxes, hw)
    for li in range(4):
        n = int(counts[li])
        assert 0 <= n <= nb * g.per_image[li]
        lst = g.lists[li].cpu().numpy()[:n].tolist()
        assert len(set(lst)) == n and lst == sorted(lst) and all(0 <= v < nb * g.per_image[li] for v in lst), (li, lst)
        need = {_group_of(li, *p, hw=hw) for p in want[li]}
        assert need <= set(lst), "level %d: pixels RoIAlign reads lie outside the list: groups %s" % (li + 2, sorted(need - set(lst)))
        assert need == set(lst), (li, sorted(set(lst) - need))
    if which == "empty_p4":
        assert counts[2] == 0 and not want[2]


_CONV_CHILD = r"""
import torch
from image_captioning_amd import ops
N, H, W, C = 2, 42, 56, 64                   # 6 x 4 tile groups per image, the last row (2 of 8 pixels) and column (8 of 16) ragged
g = torch.Generator(device='cuda').manual_seed(5)
x = torch.randn(N, H, W, C, device='cuda', generator=g)
w = torch.randn(C, 9 * C, device='cuda', generator=g) / (9 * C) ** 0.5
sc = torch.rand(C, device='cuda', generator=g) + 0.5
sh = torch.randn(C, device='cuda', generator=g)
u = ops.winograd_pack_b3(w, C, C)
nan = float('nan')
dense = ops.conv2d(x, w, 3, 3, 1, 1, 1, H, W, sc, sh, None, 0, True, out=torch.full((N, H, W, C), nan, device='cuda'), w_wino_b3=u)
assert bool(torch.isfinite(dense).all())
groups = [0, 5, 10, 23, 24 + 7, 47]          # the first group, interior ones, image 0's and image 1's ragged corner groups
lst = torch.tensor(groups + [3] * (48 - len(groups)), dtype=torch.int32, device='cuda')
for count in (len(groups), 3, 0):
    cnt = torch.tensor([count], dtype=torch.int32, device='cuda')
    out = torch.full((N, H, W, C), nan, device='cuda')
    ops.conv2d_winograd_groups(x, w, u, lst, cnt, out, scale=sc, shift=sh, relu=True)
    mask = torch.zeros(N, H, W, dtype=torch.bool, device='cuda')
    for gi in groups[:count]:
        n, r = divmod(gi, 24)
        gy, gx = divmod(r, 4)
        mask[n, 8 * gy:8 * gy + 8, 16 * gx:16 * gx + 16] = True
    assert torch.equal(out[mask], dense[mask]), count
    assert bool(torch.isnan(out[~mask]).all()), count
torch.cuda.synchronize()
print('groups ok')
"""


@pytest.mark.parametrize("cout", ["32", "64"])
def test_list_driven_convolution_is_the_dense_one_on_the_listed_groups(cout):
    """Both item widths (DCAP_WINO_COUT is read once per process: a child each), a full, a shortened and an empty list."""
    env = dict(os.environ, DCAP_WINO_COUT=cout)
    r = subprocess.run([sys.executable, "-c", _CONV_CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "groups ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_list_driven_convolution_refuses_other_layers():
    from image_captioning_amd import _lib
    x = torch.zeros(1, 16, 16, 48, device="cuda")
    w = torch.zeros(64, 9 * 48, device="cuda")
    lst, cnt = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.DcapError):                  # Cin = 48: wino_shape_ok refuses it, and so does this entry point
        ops.conv2d_winograd_groups(x, w, torch.zeros(48 * 48 * 64, dtype=torch.int16, device="cuda"), lst, cnt, torch.zeros(1, 16, 16, 64, device="cuda"))


@pytest.fixture(scope="module")
def small_plan():
    from image_captioning_amd import synth
    from image_captioning_amd.encoder import EncoderPlan
    plan = EncoderPlan(synth.encoder_weights(0, 2), B, S, S, "cuda", stage4_blocks=2)
    img = torch.tensor(synth.images(7, B, S, S), device="cuda")
    return plan, img


def test_forward_rois_equals_the_dense_pass_eager_captured_and_replayed(small_plan):
    plan, img = small_plan
    assert plan.sparse_rois
    sets = [torch.tensor(b, device="cuda") for b in _box_sets()]
    plan.forward(img)
    dense = [plan.roi_features(boxes_norm=b).clone() for b in sets]
    assert all(bool(torch.isfinite(d).all()) for d in dense)
    did = []
    for b, want in zip(sets, dense):
        for p in plan.P:
            p.fill_(float("nan"))                        # a value left by an earlier pass must not hide a missed group
        got = plan.forward_rois(img, b.clone())          # (a fresh tensor every call: nothing captured may hold its address)
        did.append(plan._steps["rois%d" % R].last)
        assert torch.equal(got, want), "call %d (%s): max |diff| %.3e" % (len(did), did[-1], float((got - want).abs().nan_to_num(1e30).max()))
    assert did == ["eager", "capture", "replay"]
    torch.cuda.synchronize()


def test_forward_rois_takes_the_dense_pass_where_the_maps_have_other_readers():
    from image_captioning_amd import synth
    from image_captioning_amd.encoder import EncoderPlan
    plan = EncoderPlan(synth.encoder_weights(0, 2), 1, S, S, "cuda", stage4_blocks=2, wino_products="f32")
    assert not plan.sparse_rois                          # fp32-product Winograd kernels on the FPN outputs: no list-driven form
    img = torch.tensor(synth.images(7, 1, S, S), device="cuda")
    boxes = torch.tensor(_box_sets()[0][:1], device="cuda")
    got = plan.forward_rois(img, boxes)
    assert bool(torch.isfinite(torch.stack(plan.P[3:])).all())
    assert torch.equal(got, plan.roi_features(boxes_norm=boxes))


def test_caption_pipeline_is_bit_identical_with_the_sparse_path_on_and_off(small_plan, monkeypatch):
    from image_captioning_amd import synth
    from image_captioning_amd.pipeline import CaptionTrainPipeline
    from image_captioning_amd.text_generation_model_v2 import Adam, DenseCapConfig, SampleTables, build_model
    plan, img = small_plan
    V, T = 1000, 6
    sets = [torch.tensor(b, device="cuda") for b in _box_sets()]
    tables = SampleTables.from_captions(synth.captions_v2(3, B * R, T, V, full=True), torch.device("cuda"))
    plan.images.copy_(img)
    results = {}
    for sparse in ("1", "0"):
        monkeypatch.setenv("DCAP_SPARSE_FPN", sparse)
        cfg = DenseCapConfig(V, synth.embedding_matrix(4, V))
        cfg.PADDING_SIZE = T
        dec = build_model((7, 7, 256), (T,), cfg, 256, inject=True, device=torch.device("cuda"), seed=5)
        dec.compile(optimizer=Adam(amsgrad=True), loss="categorical_crossentropy")
        pipe = CaptionTrainPipeline(plan, dec, R)
        assert pipe.sparse_fpn == (sparse == "1")
        losses = [pipe.step(None, b, tables) for b in sets] + [pipe.flush()]
        torch.cuda.synchronize()
        results[sparse] = ([float(l.item()) for l in losses if l is not None], dec.store.flat.clone())
    assert len(results["1"][0]) == 3 and all(np.isfinite(results["1"][0]))
    assert results["1"][0] == results["0"][0]
    assert torch.equal(results["1"][1], results["0"][1])
