"""GenerationMatchLayer + unmold_generations on the device: ops.refine_generations against the product's own host functions
(dense_model.refine_generations(caption_scores=) followed by dense_model.unmold_generations, which test_golden_reference.py pins to the
reference), bit for bit, and DenseImageCapRCNN.generate_captions(postprocess="device") against postprocess="host".

The host functions are fed the device's own float64 caption scores (scores_out), so NumPy's log and pairwise summation stay out of the
comparison of decisions; scores_out itself is held against np.log(float64(p)).sum(1) within 1e-12 * max(1, |s|) (the device adds in
index order, NumPy pairwise: a few ulps of a sum of at most 15 terms), -inf matching -inf.  NumPy's default argsort promises no order
among equal scores, so the tie / NaN cases state the expected order themselves, np.argsort(kind="stable")[::-1], and run it through a
restatement of the host NMS."""
import types

import numpy as np
import pytest
import torch

from _decode_cases import record_host_syncs

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _cfg(side, thr=0.3, max_instances=100):
    return types.SimpleNamespace(IMAGE_SHAPE=np.array([side, side, 3]), DETECTION_NMS_THRESHOLD=thr, DETECTION_MAX_INSTANCES=max_instances)


def _dev(a, dt):
    return torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")


def _boxes(rng, n, nclu):
    """n normalised (y1,x1,y2,x2) float32 boxes around nclu centres: members of a cluster overlap by more than 0.3 often, not always;
    centres near the border put boxes partly and wholly outside a padded window."""
    c, hw = rng.uniform(0.02, 0.98, (nclu, 2)), rng.uniform(0.04, 0.3, (nclu, 2))
    which = rng.integers(0, nclu, n)
    ctr = c[which] + 0.15 * hw[which] * rng.standard_normal((n, 2))
    size = hw[which] * np.exp(0.25 * rng.standard_normal((n, 2)))
    return np.concatenate([ctr - 0.5 * size, ctr + 0.5 * size], axis=1).astype(F32)


def _word_scores(rng, n, T):
    return rng.uniform(0.05, 1.0, (n, T)).astype(F32)


def _device(rois, windows, shapes, cfg, word_scores=None, caption_scores=None):
    """ops.refine_generations -> host copies (boxes [B,M,4], keep [B,M], count [B], scores [B,N])."""
    from image_captioning_amd import ops, dense_model
    B = rois.shape[0]
    consts = np.stack([dense_model.refine_constants(windows[b], cfg, shapes[b]) for b in range(B)]).reshape(B, -1)
    kw = {}
    if word_scores is not None:
        kw["word_scores"] = _dev(word_scores, torch.float32)
    else:
        kw["caption_scores"] = _dev(caption_scores, torch.float32)[:, 0]          # column 0 of [B*N,k]: element stride k
    out = ops.refine_generations(_dev(rois, torch.float32), _dev(consts, torch.float64), cfg.DETECTION_NMS_THRESHOLD,
                                 cfg.DETECTION_MAX_INSTANCES, **kw)
    return [t.cpu().numpy() for t in out]


def _host(rois, scores, window, shape, cfg):
    """The product's host path for one image from given float64 caption scores -> (final boxes, kept RoI indices, boxes before
    unmolding, their non-empty mask)."""
    from image_captioning_amd import dense_model
    boxes, keep = dense_model.refine_generations(rois, None, window, cfg, caption_scores=scores)
    final, ok = dense_model.unmold_generations(boxes, shape, window)
    return final[ok], keep[ok], boxes, ok


def _nms_in_order(boxes, order, thr):
    """dense_model.non_max_suppression with the order given instead of np.argsort's."""
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    order, keep = np.asarray(order), []
    while order.size:
        i, rest = order[0], order[1:]
        keep.append(i)
        ih = np.maximum(np.minimum(boxes[i, 2], boxes[rest, 2]) - np.maximum(boxes[i, 0], boxes[rest, 0]), 0)
        iw = np.maximum(np.minimum(boxes[i, 3], boxes[rest, 3]) - np.maximum(boxes[i, 1], boxes[rest, 1]), 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = ih * iw / (area[i] + area[rest] - ih * iw)
        order = rest[~(iou > thr)]
    return np.asarray(keep, np.int32)


def _assert_image(got, b, want_boxes, want_keep):
    boxes, keep, count, _ = got
    n = len(want_keep)
    assert count[b] == n
    assert np.array_equal(keep[b, :n], want_keep) and np.all(keep[b, n:] == -1)
    assert np.array_equal(boxes[b, :n], want_boxes) and np.all(boxes[b, n:] == 0)
    assert boxes.dtype == np.int32 and keep.dtype == np.int32 and count.dtype == np.int32


def _assert_scores(scores, word_scores):
    with np.errstate(divide="ignore"):
        want = np.log(word_scores.astype(F64)).sum(1)
    got = scores.reshape(-1)
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf])
    assert np.all(np.abs(got[~inf] - want[~inf]) <= 1e-12 * np.maximum(1.0, np.abs(want[~inf])))


def _check(rois, windows, shapes, cfg, word_scores=None, caption_scores=None):
    """Device against host on every image of the batch; returns (device outputs, per-image host results)."""
    B, N = rois.shape[:2]
    got = _device(rois, windows, shapes, cfg, word_scores, caption_scores)
    assert got[3].dtype == np.float64 and got[3].shape == (B, N)
    if word_scores is not None:
        _assert_scores(got[3], word_scores)
    else:
        assert np.array_equal(got[3].reshape(-1), caption_scores[:, 0].astype(F64), equal_nan=True)
    hosts = []
    for b in range(B):
        h = _host(rois[b], got[3][b], windows[b], shapes[b], cfg)
        _assert_image(got, b, h[0], h[1])
        hosts.append(h)
    return got, hosts


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 130, 600])
def test_against_the_host_path_at_the_mask_word_edges_and_a_second_scan_group(gpu, N):
    """The edges of the mask's 64-bit words, and N = 600: a second group of the scan (NMS_G * 64 = 512).  A padded window on a
    non-power-of-two side, so boxes are clipped, some to nothing."""
    from image_captioning_amd import dense_model
    rng = np.random.default_rng(100 + N)
    cfg = _cfg(320, max_instances=N if N == 600 else 100)             # N = 600: no cut, the scan walks all ten words (two groups)
    rois = _boxes(rng, N, max(1, N // 6))[None]
    window = (40, 0, 280, 320)
    got, hosts = _check(rois, [window], [(300, 400, 3)], cfg, word_scores=_word_scores(rng, N, 15))
    if N >= 63:
        survivors = len(dense_model.non_max_suppression(dense_model.clip_to_window(window, rois[0].astype(F64) * 320.0), got[3][0], 0.3))
        assert 1 < got[2][0] <= survivors < N                         # the NMS suppresses, the filter drops, something is left


@pytest.mark.gpu
def test_batch_of_two_with_different_windows_at_1000_rois(gpu):
    rng = np.random.default_rng(7)
    cfg = _cfg(1024, max_instances=100)
    rois = np.stack([_boxes(rng, 1000, 150), _boxes(rng, 1000, 40)])
    windows, shapes = [(128, 0, 896, 1024), (0, 171, 1024, 853)], [(600, 800, 3), (1500, 1000, 3)]
    got, hosts = _check(rois, windows, shapes, cfg, word_scores=_word_scores(rng, 2000, 15))
    assert got[2][0] > 0 and got[2][1] > 0
    assert not np.array_equal(got[0][0], got[0][1])


# ---------------------------------------------------------------------------------------------- max_instances, padding
@pytest.mark.gpu
def test_max_instances_below_and_above_the_number_of_survivors(gpu):
    """Below: the cut happens BEFORE the empty-box filter, as on the host (a clipped-away box among the first max_instances takes a slot
    and is then dropped, so fewer than max_instances come out although more survived the NMS).  Above: the tail is -1 and the count
    is the number of survivors."""
    from image_captioning_amd import dense_model
    rng = np.random.default_rng(11)
    N = 200
    rois, ws = _boxes(rng, N, 60)[None], _word_scores(rng, N, 15)
    window, shape = (40, 0, 280, 320), (300, 400, 3)
    ws[:5] = 1.0 - 0.01 * np.arange(5, dtype=F32)[:, None]            # the five best captions ...
    rois[0, :5] = np.array([[0.01, 0.1 * i, 0.05, 0.1 * i + 0.08] for i in range(5)], F32)      # ... sit in the padding above the window
    below, above = _cfg(320, max_instances=20), _cfg(320, max_instances=190)
    got, hosts = _check(rois, [window], [shape], below, word_scores=ws)
    boxes = dense_model.clip_to_window(window, rois[0].astype(F64) * 320.0)
    survivors = len(dense_model.non_max_suppression(boxes, got[3][0], 0.3))
    assert 20 < survivors < 190
    assert got[2][0] <= 15 and not hosts[0][3].all()                # 20 slots, five of them empty boxes
    got, hosts = _check(rois, [window], [shape], above, word_scores=ws)
    assert got[2][0] == hosts[0][3].sum() <= survivors and np.all(got[1][0, survivors:] == -1)


@pytest.mark.gpu
def test_zero_padded_proposals_survive_the_nms_and_take_slots(gpu):
    """The ProposalLayer pads with all-zero RoIs, whose captions (and scores) are identical: 0/0 overlaps suppress nothing, so they all
    survive, take max_instances slots where their score ranks them, and leave at the empty-box filter."""
    rng = np.random.default_rng(13)
    N, pad = 130, 40
    rois, ws = _boxes(rng, N, 30)[None], _word_scores(rng, N, 15)
    rois[0, N - pad:] = 0
    ws[N - pad:] = 0.45
    cfg = _cfg(320, max_instances=60)
    got, hosts = _check(rois, [(40, 0, 280, 320)], [(300, 400, 3)], cfg, word_scores=ws)
    s = got[3][0]
    assert len(set(s[N - pad:])) == 1 and (s[:N - pad] < s[-1]).sum() > 20 and (s[:N - pad] > s[-1]).sum() > 5
    taken = len(hosts[0][2])                                           # slots used before the filter
    above = int((s[:N - pad] > s[-1]).sum())
    assert taken == 60 and 0 < got[2][0] <= above < 60                 # every slot is taken, at least 60 - above of them by padding
    assert (~hosts[0][3]).sum() >= 60 - above
    assert np.all(got[1][0, :got[2][0]] < N - pad)


# ---------------------------------------------------------------------------------------------- unmolding and rounding
@pytest.mark.gpu
def test_unmolding_padded_windows_and_a_box_that_empties_at_the_truncation(gpu):
    """IMAGE_SHAPE 320 with the window (40, 0, 280, 320) of a 300 x 400 original (scale 1.25) and the window (0, 40, 320, 280) of a
    150 x 100 original (scale 0.41...): boxes partly and wholly outside the window, and a planted best box (y 101..102) that is not
    empty after rint but is after (box - shift) * scale is truncated."""
    rng = np.random.default_rng(17)
    N = 90
    rois = np.stack([_boxes(rng, N, 25), _boxes(rng, N, 25)])
    ws = _word_scores(rng, 2 * N, 15)
    rois[1, 0] = np.array([101, 100, 102, 160], F32) / F32(320)
    ws[N] = 1.0
    rois[0, 1] = np.array([0.0, 0.2, 0.1, 0.4], F32)               # wholly above the first window
    rois[0, 2] = np.array([0.05, 0.2, 0.4, 0.5], F32)              # partly
    windows, shapes = [(40, 0, 280, 320), (0, 40, 320, 280)], [(300, 400, 3), (150, 100, 3)]
    got, hosts = _check(rois, windows, shapes, _cfg(320, max_instances=80), word_scores=ws)
    pre, ok = hosts[1][2], hosts[1][3]
    assert tuple(pre[0]) == (101, 100, 102, 160) and not ok[0]         # kept first, non-empty before unmolding, dropped after
    assert 0 not in got[1][1, :got[2][1]]
    assert not hosts[0][3].all() and hosts[0][3].any()


@pytest.mark.gpu
def test_half_integer_boxes_round_half_to_even(gpu):
    """Pixel boxes at exact half-integers (normalised (i + 0.5) / 1024, exact in float32, on a 1024 side): np.rint goes to the even
    neighbour, up for odd i and down for even i."""
    rng = np.random.default_rng(19)
    N = 100
    y1, x1 = rng.integers(0, 900, N), rng.integers(0, 900, N)
    px = np.stack([y1, x1, y1 + rng.integers(1, 120, N), x1 + rng.integers(1, 120, N)], axis=1) + 0.5
    rois = (px / 1024.0).astype(F32)[None]
    assert np.array_equal(rois[0].astype(F64) * 1024.0, px)
    got, hosts = _check(rois, [(0, 0, 1024, 1024)], [(1024, 1024, 3)], _cfg(1024, max_instances=100), word_scores=_word_scores(rng, N, 15))
    kept = got[1][0, :got[2][0]]
    want = np.rint(px[kept]).astype(np.int32)                           # scale 1, shift 0: the unmolded boxes are the rounded ones
    assert np.array_equal(got[0][0, :got[2][0]], want)
    up, down = np.floor(px[kept]) % 2 == 1, np.floor(px[kept]) % 2 == 0
    assert up.any() and down.any()
    assert np.array_equal(want[up], (px[kept][up] + 0.5).astype(np.int32)) and np.array_equal(want[down], (px[kept][down] - 0.5).astype(np.int32))


@pytest.mark.gpu
def test_overlap_equal_to_the_threshold_is_kept(gpu):
    """(0, 0, 10, 13) and (0, 7, 10, 20): intersection 60, union 200, 60 / 200 is the double 0.3 exactly.  With thr = 0.3 the overlap
    does not exceed it and both are kept; one ulp below 0.3 the second box goes."""
    rois = (np.array([[0, 0, 10, 13], [0, 7, 10, 20]], F64) / 1024.0).astype(F32)[None]
    assert 60.0 / 200.0 == 0.3
    ws = np.array([[0.9], [0.5]], F32)
    for thr, want in ((0.3, [0, 1]), (np.nextafter(0.3, 0.0), [0])):
        got, hosts = _check(rois, [(0, 0, 1024, 1024)], [(1024, 1024, 3)], _cfg(1024, thr=float(thr), max_instances=5), word_scores=ws)
        assert list(got[1][0, :got[2][0]]) == want


# ---------------------------------------------------------------------------------------------- the two score inputs
@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 15])
def test_word_scores_with_an_exact_zero(gpu, T):
    """A word probability of exactly 0 makes the caption score -inf: an ordinary value, ranked last."""
    rng = np.random.default_rng(23 + T)
    N = 70
    rois, ws = _boxes(rng, N, 50)[None], _word_scores(rng, N, T)
    ws[5, T // 2] = 0.0
    got, hosts = _check(rois, [(0, 0, 512, 512)], [(512, 512, 3)], _cfg(512, max_instances=70), word_scores=ws)
    assert got[3][0, 5] == -np.inf and np.isfinite(np.delete(got[3][0], 5)).all()
    n = got[2][0]
    assert 5 not in got[1][0, :n] or got[1][0, n - 1] == 5


@pytest.mark.gpu
def test_caption_scores_with_a_row_stride(gpu):
    """Column 0 of the beam decoder's [B*N, k] scores, k = 3; the other columns hold larger values that must not be read."""
    rng = np.random.default_rng(29)
    N = 150
    rois = np.stack([_boxes(rng, N, 40), _boxes(rng, N, 40)])
    cs = -rng.uniform(1.0, 30.0, (2 * N, 3)).astype(F32)
    cs[:, 1:] = 5.0
    _check(rois, [(0, 0, 512, 512), (64, 0, 448, 512)], [(512, 512, 3), (300, 400, 3)], _cfg(512, max_instances=50), caption_scores=cs)


# ---------------------------------------------------------------------------------------------- ties and NaN
@pytest.mark.gpu
def test_equal_scores_and_nan_follow_the_stable_sort_reversed(gpu):
    """The order is np.argsort(scores, kind="stable")[::-1]: among equal scores the HIGHER RoI index first, NaN first of all.  Planted:
    30 distinct best scores, then a run of 70 equal ones (ranks 30..99: across a mask-word edge), equal pairs further down, one NaN,
    a -0.0 beside a +0.0 (equal for NumPy) -- on boxes that overlap, so the order decides who survives."""
    from image_captioning_amd import dense_model
    rng = np.random.default_rng(31)
    N = 200
    rois = _boxes(rng, N, 25)[None]
    s = -rng.uniform(20.0, 40.0, N).astype(F32)
    perm = rng.permutation(N)
    s[perm[:30]] = -0.5 - 0.25 * np.arange(30, dtype=F32)
    s[perm[30:100]] = F32(-15.5)
    for a in range(100, 140, 2):
        s[perm[a + 1]] = s[perm[a]]
    s[perm[150]] = np.nan
    s[perm[151]], s[perm[152]] = F32(-0.0), F32(0.0)
    cfg = _cfg(320, max_instances=120)
    window, shape = (40, 0, 280, 320), (300, 400, 3)
    got = _device(rois, [window], [shape], cfg, caption_scores=np.repeat(s[:, None], 2, axis=1))
    assert np.array_equal(got[3][0], s.astype(F64), equal_nan=True)
    order = np.argsort(got[3][0], kind="stable")[::-1]
    assert order[0] == perm[150] and set(order[1:3]) == {perm[151], perm[152]} and order[1] > order[2]
    run = order[33:103]
    assert set(run) == set(perm[30:100]) and np.all(np.diff(run) < 0)
    boxes = dense_model.clip_to_window(window, rois[0].astype(F64) * 320.0)
    keep = _nms_in_order(boxes, order, 0.3)
    assert len(keep) < N                                               # the NMS suppresses something
    keep = keep[:120]
    final, ok = dense_model.unmold_generations(np.rint(boxes[keep]).astype(np.int32), shape, window)
    assert len(set(keep[ok]) & set(perm[30:100])) > 2                   # members of the run survive: their order was exercised
    _assert_image(got, 0, final[ok], keep[ok])


# ---------------------------------------------------------------------------------------------- empty inputs, refusals
@pytest.mark.gpu
def test_empty_batch_and_no_rois(gpu):
    from image_captioning_amd import ops
    for B, N in ((0, 7), (2, 0), (0, 0)):
        rois = torch.zeros((B, N, 4), device="cuda:0")
        consts = torch.zeros((B, 10), dtype=torch.float64, device="cuda:0")
        for kw in (dict(word_scores=torch.zeros((B * N, 15), device="cuda:0")), dict(caption_scores=torch.zeros((B * N, 3), device="cuda:0")[:, 0])):
            boxes, keep, count, scores = ops.refine_generations(rois, consts, 0.3, 9, **kw)
            assert tuple(boxes.shape) == (B, 9, 4) and tuple(keep.shape) == (B, 9) and tuple(count.shape) == (B,) and tuple(scores.shape) == (B, N)
            assert boxes.dtype == torch.int32 and keep.dtype == torch.int32 and count.dtype == torch.int32 and scores.dtype == torch.float64
            assert bool((keep == -1).all()) and bool((count == 0).all()) and bool((boxes == 0).all())


@pytest.mark.gpu
def test_refuses_more_rois_than_the_scan_holds_and_misshapen_tensors(gpu):
    from image_captioning_amd import ops, _lib
    consts = torch.zeros((1, 10), dtype=torch.float64, device="cuda:0")
    rois = torch.zeros((1, 8, 4), device="cuda:0")
    ws = torch.ones((8, 3), device="cuda:0")
    with pytest.raises(_lib.DcapError, match="8192"):
        ops.refine_generations(torch.zeros((1, 8193, 4), device="cuda:0"), consts, 0.3, 10, word_scores=torch.ones((8193, 1), device="cuda:0"))
    for bad in (dict(word_scores=ws[:7]), dict(word_scores=ws.double()), dict(word_scores=ws, caption_scores=ws[:, 0]), dict(),
                dict(caption_scores=ws.cpu()[:, 0]), dict(caption_scores=ws)):
        with pytest.raises(_lib.DcapError):
            ops.refine_generations(rois, consts, 0.3, 10, **bad)
    with pytest.raises(_lib.DcapError):
        ops.refine_generations(rois, consts.float(), 0.3, 10, word_scores=ws)
    with pytest.raises(_lib.DcapError):
        ops.refine_generations(rois, consts, 0.3, 0, word_scores=ws)
    with pytest.raises(_lib.DcapError):
        ops.refine_generations(rois.reshape(1, 4, 8), consts, 0.3, 10, word_scores=ws)


# ---------------------------------------------------------------------------------------------- the joint model
def _joint(images_per_gpu, S=256, V=1000, T=5, proposals=300, max_instances=50):
    """The joint model in inference mode on synthetic weights (as _decode_cases.joint_model, with the sizes open)."""
    from image_captioning_amd import synth
    from image_captioning_amd.config import Config
    from image_captioning_amd.dense_model import DenseImageCapRCNN

    class Cfg(Config):
        NAME = "joint"
        IMAGES_PER_GPU = images_per_gpu
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
        PADDING_SIZE = T
        VOCABULARY_SIZE = V
        EMBEDDING_SIZE = 300
        RECURRENT_DROPOUT = 0.0
        POST_NMS_ROIS_INFERENCE = proposals
        DETECTION_MAX_INSTANCES = max_instances
    cfg = Cfg()
    Wt = dict(synth.encoder_weights(0, 1), **synth.rpn_weights(4))
    Wt['rpn_conv_shared/kernel'] = Wt['rpn_conv_shared/kernel'] * np.float32(0.05)
    Wt['rpn_bbox_pred/kernel'] = Wt['rpn_bbox_pred/kernel'] * np.float32(0.3)
    Wt.update(synth.head_weights(1))
    Wt['mrcnn_class_conv1/kernel'] = Wt['mrcnn_class_conv1/kernel'] * np.float32(0.05)
    Wt.update(synth.v1_weights(2, V))
    Wt['imgcap_embedding_layer/embeddings'] = synth.embedding_matrix(3, V)
    cfg.EMBEDDING_WEIGHTS = Wt['imgcap_embedding_layer/embeddings']
    model = DenseImageCapRCNN("inference", cfg, "logs", stage4_blocks=1)
    model.set_weights(Wt)
    return model, cfg


@pytest.fixture(scope="module")
def joint1(gpu):
    return _joint(1)


def _caption_scores_are_apart(model, kw, b=0):
    """The condition on the input: the float64 caption scores the host leg's NMS was ordered by (recomputed from the same proposals;
    the zero-padded proposals, identical in everything, count once) differ by more than 1e-9 relative between sorted neighbours.
    Returns the number of real proposals."""
    props = model.last_proposals
    feats = model.plan().roi_features(boxes_norm=props)
    _, _, sc = model.caption_model.generate(feats[b], return_probabilities=False, **kw)
    s = sc[:, 0].astype(F64) if kw["decoder"] == "beam" else np.log(sc.astype(F64)).sum(1)
    real = np.abs(props[b].cpu().numpy()).sum(1) > 0
    s = np.sort(np.concatenate([s[real], s[~real][:1]]))
    assert np.all(np.diff(s) > 1e-9 * np.maximum(1.0, np.abs(s[1:]))), "near-tie in the caption scores: pick another image seed"
    return int(real.sum())


def _same(host, device):
    assert len(host) == len(device)
    for h, d in zip(host, device):
        assert sorted(h) == sorted(d)
        for key in h:
            assert h[key].dtype == d[key].dtype and h[key].shape == d[key].shape, key
            assert np.array_equal(h[key].view(np.int32), d[key].view(np.int32)), key


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(decoder="incremental"), dict(decoder="beam", beam_size=3, end_id=2)], ids=["incremental", "beam3"])
def test_generate_captions_device_equals_host(gpu, joint1, kw):
    from image_captioning_amd import synth
    model, cfg = joint1
    img = synth.images(7, 1, 256, 256)[0]
    host = model.generate_captions([img], return_probabilities=False, **kw)
    assert _caption_scores_are_apart(model, kw) > 50                  # enough real proposals for the NMS to matter
    device = model.generate_captions([img], return_probabilities=False, postprocess="device", **kw)
    assert 0 < len(host[0]["rois"]) <= cfg.DETECTION_MAX_INSTANCES
    assert sorted(host[0]) == (["beam_ids", "beam_scores", "ids", "rois"] if kw["decoder"] == "beam" else ["ids", "rois"])
    _same(host, device)


@pytest.mark.gpu
def test_generate_captions_device_equals_host_on_a_batch_of_two_sizes(gpu):
    from image_captioning_amd import synth
    model, cfg = _joint(2)
    imgs = [synth.images(8, 1, 200, 256)[0], synth.images(9, 1, 256, 150)[0]]
    for kw in (dict(decoder="incremental"), dict(decoder="beam", beam_size=3, end_id=2)):
        host = model.generate_captions(imgs, return_probabilities=False, **kw)
        for b in range(2):
            _caption_scores_are_apart(model, kw, b)
        device = model.generate_captions(imgs, return_probabilities=False, postprocess="device", **kw)
        assert len(host) == 2 and all(len(r["rois"]) > 0 for r in host)
        assert not np.array_equal(host[0]["rois"], host[1]["rois"])
        _same(host, device)


@pytest.mark.gpu
def test_the_device_path_copies_to_the_host_once(gpu, joint1, monkeypatch):
    """Between the image upload and the one result copy nothing comes to the host: the only Tensor.cpu / .item / .numpy / .tolist calls
    of a generate_captions(postprocess="device") are that copy's; the host path makes several."""
    from image_captioning_amd import synth
    model, cfg = joint1
    img = synth.images(7, 1, 256, 256)[0]
    for kw in (dict(decoder="incremental"), dict(decoder="beam", beam_size=3, end_id=2)):
        model.generate_captions([img], return_probabilities=False, postprocess="device", **kw)      # warm: buffers and workspaces
        calls = record_host_syncs(monkeypatch)
        model.generate_captions([img], return_probabilities=False, postprocess="device", **kw)
        monkeypatch.undo()
        assert calls == ["cpu", "numpy"]
        calls = record_host_syncs(monkeypatch)
        model.generate_captions([img], return_probabilities=False, **kw)
        monkeypatch.undo()
        assert calls.count("cpu") >= 2
