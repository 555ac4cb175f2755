"""Device-built RPN targets, the parts that need no GPU: the keyed chooser that makes dense_model.build_rpn_targets reproduce the
device's subsample (tests/_rpn_targets_ref.py), data_generator(rpn_targets="device"), and the argument refusals."""
import numpy as np
import pytest

import _rpn_targets_ref as R

BOXES = R.random_boxes(1, 24, 128)


def _uncut(anchors, boxes):
    """The matching before any subsampling: a budget no class reaches."""
    return R.host_targets(anchors, boxes, 2 * anchors.shape[0], seed=0)[0]


@pytest.mark.parametrize("budget", [16, 256])
def test_the_keyed_chooser_keeps_the_smallest_pairs(budget):
    anchors, _ = R.pyramid(128)
    full = _uncut(anchors, BOXES)
    pos, neg = np.nonzero(full == 1)[0], np.nonzero(full == -1)[0]
    assert len(pos) > 8 and len(neg) > 256                      # budget 16 cuts both classes, budget 256 only the negatives
    seed, offset = 1234, 7
    match, deltas = R.host_targets(anchors, BOXES, budget, seed, offset)
    n_pos = min(len(pos), budget // 2)
    assert int((match == 1).sum()) == n_pos and int((match == -1).sum()) == budget - n_pos
    for ids, kept in ((pos, n_pos), (neg, budget - n_pos)):
        order = np.lexsort((ids, R.keys(ids, seed, offset)))
        want = np.sort(ids[order[:kept]])
        assert np.array_equal(np.nonzero(match == full[ids[0]])[0], want)
    assert not deltas[n_pos:].any() and np.isfinite(deltas).all()


def test_the_chooser_is_a_pure_function_of_seed_and_offset():
    anchors, _ = R.pyramid(128)
    a = R.KeyedChooser(5, 3)
    ids = np.arange(0, 4092, 3)
    first = a.choice(ids, 100)
    a.choice(ids[::-1], 7)                                      # other calls in between change nothing: no state
    assert np.array_equal(a.choice(ids, 100), first)
    assert np.array_equal(np.sort(a.choice(ids[::-1].copy(), 100)), np.sort(first))          # ... nor does the order of the ids
    assert np.array_equal(R.KeyedChooser(5, 3).choice(ids, 100), first)
    assert not np.array_equal(np.sort(R.KeyedChooser(5, 4).choice(ids, 100)), np.sort(first))
    assert not np.array_equal(np.sort(R.KeyedChooser(6, 3).choice(ids, 100)), np.sort(first))
    m1, m2 = R.host_targets(anchors, BOXES, 16, 5, 3)[0], R.host_targets(anchors, BOXES, 16, 5, 4)[0]
    full = _uncut(anchors, BOXES)
    assert not np.array_equal(m1, m2)                           # another offset: another cut ...
    assert np.all(full[m1 != 0] == m1[m1 != 0]) and np.all(full[m2 != 0] == m2[m2 != 0])      # ... of the same matching


def test_without_boxes_every_anchor_is_a_negative():
    anchors, _ = R.pyramid(128)
    match, deltas = R.host_targets(anchors, np.zeros((0, 4)), 16, 9)
    assert int((match == -1).sum()) == 16 and not (match == 1).any() and not deltas.any()


def test_host_packed_is_the_steps_own_packing():
    """selection() restates DenseImageCapRCNN._rpn_selection; checked against the method itself on a stub that has only what it reads."""
    import types
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    anchors, sizes = R.pyramid(128)
    heads = [types.SimpleNamespace(shape=(2, 128 // s, 128 // s, 20)) for s in (4, 8, 16, 32, 64)]
    stub = types.SimpleNamespace(A=3, plan=lambda: types.SimpleNamespace(rpn_heads=heads))
    match = R.host_targets(anchors, BOXES, 64, 3)[0]
    for image in (0, 1):
        want = DenseImageCapRCNN._rpn_selection(stub, match, image)
        assert all(np.array_equal(a, b) for a, b in zip(R.selection(match, sizes, image), want))
    p = R.host_packed(anchors, [BOXES, BOXES[:1]], sizes, 64, 3)
    assert p["counts"][0] == len(p["lvl"]) == 128 and p["counts"][1] == p["deltas"].shape[0] == int((p["mt"] == 1).sum())
    assert not np.array_equal(p["match"][0], p["match"][1])


# ------------------------------------------------------------------------------------------------ the generator
def _toy(cfg, boxes_of=None):
    from image_captioning_amd.utils import Dataset

    class Toy(Dataset):
        def load_image(self, image_id):
            return np.random.RandomState(image_id).randint(0, 255, (96, 128, 3)).astype(np.uint8)

        def load_captions_and_rois(self, image_id):
            n = boxes_of(image_id) if boxes_of is not None else (7 if image_id == 0 else 2 + image_id % 3)
            r = np.random.RandomState(image_id)
            y, x = r.randint(0, 60, n), r.randint(0, 60, n)
            boxes = np.stack([y, x, y + r.randint(8, 60, n), x + r.randint(8, 60, n)], axis=1).reshape(n, 4)
            return boxes, r.randint(1, 9, (n, cfg.PADDING_SIZE)).astype(np.float32)
    ds = Toy()
    for i in range(4):
        ds.add_image("toy", image_id=i, path=None)
    ds.prepare()
    return ds


def _cfg():
    from image_captioning_amd.config import Config

    class Cfg(Config):
        IMAGES_PER_GPU = 1
        IMAGE_MIN_DIM = 128
        IMAGE_MAX_DIM = 128
        TRAIN_ROIS_PER_IMAGE = 12
        PADDING_SIZE = 5
        MAX_GT_INSTANCES = 5
        RPN_TRAIN_ANCHORS_PER_IMAGE = 64
    return Cfg()


def _todays_generator(dataset, config, batch_size, rng):
    """The host generator as it stood before the rpn_targets argument, restated from its public pieces (shuffle and augment on)."""
    from image_captioning_amd import dense_model as D, utils
    anchors = utils.generate_pyramid_anchors(config.RPN_ANCHOR_SCALES, config.RPN_ANCHOR_RATIOS, config.BACKBONE_SHAPES,
                                             config.BACKBONE_STRIDES, config.RPN_ANCHOR_STRIDE)
    ids, index, batch = np.copy(dataset.image_ids), -1, []
    while True:
        index = (index + 1) % len(ids)
        if index == 0:
            rng.shuffle(ids)
        image, meta, caps, boxes = D.load_image_gt(dataset, config, ids[index], True, rng)
        match, deltas = D.build_rpn_targets(image.shape, anchors, caps, boxes, config, rng)
        if boxes.shape[0] > config.MAX_GT_INSTANCES:
            pick = rng.choice(np.arange(boxes.shape[0]), config.MAX_GT_INSTANCES, replace=False)
            caps, boxes = caps[pick], boxes[pick]
        gc, gb = np.zeros((config.MAX_GT_INSTANCES, config.PADDING_SIZE), caps.dtype), np.zeros((config.MAX_GT_INSTANCES, 4), boxes.dtype)
        gc[:caps.shape[0]], gb[:boxes.shape[0]] = caps, boxes
        batch.append((D.mold_image(image.astype(np.float32), config).astype(np.float32), meta, match[:, None], deltas, gc, gb))
        if len(batch) == batch_size:
            yield [np.stack([b[k] for b in batch]) for k in range(6)]
            batch = []


def test_the_host_mode_is_todays_generator_and_stream():
    from image_captioning_amd.dense_model import data_generator
    cfg = _cfg()
    ds = _toy(cfg)
    runs = []
    for kwargs in ({}, {"rpn_targets": "host"}):
        rng = np.random.RandomState(11)
        gen = data_generator(ds, cfg, batch_size=2, rng=rng, **kwargs)
        runs.append(([next(gen) for _ in range(5)], rng.randint(0, 2 ** 31, 4)))           # 10 images: into the third epoch's shuffle
    rng = np.random.RandomState(11)
    ref = _todays_generator(ds, cfg, 2, rng)
    want = ([next(ref) for _ in range(5)], rng.randint(0, 2 ** 31, 4))
    for batches, tail in runs:
        assert np.array_equal(tail, want[1])                    # the same draws were consumed
        for (inputs, outputs), w in zip(batches, want[0]):
            assert outputs == [] and len(inputs) == 6
            assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(inputs, w))


def test_the_device_mode_yields_the_boxes_instead_of_the_targets(monkeypatch):
    from image_captioning_amd import dense_model as D
    cfg = _cfg()
    ds = _toy(cfg)

    def never(*a, **k):
        raise AssertionError("build_rpn_targets called in device mode")
    host = D.data_generator(ds, cfg, shuffle=False, augment=False, batch_size=2, rng=np.random.RandomState(0))
    first_host = next(host)[0]
    monkeypatch.setattr(D, "build_rpn_targets", never)
    gen = D.data_generator(ds, cfg, shuffle=False, augment=False, batch_size=2, rng=np.random.RandomState(0), rpn_targets="device")
    inputs, outputs = next(gen)
    assert outputs == [] and len(inputs) == 6 and inputs[3] is None
    images, metas, boxes, _, caps, gt_boxes = inputs
    assert isinstance(boxes, list) and [b.shape for b in boxes] == [(7, 4), (3, 4)]        # ALL boxes, before the MAX_GT_INSTANCES pick
    for b, image_id in zip(boxes, (0, 1)):
        assert np.array_equal(b, ds.load_captions_and_rois(image_id)[0])
    assert np.array_equal(images, first_host[0]) and np.array_equal(metas, first_host[1])
    assert caps.shape == (2, 5, 5) and gt_boxes.shape == (2, 5, 4) and np.all(np.abs(gt_boxes[0]).sum(axis=1) > 0)
    assert np.array_equal(gt_boxes[1], first_host[5][1]) and np.array_equal(caps[1], first_host[4][1])   # (image 1: no pick, no draw)
    second = next(gen)[0]
    assert [b.shape[0] for b in second[2]] == [4, 2] and second[2] is not boxes


def test_the_device_mode_skips_an_image_without_boxes_and_refuses_too_many():
    from image_captioning_amd.dense_model import data_generator
    cfg = _cfg()
    gen = data_generator(_toy(cfg, lambda i: 0 if i == 1 else 2), cfg, shuffle=False, augment=False, batch_size=1, rpn_targets="device")
    metas = [next(gen)[0][1][0, 0] for _ in range(3)]
    assert metas == [0, 2, 3]                                   # image 1 has no boxes: skipped, as the host path skips it
    gen = data_generator(_toy(cfg, lambda i: 513 if i == 1 else 2), cfg, shuffle=False, augment=False, batch_size=1, rpn_targets="device")
    next(gen)
    with pytest.raises(ValueError, match='rpn_targets="host"'):
        next(gen)
    with pytest.raises(ValueError, match="rpn_targets must be"):
        next(data_generator(_toy(cfg), cfg, rpn_targets="gpu"))


# ------------------------------------------------------------------------------------------------ refusals, on attribute-less stubs
def test_an_unknown_mode_is_refused_before_the_model_is_touched():
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    from image_captioning_amd import train_dense_captions

    class Untouchable(object):
        def __getattr__(self, name):
            raise AssertionError("the model was touched: %s" % name)
    with pytest.raises(ValueError, match="rpn_targets must be"):
        DenseImageCapRCNN.train(Untouchable(), None, None, 1e-3, 1, "no_backbone", rpn_targets="Device")
    with pytest.raises(ValueError, match="rpn_targets must be"):
        train_dense_captions.main(root_dir="/nonexistent", rpn_targets="gpu")


def test_the_step_refuses_more_boxes_than_the_device_covers():
    import types
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    stub = types.SimpleNamespace(images_per_gpu=1)
    with pytest.raises(ValueError, match='rpn_targets="host"'):
        DenseImageCapRCNN._rpn_box_parts(stub, [np.zeros((513, 4))])
    with pytest.raises(ValueError, match="IMAGES_PER_GPU"):
        DenseImageCapRCNN._rpn_box_parts(stub, [np.zeros((2, 4)), np.zeros((2, 4))])
    parts = DenseImageCapRCNN._rpn_box_parts(stub, [np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.int32)])
    assert parts["rpn_gtc"].tolist() == [2] and parts["rpn_gt"].dtype == np.int32 and parts["rpn_gt"].size == 8 * 512
    assert np.array_equal(parts["rpn_gt"].view(np.float64).reshape(512, 4)[:2], [[1, 2, 3, 4], [5, 6, 7, 8]])


def test_the_wrapper_rejects_host_tensors_and_bad_shapes():
    import torch
    from image_captioning_amd import _lib, ops
    a, g, c = torch.zeros(12, 4, dtype=torch.float64), torch.zeros(1, 2, 4, dtype=torch.float64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.DcapError, match="must live on the GPU"):
        ops.rpn_targets(a, g, c, [12], 4, (0.1, 0.1, 0.2, 0.2), seed=1)
