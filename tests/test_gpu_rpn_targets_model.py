"""The joint model fed data_generator(rpn_targets="device") batches -- the images' boxes at position 2, None at position 3 -- against a
twin fed the host arrays those boxes stand for: rpn_match from dense_model.build_rpn_targets with the keyed chooser
(tests/_rpn_targets_ref.py) at the model's own key and stream position, rpn_bbox the device's own delta rows.  Everything downstream of
the packed selection is the same launches on the same values, so losses and updated weights are equal bit for bit."""
import numpy as np
import pytest
import torch

import _rpn_targets_ref as R
from _joint_cases import make_joint

pytestmark = pytest.mark.gpu

S, V, T, BLOCKS = 256, 1000, 5, 1


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def base(gpu):
    """(cfg, weights) of the small joint model; every test builds its own models from them."""
    _, cfg, Wt = make_joint(S, V, T, BLOCKS)
    return cfg, Wt


def _model(base, B=1, graph=False, model_dir="logs"):
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    cfg, Wt = base
    cfg.IMAGES_PER_GPU, cfg.BATCH_SIZE = B, B
    m = DenseImageCapRCNN("training", cfg, model_dir, stage4_blocks=BLOCKS)
    m.set_weights(Wt)
    m.compile(1e-4)
    m.use_step_graph = graph
    return m


def _pyramid(cfg):
    from image_captioning_amd import utils
    anchors = utils.generate_pyramid_anchors(cfg.RPN_ANCHOR_SCALES, cfg.RPN_ANCHOR_RATIOS, cfg.BACKBONE_SHAPES, cfg.BACKBONE_STRIDES,
                                             cfg.RPN_ANCHOR_STRIDE)
    return anchors, [int(h * w * len(cfg.RPN_ANCHOR_RATIOS)) for h, w in cfg.BACKBONE_SHAPES]


def _device_batch(B, seed):
    """One data_generator(rpn_targets="device") batch: image b has 5 + 4 b boxes; the first three are its GT instances."""
    from image_captioning_amd import synth
    boxes = [R.random_boxes(seed + 10 * b, 5 + 4 * b, S) for b in range(B)]
    gt_boxes, gt_caps = np.zeros((B, 6, 4), np.float32), np.zeros((B, 6, T), np.int32)
    for b in range(B):
        gt_boxes[b, :3], gt_caps[b, :3] = boxes[b][:3], synth.captions_v1(seed + b, 3, T, V, lmin=1, lmax=3)
    return [synth.images(seed, B, S, S), np.zeros((B, 12)), boxes, None, gt_caps, gt_boxes]


def _host_batch(ops, model, batch, step, training=True):
    """The host arrays `batch` stands for at the model's stream position `step`."""
    cfg = model.config
    anchors, sizes = _pyramid(cfg)
    n, key, B = int(cfg.RPN_TRAIN_ANCHORS_PER_IMAGE), model._rpn_target_seed(training), len(batch[2])
    want = R.host_packed(anchors, batch[2], sizes, n, key, step, cfg.RPN_BBOX_STD_DEV)
    gt = np.zeros((B, max(len(b) for b in batch[2]), 4))
    for b, bx in enumerate(batch[2]):
        gt[b, :len(bx)] = bx
    out = ops.rpn_targets(torch.tensor(anchors, device="cuda"), torch.tensor(gt, device="cuda"),
                          torch.tensor([len(b) for b in batch[2]], dtype=torch.int32, device="cuda"), sizes, n, cfg.RPN_BBOX_STD_DEV, key, offset=step)
    counts, rows = out[0].cpu().numpy(), out[4].cpu().numpy()
    assert counts.tolist() == want["counts"].tolist() and np.array_equal(out[3].cpu().numpy()[:counts[0]], want["mt"])
    bbox, at = np.zeros((B, n, 4), np.float32), 0
    for b in range(B):
        k = int((want["match"][b] == 1).sum())
        bbox[b, :k] = rows[at:at + k]
        at += k
    return [batch[0], batch[1], want["match"][:, :, None], bbox, batch[4], batch[5]]


@pytest.mark.parametrize("B, graph", [(1, False), (2, False), (1, True), (2, True)])
def test_device_built_targets_equal_the_host_arrays_bit_for_bit(gpu, base, B, graph):
    """Eager: two steps.  Captured (use_step_graph): four -- two eager warm-up steps, the capture, one replay."""
    from image_captioning_amd import ops
    steps = 4 if graph else 2
    batches = [_device_batch(B, 30 + s) for s in range(steps)]
    dev, twin = _model(base, B, graph), _model(base, B, graph)
    got = [dev.train_on_batch(b) for b in batches]
    want = [twin.train_on_batch(_host_batch(ops, twin, b, s + 1)) for s, b in enumerate(batches)]
    assert got == want, (got, want)
    assert torch.equal(dev.store.flat, twin.store.flat)
    assert len({tuple(l) for l in got}) == steps and all(l[1] > 0 and l[2] > 0 for l in got)      # different batches, live RPN losses
    if graph:
        assert any(k[0] == "train" for k in dev._graphs) and dev.step_graph_fallback is None


def test_the_joint_pipeline_equals_the_serial_steps(gpu, base):
    from image_captioning_amd.pipeline import JointTrainPipeline
    batches = [_device_batch(1, 50 + s) for s in range(4)]
    serial, piped = _model(base), _model(base)
    want = [serial.train_on_batch_device(b).clone() for b in batches]
    pipe = JointTrainPipeline(piped)
    got = [l.clone() for l in (pipe.step(b) for b in batches) if l is not None] + [pipe.flush().clone()]
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(got), torch.stack(want)) and torch.equal(piped.store.flat, serial.store.flat)
    assert len(np.unique(torch.stack(got).cpu().numpy(), axis=0)) == 4


def test_validation_draws_from_its_own_stream(gpu, base):
    a, b = _model(base), _model(base)
    batches = [_device_batch(1, 70 + s) for s in range(3)]
    la = [a.train_on_batch(batches[0]), a.train_on_batch(batches[1])]
    lb = [b.train_on_batch(batches[0])]
    val = b.test_on_batch(batches[2])
    lb.append(b.train_on_batch(batches[1]))
    assert la == lb and torch.equal(a.store.flat, b.store.flat)
    assert np.isfinite(val).all() and val[1] > 0
    assert b._rpn_target_seed(True) != b._rpn_target_seed(False)


def test_train_runs_an_epoch_without_the_host_function(gpu, base, tmp_path, monkeypatch):
    from image_captioning_amd import dense_model, utils
    cfg, Wt = base

    class Toy(utils.Dataset):
        def load_image(self, image_id):
            return np.random.RandomState(image_id).randint(0, 255, (S, S, 3)).astype(np.uint8)

        def load_captions_and_rois(self, image_id):
            r = np.random.RandomState(100 + image_id)
            n = 2 + image_id % 3
            caps = np.zeros((n, T), np.float32)
            caps[:, 0], caps[:, 1:3], caps[:, 3] = 1, r.randint(3, V, (n, 2)), 2
            return R.random_boxes(200 + image_id, n, S).astype(np.int64), caps
    train, val = Toy(), Toy()
    for ds, ids in ((train, range(4)), (val, range(4, 6))):
        for i in ids:
            ds.add_image("toy", image_id=i, path=None)
        ds.prepare()

    def never(*a, **k):
        raise AssertionError("build_rpn_targets called with rpn_targets='device'")
    monkeypatch.setattr(dense_model, "build_rpn_targets", never)
    monkeypatch.setattr(cfg, "STEPS_PER_EPOCH", 3, raising=False)
    m = _model(base, model_dir=str(tmp_path / "logs"))
    before = m.store.flat.clone()
    hist = m.train(train, val, learning_rate=1e-5, epochs=1, layers="no_backbone", rpn_targets="device")
    assert len(hist) == 1 and all(np.isfinite(v) for v in hist[0].values())
    assert hist[0]["rpn_class_loss"] > 0 and hist[0]["val_rpn_class_loss"] > 0
    assert not torch.equal(before, m.store.flat)
