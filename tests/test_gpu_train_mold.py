"""The joint model trained from data_generator(mold="device") batches -- raw images and flip flags, resized, padded and mirrored on the
device -- against a twin trained from the host generator's batches of the same seed.  The device writes the bytes the host path
uploads (tests/test_gpu_resize_flip.py), so every loss and every weight is equal bit for bit: eagerly, with the step captured and
replayed, through JointTrainPipeline, in test_on_batch and through train(mold="device", prefetch=2)."""
import numpy as np
import pytest
import torch

import _mold_cases as M
from _joint_cases import make_joint

pytestmark = pytest.mark.gpu

V, T, BLOCKS = 24, 5, 1


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def base(gpu):
    """(config class, weights) of the small joint model on a 128 x 128 canvas; every test builds its own models from them."""
    _, cfg, Wt = make_joint(M.MAX_DIM, V, T, BLOCKS)
    return type(cfg), cfg.EMBEDDING_WEIGHTS, Wt


def _config(base, B):
    cls, embedding, _ = base
    cfg = type("Cfg", (cls,), dict(IMAGE_MIN_DIM=M.MIN_DIM, IMAGES_PER_GPU=B, STEPS_PER_EPOCH=2))()       # (make_joint's does not resize)
    cfg.EMBEDDING_WEIGHTS = embedding
    assert cfg.BATCH_SIZE == B and tuple(cfg.IMAGE_SHAPE[:2]) == (M.MAX_DIM, M.MAX_DIM)
    return cfg


def _model(base, cfg, graph=False, model_dir="logs"):
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    m = DenseImageCapRCNN("training", cfg, model_dir, stage4_blocks=BLOCKS)
    m.set_weights(base[2])
    m.compile(1e-4)
    m.use_step_graph = graph
    return m


def _batches(cfg, n, rpn_targets, mold, seed=3):
    from image_captioning_amd.dense_model import data_generator
    gen = data_generator(M.make_dataset(T, V), cfg, augment=True, batch_size=cfg.BATCH_SIZE, rng=np.random.RandomState(seed),
                         rpn_targets=rpn_targets, mold=mold)
    return [next(gen)[0] for _ in range(n)]


def _no_host_resample(monkeypatch):
    from image_captioning_amd import utils

    def refuse(*a, **k):
        raise AssertionError("mold='device' resampled on the host")
    monkeypatch.setattr(utils, "imresize", refuse)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("B, rpn_targets", [(1, "host"), (2, "device")])
def test_twin_models_agree_bit_for_bit(gpu, base, monkeypatch, B, rpn_targets, graph):
    """Eager: three steps.  Captured (use_step_graph): four -- two eager warm-up steps, the capture, one replay."""
    from image_captioning_amd import utils
    cfg, steps = _config(base, B), 4 if graph else 3
    host_batches = _batches(cfg, steps, rpn_targets, "host")
    host, dev = _model(base, cfg, graph), _model(base, cfg, graph)
    want = [host.train_on_batch(b) for b in host_batches]
    _no_host_resample(monkeypatch)
    raw_batches = _batches(cfg, steps, rpn_targets, "device")
    flips = [f for b in raw_batches for f in b[0].flips]
    assert all(isinstance(b[0], utils.RawImageBatch) for b in raw_batches) and True in flips and False in flips
    got = [dev.train_on_batch(b) for b in raw_batches]
    assert got == want, (got, want)
    assert torch.equal(dev.store.flat, host.store.flat)
    assert np.array_equal(dev.plan().images.cpu().numpy(), M.canvases(raw_batches[-1][0]))       # the buffer the last step read
    assert len({tuple(l) for l in got}) == steps and all(np.isfinite(l).all() and l[1] > 0 for l in got)
    if graph:
        assert any(k[0] == "train" for k in dev._graphs) and dev.step_graph_fallback is None


def test_the_joint_pipeline_fed_raw_batches_equals_the_serial_steps(gpu, base, monkeypatch):
    from image_captioning_amd.pipeline import JointTrainPipeline
    cfg = _config(base, 1)
    host_batches = _batches(cfg, 4, "host", "host")
    serial, piped = _model(base, cfg), _model(base, cfg)
    want = [serial.train_on_batch_device(b).clone() for b in host_batches]
    _no_host_resample(monkeypatch)
    raw_batches = _batches(cfg, 4, "host", "device")
    pipe = JointTrainPipeline(piped)
    got = [l.clone() for l in (pipe.step(b) for b in raw_batches) if l is not None] + [pipe.flush().clone()]
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(got), torch.stack(want)) and torch.equal(piped.store.flat, serial.store.flat)
    assert len(np.unique(torch.stack(got).cpu().numpy(), axis=0)) == 4
    for j, b in ((0, raw_batches[2]), (1, raw_batches[3])):                      # the two plans hold the last two batches' canvases
        assert np.array_equal(pipe.plans[j].images.cpu().numpy(), M.canvases(b[0]))


def test_test_on_batch_takes_a_raw_batch(gpu, base, monkeypatch):
    """Twins again: a validation pass advances the model's validation streams (detection targets, RPN subsample), so the second pass of
    ONE model is another sample whatever it is fed."""
    cfg = _config(base, 2)
    host, dev = _model(base, cfg), _model(base, cfg)
    before = dev.store.flat.clone()
    want = host.test_on_batch(_batches(cfg, 1, "device", "host", seed=4)[0])
    _no_host_resample(monkeypatch)
    raw = _batches(cfg, 1, "device", "device", seed=4)[0]
    assert raw[0].flips == [True, True] and raw[1][:, 0].tolist() == [0, 1]      # the 100 x 68 image (padding 20 / 21) is mirrored
    got = dev.test_on_batch(raw)
    assert got == want and np.isfinite(got).all() and torch.equal(dev.store.flat, before)


def test_train_with_device_mold_and_prefetch_returns_the_same_history(gpu, base, tmp_path, monkeypatch):
    import threading
    cfg = _config(base, 1)

    def run(name, **kw):
        np.random.seed(11)                                   # train()'s generators draw from np.random
        m = _model(base, cfg, model_dir=str(tmp_path / name))
        hist = m.train(M.make_dataset(T, V), M.make_dataset(T, V), learning_rate=1e-5, epochs=1, layers="no_backbone", **kw)
        return hist, m.store.flat.clone()
    host, w_host = run("host", mold="host", prefetch=0)
    _no_host_resample(monkeypatch)
    device, w_device = run("device", mold="device", prefetch=2)
    assert len(host) == 1 and all(np.isfinite(v) for v in host[0].values()) and host[0]["rpn_class_loss"] > 0
    assert host == device and torch.equal(w_host, w_device)
    assert not any(t.name == "dcap-prefetch" and t.is_alive() for t in threading.enumerate())       # train() stopped its thread
