"""Resize and pad on the device (ops.resize_pad_images / dc_resize_pad_u8) against PIL, byte for byte, and mold="device" of the
inference and training entry points against mold="host" on every result.

No tolerance anywhere: the kernels restate PIL's integer algorithm (tests/_resize_ref.py pins the written steps to the installed
Pillow on the CPU), so the canvas is np.array_equal to Image.resize(BILINEAR) + np.pad and everything computed from it is the host
path's bit for bit.  Outputs are pre-filled with 0xAA, so a padding byte the kernel leaves unwritten shows."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import _resize_ref as R


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _centre(new, size):
    return (size - new) // 2


def _run(images, sizes, canvas):
    """Each image resized to its (new_h, new_w), centred as resize_image centres it, into a 0xAA-filled canvas -> (got, want)."""
    from image_captioning_amd import ops
    H, W = canvas
    place = [(nh, nw, _centre(nh, H), _centre(nw, W)) for nh, nw in sizes]
    out = torch.full((len(images), H, W, 3), 0xAA, dtype=torch.uint8, device="cuda:0")
    got = ops.resize_pad_images(images, placements=place, out=out)
    assert got is out
    want = np.stack([R.padded(R.pil_resize(im, nh, nw), H, W, top, left) for im, (nh, nw, top, left) in zip(images, place)])
    return got.cpu().numpy(), want


CASES = [((60, 80), (77, 102), (128, 128)),          # non-integer upscale, odd padding remainder on both axes
         ((150, 201), (64, 86), (128, 128)),         # downscale by 2.34: rows of 7 coefficients
         ((300, 17), (31, 170), (64, 192)),          # rows of 21 one way, a tenfold upscale the other (wider than 128: its own canvas)
         ((5, 7), (128, 128), (128, 128)),           # edge clamping everywhere, no padding
         ((1, 9), (3, 27), (128, 128)),              # one source row
         ((40, 64), (80, 64), (128, 128)),           # the horizontal pass is the identity
         ((64, 40), (64, 90), (128, 128)),           # the vertical pass is the identity
         ((97, 131), (97, 131), (160, 160)),         # pure copy plus pad (odd sizes; wider than 128: its own canvas)
         ((600, 800), (768, 1024), (1024, 1024))]    # the production shape: more blocks per row than one, 1024 grid rows


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst,canvas", CASES, ids=["%dx%d-%dx%d" % (s + d) for s, d, _ in CASES])
def test_kernel_equals_pil_on_noise(gpu, src, dst, canvas):
    got, want = _run([_noise(src[0] * 1000 + src[1], *src)], [dst], canvas)
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("value", [0, 255])
def test_constant_images(gpu, value):
    got, want = _run([np.full((37, 53, 3), value, np.uint8)], [(128, 96)], (128, 128))
    assert np.array_equal(got, want) and (got[0, :, 16:112] == value).all() and (got[0, :, :16] == 0).all()


@pytest.mark.gpu
def test_three_sizes_in_one_call_at_odd_byte_offsets(gpu):
    from image_captioning_amd import ops
    images = [_noise(1, 35, 51), _noise(2, 150, 201), _noise(3, 64, 40)]
    sizes = [(77, 102), (64, 86), (64, 90)]
    place = [(nh, nw, _centre(nh, 128), _centre(nw, 128)) for nh, nw in sizes]
    packed, rec = ops.pack_resize_batch(images, place)
    assert rec[1, 0] % 2 == 1 and rec[2, 0] % 2 == 1                              # the second and third image start at odd offsets
    got, want = _run(images, sizes, (128, 128))
    assert np.array_equal(got, want)
    # the already-uploaded form, into a canvas that itself starts at an odd address
    flat = torch.full((3 * 128 * 128 * 3 + 1,), 0xAA, dtype=torch.uint8, device="cuda:0")
    out = flat[1:].view(3, 128, 128, 3)
    assert out.data_ptr() % 2 == 1
    ops.resize_pad_packed(torch.from_numpy(packed).to("cuda:0"), rec, out=out)
    assert np.array_equal(out.cpu().numpy(), want) and int(flat[0]) == 0xAA


@pytest.mark.gpu
def test_the_committed_sample_images_hash_to_the_fixture(gpu, repo_root):
    from image_captioning_amd import ops, utils
    golden = os.path.join(repo_root, "tests", "golden")
    rows = json.load(open(os.path.join(golden, "sample_images.json")))
    names = sorted(rows)
    images = [utils.imread(os.path.join(golden, "sample_images", n)) for n in names]
    for n, im in zip(names, images):
        assert hashlib.sha1(np.ascontiguousarray(im).tobytes()).hexdigest() == rows[n]["sha1"], n        # the decode the fixture was made from
    out = ops.resize_pad_images(images, 800, 1024).cpu().numpy()                   # the six in ONE call
    assert out.shape == (6, 1024, 1024, 3)
    for b, n in enumerate(names):
        assert hashlib.sha1(out[b].tobytes()).hexdigest() == rows[n]["resized_sha1"], n


@pytest.mark.gpu
def test_entry_point_refusals_launch_nothing(gpu):
    from image_captioning_amd import _lib, ops
    lib = _lib.load()
    img = _noise(4, 10, 12)
    out = torch.full((1, 32, 32, 3), 0xAA, dtype=torch.uint8, device="cuda:0")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(place, null=None):
        packed, rec = ops.pack_resize_batch([img], [place])
        dev = torch.from_numpy(packed).to("cuda:0")
        d = _lib.ResizePadDesc()
        d.B, d.packed, d.packed_bytes, d.records, d.out, d.H, d.W = 1, dev.data_ptr(), dev.numel(), rec.ctypes.data, out.data_ptr(), 32, 32
        if null in ("packed", "records", "out"):
            setattr(d, null, None)
        rc = lib.dc_resize_pad_u8(C.byref(d), None if null == "workspace" else C.c_void_p(ws.data_ptr()), ws.numel(), stream)
        return rc, lib.dc_resize_pad_u8_workspace_bytes(C.byref(d))

    EINVAL, EWORKSPACE = -1, -3
    assert call((20, 24, 6, 4)) == (0, 10 * 24 * 3 + (24 * 5 + 20 * 5) * 4)    # the legal call (workspace: the intermediate, then two tables of 2 + 3 ints per index)
    out.fill_(0xAA)
    for place in ((20, 24, 13, 4), (20, 24, 6, 9), (20, 24, -1, 4), (20, 24, 6, -1), (33, 24, 0, 4)):     # a window outside the canvas
        assert call(place) == (EINVAL, 0), place
    for place in ((0, 24, 6, 4), (20, 0, 6, 4)):                                   # a zero size
        assert call(place) == (EINVAL, 0), place
    for null in ("packed", "records", "out"):
        assert call((20, 24, 6, 4), null) == (EINVAL, 0), null
    assert call((20, 24, 6, 4), "workspace")[0] == EWORKSPACE
    with pytest.raises(_lib.DcapError, match="leaves the 32 x 32 canvas"):
        ops.resize_pad_images([img], placements=[(20, 24, 13, 4)], out=out)
    torch.cuda.synchronize()
    assert bool((out == 0xAA).all())


# ---------------------------------------------------------------------------------------------- the models
MIN_DIM, MAX_DIM = 192, 256


def _joint(images_per_gpu, V=1000, T=5, proposals=300, max_instances=50):
    """The small joint model of tests/test_gpu_refine_generations.py, with a min / max side that makes the resize do work."""
    from image_captioning_amd import synth
    from image_captioning_amd.config import Config
    from image_captioning_amd.dense_model import DenseImageCapRCNN

    class Cfg(Config):
        NAME = "joint"
        IMAGES_PER_GPU = images_per_gpu
        IMAGE_MIN_DIM = MIN_DIM
        IMAGE_MAX_DIM = MAX_DIM
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
    return model


def _same(host, device):
    assert len(host) == len(device)
    for h, d in zip(host, device):
        assert sorted(h) == sorted(d)
        for key in h:
            assert h[key].dtype == d[key].dtype and h[key].shape == d[key].shape, key
            assert np.array_equal(h[key].view(np.int32), d[key].view(np.int32)), key


def _no_host_resample(monkeypatch):
    from image_captioning_amd import utils

    def refuse(*a, **k):
        raise AssertionError("mold='device' resampled on the host")
    monkeypatch.setattr(utils, "imresize", refuse)


# batch of one: 150 x 200 -> 192 x 256 (up); batch of two: 100 x 150 -> 171 x 256 (up, an odd height) and 300 x 400 -> 192 x 256 (down)
BATCHES = {1: [(150, 200)], 2: [(100, 150), (300, 400)]}


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2])
def test_generate_captions_device_mold_equals_host_mold(gpu, monkeypatch, batch):
    from image_captioning_amd import utils
    model = _joint(batch)
    images = [_noise(10 + i, h, w) for i, (h, w) in enumerate(BATCHES[batch])]
    assert [utils.resize_geometry(im.shape, MIN_DIM, MAX_DIM, True)[:2] for im in images] == {1: [(192, 256)], 2: [(171, 256), (192, 256)]}[batch]
    for postprocess in ("host", "device"):
        kw = dict(return_probabilities=False, decoder="incremental", postprocess=postprocess)
        host = model.generate_captions(images, **kw)
        want_images = model.plan().images.cpu().numpy()
        with monkeypatch.context() as m:
            _no_host_resample(m)
            device = model.generate_captions(images, mold="device", **kw)
        assert np.array_equal(model.plan().images.cpu().numpy(), want_images)
        assert all(len(r["rois"]) > 0 for r in host) and sorted(host[0]) == ["ids", "rois"]
        _same(host, device)


@pytest.mark.gpu
def test_feature_model_device_mold_equals_host_mold(gpu, monkeypatch):
    from image_captioning_amd import generate_one_roi_features, generate_roi_features, synth
    from image_captioning_amd.config import Config
    from image_captioning_amd.modified_dense_model import DenseImageCapRCNN

    class Cfg(Config):
        NAME = "features"
        IMAGES_PER_GPU = 2
        IMAGE_MIN_DIM = MIN_DIM
        IMAGE_MAX_DIM = MAX_DIM
    model = DenseImageCapRCNN("inference", Cfg(), "logs", stage4_blocks=1)
    model.set_weights(synth.encoder_weights(0, 1))
    images = [_noise(20 + i, h, w) for i, (h, w) in enumerate(BATCHES[2])]
    rois = synth.rois(5, 2, 6, MAX_DIM, MAX_DIM, lo=16, hi=MAX_DIM)
    host = model.generate_captions(images, rois, device_features=True)
    with monkeypatch.context() as m:
        _no_host_resample(m)
        device = model.generate_captions(images, rois, mold="device", device_features=True)
    for h, d in zip(host, device):
        assert d["features"].is_cuda and d["features"].shape == (6, 7, 7, 256) and torch.equal(h["features"], d["features"])
    assert float(host[0]["features"].abs().max()) > 0 and not torch.equal(host[0]["features"], host[1]["features"])

    # the façades: one image per call, through a batch-of-one model
    class Cfg1(Cfg):
        IMAGES_PER_GPU = 1
    one = DenseImageCapRCNN("inference", Cfg1(), "logs", stage4_blocks=1)
    one.set_weights(synth.encoder_weights(0, 1))

    class DS(object):
        def load_image(self, i):
            return images[i]

        def load_captions_and_rois(self, i):
            return rois[i], None
    for fn in (generate_one_roi_features.generate_features, generate_one_roi_features.generate_image_level_features):
        want = fn(DS(), 1, one)
        with monkeypatch.context() as m:
            _no_host_resample(m)
            got = fn(DS(), 1, one, mold="device")
        assert want.dtype == got.dtype == np.float32 and np.array_equal(want.view(np.int32), got.view(np.int32))
    rpn = DenseImageCapRCNN("inference", Cfg1(), "logs", stage4_blocks=1, use_generated_rois=True)
    rpn.set_weights(dict(synth.encoder_weights(0, 1), **synth.rpn_weights(4)))
    want = generate_roi_features.generate_features(images[0], rpn)
    with monkeypatch.context() as m:
        _no_host_resample(m)
        got = generate_roi_features.generate_features(images[0], rpn, mold="device")
    assert want.shape == (7 * 7 * 256,) and np.array_equal(want.view(np.int32), got.view(np.int32))


@pytest.mark.gpu
def test_train_on_dataset_device_mold_gives_the_same_logs(gpu, monkeypatch):
    from image_captioning_amd import synth
    from image_captioning_amd.config import Config
    from image_captioning_amd.modified_dense_model import DenseImageCapRCNN
    from image_captioning_amd.text_generation_model_v2 import DenseCapConfig, VisualGenomeDataset, build_model, Adam, train_on_dataset
    S, V, Rn, L, k = 128, 40, 4, 3, 2

    class FCfg(Config):
        NAME = "toy"
        IMAGES_PER_GPU = 1
        IMAGE_MIN_DIM = 96
        IMAGE_MAX_DIM = S
    feats = DenseImageCapRCNN("inference", FCfg(), "logs", stage4_blocks=1)
    feats.set_weights(synth.encoder_weights(0, 1))
    w2i = {"<unk>": 0, "<start>": 1, "<end>": 2}
    w2i.update({"w%d" % i: i for i in range(3, V)})
    ds = VisualGenomeDataset(w2i, L + 2)
    rng = np.random.RandomState(5)
    for i, (h, w) in enumerate([(70, 100), (200, 150), (200, 150), (70, 100)]):          # 70 x 100 -> 90 x 128 (up), 200 x 150 -> 128 x 96 (down)
        y, x = rng.randint(0, S - 40, Rn), rng.randint(0, S - 40, Rn)
        rois = [[int(a), int(b), int(a + rng.randint(24, 40)), int(b + rng.randint(24, 40))] for a, b in zip(y, x)]
        caps = [[" ".join("w%d" % rng.randint(3, V) for _ in range(L))] for _ in range(Rn)]
        ds.add_image("VisualGenome", image_id=1000 + i, path="none", width=w, height=h, rois=rois, captions=caps, pixels=_noise(30 + i, h, w))
    ds.prepare()
    cfg = DenseCapConfig(V, synth.embedding_matrix(3, V))
    cfg.PADDING_SIZE = L + 2

    def run(**kw):
        m = build_model((7, 7, 256), (cfg.PADDING_SIZE,), cfg, 256, inject=True, seed=7)
        m.compile(optimizer=Adam(amsgrad=True), loss="categorical_crossentropy")
        logs = train_on_dataset(m, feats, ds, images_per_step=k, rois_per_image=Rn, epochs=1, steps_per_epoch=2, verbose=0, **kw)
        return logs, m.get_weights_dict()
    host, w_host = run()
    with monkeypatch.context() as m:
        _no_host_resample(m)
        device, w_device = run(mold="device")
    assert len(host) == 1 and np.isfinite(host[0]["loss"]) and host == device
    assert all(np.array_equal(w_host[n], w_device[n]) for n in w_host)
