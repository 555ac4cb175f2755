"""Mask R-CNN's host side (no GPU): what the model refuses, the configuration, the head's stored and Keras shapes, the ops wrappers'
refusals on CPU tensors (checked before the library is loaded) and an HDF5 round trip of the new layers."""
import numpy as np
import pytest
import torch


def _cfg(num_classes=9, **over):
    from image_captioning_amd.mask_rcnn_model import MaskRCNNConfig

    class Cfg(MaskRCNNConfig):
        IMAGES_PER_GPU = 1
        IMAGE_MIN_DIM = 128
        IMAGE_MAX_DIM = 128
    for k, v in over.items():
        setattr(Cfg, k, v)
    return Cfg(num_classes)


def test_config():
    from image_captioning_amd.config import Config
    from image_captioning_amd.mask_rcnn_model import MaskRCNNConfig
    cfg = MaskRCNNConfig()
    assert (cfg.NAME, cfg.NUM_CLASSES, cfg.USE_MINI_MASK, cfg.MINI_MASK_SHAPE) == ("mask_rcnn", 1, True, (56, 56))
    assert MaskRCNNConfig(81).NUM_CLASSES == 81 and not hasattr(Config, "NUM_CLASSES")
    assert (cfg.MASK_POOL_SIZE, cfg.MASK_SHAPE, cfg.DETECTION_MIN_CONFIDENCE, cfg.DETECTION_MAX_INSTANCES) == (14, [28, 28], 0.7, 100)


def test_refusals_by_name():
    from image_captioning_amd.mask_rcnn_model import MaskRCNN
    with pytest.raises(ValueError, match='mode="training"'):
        MaskRCNN("training", _cfg(), "logs")
    with pytest.raises(ValueError, match="bf16"):
        MaskRCNN("inference", _cfg(), "logs", compute_dtype="bf16")
    with pytest.raises(ValueError, match="GPU_COUNT"):
        MaskRCNN("inference", _cfg(GPU_COUNT=2), "logs")
    with pytest.raises(ValueError, match="NUM_CLASSES"):
        MaskRCNN("inference", _cfg(1), "logs")
    stub = object.__new__(MaskRCNN)                                      # the refusals below read no model state
    with pytest.raises(ValueError, match="MaskRCNN.train: training is not built"):
        stub.train(None, None, 0.001, 1, "all")
    with pytest.raises(ValueError, match="MaskRCNN.compile: training is not built"):
        stub.compile(0.001)
    with pytest.raises(ValueError, match="MaskRCNN.train_on_batch: training is not built"):
        stub.train_on_batch([])
    with pytest.raises(ValueError, match="no caption decoder: use detect"):
        stub.generate_captions([])
    for name, call in (("test_on_batch", lambda: stub.test_on_batch([])), ("test_on_batch_device", lambda: stub.test_on_batch_device([])),
                       ("train_on_batch_device", lambda: stub.train_on_batch_device([])), ("forward_backward", lambda: stub.forward_backward([])),
                       ("set_trainable", lambda: stub.set_trainable(".*")), ("plan_pair", lambda: stub.plan_pair())):
        with pytest.raises(ValueError, match="MaskRCNN.%s: training is not built" % name):
            call()
    with pytest.raises(ValueError, match="step graph"):
        stub.use_step_graph = True
    stub.use_step_graph = False
    assert stub.use_step_graph is False
    with pytest.raises(ValueError, match="ParallelModel"):
        stub.grad_sync = lambda g: 1.0
    stub.grad_sync = None
    assert stub.grad_sync is None
    stub.config = _cfg()
    with pytest.raises(ValueError, match="postprocess"):
        stub.detect([], postprocess="gpu")
    with pytest.raises(ValueError, match="device_masks"):
        stub.detect([], device_masks=True)


@pytest.mark.parametrize("C", [2, 81])
def test_num_classes_2_and_81_are_accepted_and_keep_keras_shapes(C):
    from image_captioning_amd import synth
    from image_captioning_amd.mask_rcnn_model import DetectTop
    top = DetectTop([7, 7, 256], C, "cpu")
    w = top.store.w
    Cp = (C + 3) // 4 * 4
    assert tuple(w["mrcnn_class_logits/kernel"].shape) == (1024, Cp) and tuple(w["mrcnn_bbox_fc/kernel"].shape) == (1024, 4 * C)
    assert tuple(w["mrcnn_mask/kernel"].shape) == (C, 256) and tuple(w["mrcnn_mask_conv3/kernel"].shape) == (256, 2304)
    assert float(w["mrcnn_class_logits/kernel"][:, C:].abs().max() if Cp > C else 0.0) == 0.0
    W = synth.detect_head_weights(6, C)                                  # the generator the store was filled from
    assert W["mrcnn_class_logits/kernel"].shape == (1024, C) and W["mrcnn_bbox_fc/bias"].shape == (4 * C,)
    assert W["mrcnn_mask_deconv/kernel"].shape == (2, 2, 256, 256) and W["mrcnn_mask/kernel"].shape == (1, 1, 256, C)
    assert set(W) == {k for k in w if k.split("/")[0] in ("mrcnn_class_logits", "mrcnn_bbox_fc", "mrcnn_mask_deconv", "mrcnn_mask")
                      or k.startswith(("mrcnn_mask_conv", "mrcnn_mask_bn"))}
    for k, v in W.items():                                               # stored -> Keras' shapes, bit for bit
        back = top.from_stored(k, w[k].numpy())
        assert back.shape == v.shape and np.array_equal(back, v), k
    with pytest.raises(ValueError, match="shape mismatch for mrcnn_class_logits/kernel"):
        top.to_stored({"mrcnn_class_logits/kernel": np.zeros((1024, C + 1), np.float32)})
    with pytest.raises(ValueError, match="at least 2"):
        DetectTop([7, 7, 256], 1, "cpu")


def test_pack_mask_tail():
    from image_captioning_amd.packing import pack_mask_tail
    k = np.arange(2 * 3, dtype=np.float32).reshape(1, 1, 2, 3)
    assert np.array_equal(pack_mask_tail(k), [[0, 3], [1, 4], [2, 5]]) and pack_mask_tail(k).flags["C_CONTIGUOUS"]
    assert np.array_equal(pack_mask_tail(k[0, 0]), pack_mask_tail(k))


# ---- the wrappers' refusals (everything here is refused before the library is loaded) ------------------------------------------------
def _no_library(monkeypatch):
    from image_captioning_amd import _lib

    def boom():
        raise AssertionError("the wrapper loaded the library before refusing")
    monkeypatch.setattr(_lib, "load", boom)
    return _lib.DcapError


def test_class_select_refusals(monkeypatch):
    from image_captioning_amd import ops
    E = _no_library(monkeypatch)
    z, d = torch.zeros(5, 9), torch.zeros(5, 36)
    for bad_z, bad_d, what in ((torch.zeros(5), d, "logits must be"), (torch.zeros(5, 1), torch.zeros(5, 4), "C >= 2"), (torch.zeros(0, 9), d, "R >= 1"),
                               (z, torch.zeros(5, 35), "deltas must be"), (z, torch.zeros(4, 36), "deltas must be"),
                               (z, torch.zeros(5, 9, 4)[:, :, ::1].transpose(0, 1).contiguous().transpose(0, 1), "3-D deltas"),
                               (z.double(), d, "logits must be torch.float32"), (z, d.half(), "deltas must be torch.float32"),
                               (torch.zeros(5, 18)[:, ::2], d, "contiguous along its rows"), (torch.zeros(9, 5).t(), d, "contiguous along its rows")):
        with pytest.raises(E, match=what):
            ops.class_select(bad_z, bad_d)
    for kw, what in ((dict(class_ids=torch.zeros(5, dtype=torch.int64)), "class_ids must be"), (dict(scores=torch.zeros(4)), "scores must be"),
                     (dict(deltas_out=torch.zeros(5, 8)[:, ::2]), "deltas_out must be")):
        with pytest.raises(E, match=what):
            ops.class_select(z, d, **kw)


def test_mask_head_tail_refusals(monkeypatch):
    from image_captioning_amd import ops
    E = _no_library(monkeypatch)
    N, P, Cin, Cmid, C = 2, 14, 64, 32, 5
    good = dict(x=torch.zeros(N, P, P, Cin), wd=torch.zeros(2, 2, Cmid, Cin), bd=torch.zeros(Cmid), wm_t=torch.zeros(C, Cmid), bm=torch.zeros(C),
                class_ids=torch.zeros(N, dtype=torch.int32))
    for key, bad, what in (("x", torch.zeros(N, P, P + 1, Cin), "x must be"), ("x", torch.zeros(N, 17, 17, Cin), "P in 1..16"),
                           ("x", torch.zeros(N, P, P, 48), "Cin must be a multiple of 32"), ("x", torch.zeros(N, P, P, 288), "Cin must be a multiple of 32"),
                           ("wd", torch.zeros(2, 2, 40, Cin), "Cmid a multiple of 32"), ("wd", torch.zeros(2, 2, Cmid, 32), "wd must be"),
                           ("wd", torch.zeros(4, Cmid, Cin), "wd must be"), ("wm_t", torch.zeros(Cmid, C), "wm_t must be"),
                           ("bd", torch.zeros(Cmid + 1), "bd must be a contiguous"), ("bm", torch.zeros(C).double(), "bm must be torch.float32"),
                           ("class_ids", torch.zeros(N, dtype=torch.int64), "class_ids must be torch.int32"),
                           ("class_ids", torch.zeros(N + 1, dtype=torch.int32), "class_ids must be a contiguous"),
                           ("x", torch.zeros(N, P, P, 2 * Cin)[..., ::2], "x must be a contiguous")):
        with pytest.raises(E, match=what):
            ops.mask_head_tail(**dict(good, **{key: bad}))
    with pytest.raises(E, match="out must be"):
        ops.mask_head_tail(out=torch.zeros(N, 2 * P, 2 * P + 1), **good)


def test_mask_paste_refusals(monkeypatch):
    from image_captioning_amd import ops
    E = _no_library(monkeypatch)
    m, b = torch.zeros(3, 28, 28), torch.zeros(3, 4, dtype=torch.int32)
    for bad_m, bad_b, H, W, what in ((torch.zeros(3, 65, 28), b, 97, 131, "h, w in 1..64"), (torch.zeros(28, 28), b, 97, 131, "masks must be"),
                                     (m, b, 0, 131, "at least 1 x 1"), (m, b, 1 << 16, 1 << 15, "below 2\\^31"), (m.double(), b, 97, 131, "masks must be torch.float32"),
                                     (m, b.long(), 97, 131, "boxes must be torch.int32"), (m, torch.zeros(2, 4, dtype=torch.int32), 97, 131, "boxes must be a contiguous"),
                                     (torch.zeros(3, 28, 56)[:, :, ::2], b, 97, 131, "masks must be a contiguous")):
        with pytest.raises(E, match=what):
            ops.mask_paste(bad_m, bad_b, H, W)
    with pytest.raises(E, match="out must be torch.uint8"):
        ops.mask_paste(m, b, 97, 131, out=torch.zeros(3, 97, 131))


def test_cpu_tensors_are_refused_after_the_shape_checks_and_before_the_library(monkeypatch):
    from image_captioning_amd import ops
    E = _no_library(monkeypatch)
    with pytest.raises(E, match="class_select: logits must live on the GPU"):
        ops.class_select(torch.zeros(5, 9), torch.zeros(5, 36))
    with pytest.raises(E, match="mask_head_tail: x must live on the GPU"):
        ops.mask_head_tail(torch.zeros(2, 14, 14, 64), torch.zeros(2, 2, 32, 64), torch.zeros(32), torch.zeros(5, 32), torch.zeros(5),
                           torch.zeros(2, dtype=torch.int32))
    with pytest.raises(E, match="mask_paste: masks must live on the GPU"):
        ops.mask_paste(torch.zeros(3, 28, 28), torch.zeros(3, 4, dtype=torch.int32), 97, 131)


# ---- weight files -------------------------------------------------------------------------------------------------------------------
def test_hdf5_round_trip_of_the_new_layers(tmp_path):
    """A Keras-layout file of the detection heads written and read by hdf5_lite: the keys, shapes and bits survive, also when the
    layers sit in the nested groups TimeDistributed writes (/<wrapper>/<wrapper>/<inner name>/<weight>:0 reads back by the inner name)."""
    from image_captioning_amd import hdf5_lite, synth
    W = synth.detect_head_weights(3, 9)
    W.update(synth.head_weights(1))
    path = str(tmp_path / "heads.h5")
    hdf5_lite.save_keras_weights(path, W)
    back = hdf5_lite.load_keras_weights(path)
    assert set(back) == set(W) and all(back[k].shape == W[k].shape and np.array_equal(back[k], W[k]) for k in W)
    nested = {layer: "td_" + layer for layer in {k.split("/")[0] for k in W} if layer.startswith("mrcnn_mask")}
    path2 = str(tmp_path / "heads_nested.h5")
    hdf5_lite.save_keras_weights(path2, W, layer_groups=nested)
    back2 = hdf5_lite.load_keras_weights(path2)
    assert set(back2) == set(W) and all(np.array_equal(back2[k], W[k]) for k in W)
    f = hdf5_lite.H5File(path2)
    assert "td_mrcnn_mask_deconv" in f and "mrcnn_mask_deconv" not in f
