"""The RoI tag model's host side (no GPU): what it refuses, its layer regexes and loss names, the head's initialisers, the generator's
gt_classes batches, the dataset and the tag encoding with a stub tagger."""
import re

import numpy as np
import pytest


def _cfg(num_classes=8, **over):
    from image_captioning_amd.train_roi_tags import RoiTagConfig

    class Cfg(RoiTagConfig):
        IMAGES_PER_GPU = 1
        IMAGE_MIN_DIM = 128
        IMAGE_MAX_DIM = 128
        TRAIN_ROIS_PER_IMAGE = 12
        MAX_GT_INSTANCES = 5
        RPN_TRAIN_ANCHORS_PER_IMAGE = 64
    for k, v in over.items():
        setattr(Cfg, k, v)
    return Cfg(num_classes)


def test_config_and_loss_names():
    from image_captioning_amd.roi_tag_model import ROITagRCNN
    from image_captioning_amd.train_roi_tags import RoiTagConfig
    cfg = RoiTagConfig(1000)
    assert (cfg.NAME, cfg.NUM_CLASSES, cfg.IMAGES_PER_GPU, cfg.BATCH_SIZE, cfg.LEARNING_RATE) == ("roitag_rcnn", 1000, 2, 2, 0.001)
    assert ROITagRCNN.LOSS_NAMES == ("rpn_class_loss", "rpn_bbox_loss", "roi_tag_classes_loss")


def test_layer_regexes_are_the_references_with_roitag():
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    from image_captioning_amd.roi_tag_model import ROITagRCNN
    rx = ROITagRCNN.LAYER_REGEX
    assert set(rx) == {"no_backbone", "no_rpn", "3+", "4+", "5+", "all"}
    for key in ("no_backbone", "3+", "4+", "5+", "all"):
        assert rx[key] == DenseImageCapRCNN.LAYER_REGEX[key].replace("imgcap", "roitag")
    assert rx["no_rpn"] == r"(res.*)|(bn3.*)|(roitag\_.*)|(fpn\_.*)|(mrcnn\_.*)"
    full = lambda key, name: re.fullmatch(rx[key], name) is not None
    assert full("no_backbone", "roitag_class_logits") and full("no_backbone", "mrcnn_class_bn1") and not full("no_backbone", "res5a_branch2a")
    assert full("5+", "bn5c_branch2c") and not full("5+", "res4a_branch1") and not full("no_backbone", "imgcap_lstm1")
    assert full("no_rpn", "res2a_branch2a") and not full("no_rpn", "bn2a_branch2a") and not full("no_rpn", "rpn_conv_shared")


def test_tag_head_initialisers():
    from image_captioning_amd import synth
    W = synth.tag_head_weights(3, 40)
    k, b = W["roitag_class_logits/kernel"], W["roitag_class_logits/bias"]
    assert k.shape == (1024, 40) and k.dtype == np.float32 and b.shape == (40,) and b.dtype == np.float32
    assert (b == np.float32(-np.log(99.0))).all()                       # PriorProbability(0.01): sigmoid(bias) = 0.01
    assert abs(1.0 / (1.0 + np.exp(-float(b[0]))) - 0.01) < 1e-8
    assert abs(k.std() - 0.01) < 5e-4 and abs(k.mean()) < 5e-4
    assert np.array_equal(k, synth.tag_head_weights(3, 40)["roitag_class_logits/kernel"])


def test_refusals_that_need_no_device():
    from image_captioning_amd.roi_tag_model import ROITagRCNN, TagTop
    with pytest.raises(ValueError, match="bf16"):
        ROITagRCNN("training", _cfg(), "logs", compute_dtype="bf16")
    with pytest.raises(ValueError, match="GPU_COUNT"):
        ROITagRCNN("training", _cfg(GPU_COUNT=2), "logs")
    with pytest.raises(ValueError, match="multiple of 4"):
        TagTop([7, 7, 256], 10, "cpu")
    stub = object.__new__(ROITagRCNN)                                   # the refusals below read no model state
    with pytest.raises(ValueError, match="no_rpn.*backbone_from"):
        stub.train(None, None, 0.001, 1, "no_rpn")
    with pytest.raises(ValueError, match="no_rpn"):
        stub.train(None, None, 0.001, 1, ROITagRCNN.LAYER_REGEX["no_rpn"])
    with pytest.raises(ValueError, match="JointTrainPipeline"):
        stub.plan_pair()
    with pytest.raises(ValueError, match="step graph"):
        stub.use_step_graph = True
    stub.use_step_graph = False
    assert stub.use_step_graph is False
    with pytest.raises(ValueError, match="ParallelModel"):
        stub.grad_sync = lambda g: 1.0
    stub.grad_sync = None
    with pytest.raises(ValueError, match="generate_roi_tags"):
        stub.generate_captions([])
    assert ROITagRCNN.PIPELINED_FIT is False


def test_given_positive_rows_counts_rows_with_a_tag():
    from image_captioning_amd.roi_tag_model import ROITagRCNN
    assert ROITagRCNN._given_positive_rows(np.array([[1, 0, 0], [0, 0, 0], [0, 1, 1]])) == 2      # column 0 counts, unlike a caption's <start>


# ------------------------------------------------------------------------------------------------ preprocessing and dataset
VOCAB = ["red", "car", "tall", "tree", "sky", "blue", "dog", "small"]
POS = {"red": "ADJ", "car": "NOUN", "tall": "ADJ", "tree": "NOUN", "sky": "NOUN", "blue": "ADJ", "dog": "NOUN", "small": "ADJ", "runs": "VERB",
       "the": "DET", "a": "DET", "zebra": "NOUN", "is": "VERB"}


def stub_tagger(tokens):
    return [(t, POS.get(t, "X")) for t in tokens]


def test_tag_encoding_with_a_stub_tagger():
    from image_captioning_amd import roi_tag_preprocess as P
    tag_to_id, id_to_tag = P.load_corpus(VOCAB)
    assert tag_to_id["red"] == 0 and id_to_tag[7] == "small" and len(tag_to_id) == len(id_to_tag) == 8
    assert P.encode_tag("tree", tag_to_id) == 3 and P.encode_tag("zebra", tag_to_id) == -1
    v = P.encode_region_tags("The red car is a Red car", tag_to_id, stub_tagger)
    assert v.shape == (8,) and v.tolist() == [1, 1, 0, 0, 0, 0, 0, 0]                          # lower-cased, duplicates once
    assert P.encode_region_tags("a zebra runs", tag_to_id, stub_tagger).sum() == 0               # a NOUN that is no class; a VERB
    assert P.encode_region_tags("the dog runs", tag_to_id, lambda toks: [(t, "VERB") for t in toks]).sum() == 0   # the tagger decides
    assert P.decode_tags(v, id_to_tag) == ["red", "car"]
    assert P.decode_tags(np.array([0, 0, 0.2, 0, 0, 0, 0, 0.9]), id_to_tag) == ["tall", "small"]


def _dataset(precomputed=False):
    from image_captioning_amd import roi_tag_preprocess as P
    from image_captioning_amd.train_roi_tags import VisualGenomeDataset
    tag_to_id, id_to_tag = P.load_corpus(VOCAB)
    ds = VisualGenomeDataset(tag_to_id, id_to_tag, None if precomputed else stub_tagger)
    phrases = [["the red car", "a tall tree", "a zebra runs"], ["blue sky", "small dog"], ["the dog", "red sky", "a car", "tall dog", "small tree", "blue car", "tree"]]
    for i, ph in enumerate(phrases):
        r = np.random.RandomState(i)
        y, x = r.randint(0, 60, len(ph)), r.randint(0, 60, len(ph))
        rois = np.stack([y, x, y + r.randint(8, 60, len(ph)), x + r.randint(8, 60, len(ph))], axis=1).tolist()
        extra = {}
        if precomputed:
            extra["tags"] = [P.encode_region_tags(c, tag_to_id, stub_tagger) for c in ph]
        ds.add_image("toy", image_id=i, path=None, rois=rois, captions=[[c] for c in ph],
                     pixels=r.randint(0, 255, (96, 128, 3)).astype(np.uint8), **extra)
    ds.prepare()
    return ds


@pytest.mark.parametrize("precomputed", [False, True])
def test_dataset_rows(precomputed):
    ds = _dataset(precomputed)
    rois, tags = ds.load_rois_and_tags(0)
    assert rois.shape == (3, 4) and tags.shape == (3, 8)
    assert tags.tolist() == [[1, 1, 0, 0, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0, 0, 0], [0] * 8]          # the tag-less region stays, as a zero row
    rois2, names = ds.load_original_rois_and_tags(0)
    assert np.array_equal(rois, rois2) and names == ["red, car", "tall, tree", ""]
    if precomputed:
        with pytest.raises(ValueError, match="tagger"):
            ds.encode_region_tags("red car")
    else:
        assert ds.encode_region_tags("blue dog").tolist() == [0, 0, 0, 0, 0, 1, 1, 0]


def test_precomputed_rows_of_the_wrong_width_are_refused():
    ds = _dataset(True)
    ds.image_info[1]["tags"] = [[1, 0, 0], [0, 1, 0]]
    with pytest.raises(ValueError, match="3 wide"):
        ds.load_rois_and_tags(1)


@pytest.mark.parametrize("rpn_targets", ["host", "device"])
def test_generator_batches_carry_gt_classes(rpn_targets):
    from image_captioning_amd import roi_tag_model as T
    cfg = _cfg(8, IMAGES_PER_GPU=2)
    ds = _dataset()
    gen = T.data_generator(ds, cfg, shuffle=False, augment=False, batch_size=2, rng=np.random.RandomState(0), rpn_targets=rpn_targets)
    inputs, outputs = next(gen)
    assert outputs == [] and len(inputs) == 6
    images, metas, match, bbox, gt_classes, gt_boxes = inputs
    assert images.shape == (2, 128, 128, 3) and images.dtype == np.float32
    assert gt_classes.shape == (2, 5, 8) and gt_classes.dtype == np.int32 and gt_boxes.shape == (2, 5, 4)
    for b in range(2):
        rois, tags = ds.load_rois_and_tags(b)
        n = len(rois)
        assert np.array_equal(gt_boxes[b, :n], rois) and np.array_equal(gt_classes[b, :n], tags) and not gt_classes[b, n:].any() and not gt_boxes[b, n:].any()
    if rpn_targets == "host":
        assert match.shape[0] == 2 and match.shape[2] == 1 and bbox.shape == (2, 64, 4)
    else:
        assert bbox is None and [m.shape for m in match] == [(3, 4), (2, 4)]
    inputs, _ = next(gen)                                                  # image 2 has 7 regions: MAX_GT_INSTANCES of them are picked
    assert inputs[4].shape == (2, 5, 8) and (inputs[4][0].sum(axis=1) > 0).all()


def test_the_default_loader_is_todays_generator():
    """loader=None is the keyword's default: the caption generator yields what it yielded, PADDING_SIZE wide."""
    import inspect
    from image_captioning_amd import dense_model as D
    assert inspect.signature(D.data_generator).parameters["loader"].default is None
    assert inspect.signature(D.load_image_gt).parameters["loader"].default is None
    assert D.DenseImageCapRCNN.GT_LOADER is None and D.DenseImageCapRCNN.PIPELINED_FIT is True
    assert D.DenseImageCapRCNN.LOSS_NAMES[2] == "imgcap_loss"


def test_refine_tag_generations_orders_equal_scores_like_the_device_path():
    """Non-overlapping boxes all survive the NMS, in score order; equal scores (the RoIs without a confident class share -3.4e38) in
    np.argsort(kind='stable')[::-1] order, i.e. the higher index first; DETECTION_MAX_INSTANCES cuts the list; overlapping boxes lose."""
    from image_captioning_amd.roi_tag_model import refine_tag_generations
    cfg = _cfg(8, DETECTION_MAX_INSTANCES=4)
    rois = np.array([[0.0, 0.0, 0.2, 0.2], [0.3, 0.3, 0.5, 0.5], [0.6, 0.6, 0.8, 0.8], [0.0, 0.6, 0.2, 0.8], [0.6, 0.0, 0.8, 0.2],
                     [0.61, 0.01, 0.8, 0.2]], np.float32)
    none = np.float32(-3.4e38)
    scores = np.array([none, -0.5, none, -0.25, none, -0.1], np.float32)
    boxes, keep = refine_tag_generations(rois, scores, (0, 0, 128, 128), cfg)
    assert keep.tolist() == [5, 3, 1, 2]                                  # box 4 overlaps box 5; then the ties 2, 0 from the top index down
    assert boxes.dtype == np.int32 and boxes[0].tolist() == [78, 1, 102, 26]
    boxes, keep = refine_tag_generations(rois, scores, (0, 0, 96, 128), cfg)   # a window shorter than the image: clipped, then rounded
    assert boxes[keep.tolist().index(2)].tolist() == [77, 77, 96, 102]
