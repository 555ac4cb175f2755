"""The argument rules of generate_captions(postprocess=) (CaptionModelV1.check_decoder) and of ops.refine_generations, and the
declarations the device post-processing adds: no GPU needed."""
import inspect
import os

import pytest
import torch


def _check(**kw):
    from image_captioning_amd.text_generation_model import CaptionModelV1
    args = dict(decoder="incremental", return_probabilities=False)
    args.update(kw)
    return CaptionModelV1.check_decoder(args.pop("decoder"), args.pop("return_probabilities"), **args)


def test_host_is_the_default():
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    from image_captioning_amd.text_generation_model import CaptionModelV1
    assert inspect.signature(DenseImageCapRCNN.generate_captions).parameters["postprocess"].default == "host"
    assert inspect.signature(CaptionModelV1.check_decoder).parameters["postprocess"].default == "host"
    assert CaptionModelV1.POSTPROCESS == ("host", "device")
    _check()
    _check(decoder="prefix", return_probabilities=True)                  # today's default call stays legal
    _check(decoder="prefix", return_probabilities=True, postprocess="host")


def test_device_postprocess_is_accepted_with_the_device_decoders():
    _check(postprocess="device")
    _check(decoder="beam", beam_size=3, end_id=2, postprocess="device")
    _check(decoder="beam", beam_size=3, score="prob", postprocess="device")


def test_device_postprocess_refuses_the_prefix_decoder_and_probabilities():
    for kw in (dict(decoder="prefix", return_probabilities=True), dict(decoder="prefix", return_probabilities=False),
               dict(decoder="prefix", return_probabilities=None)):
        with pytest.raises(ValueError, match="postprocess='device'"):
            _check(postprocess="device", **kw)
    # the device decoders' own refusal of return_probabilities comes first and keeps its message
    with pytest.raises(ValueError, match="return_probabilities=False"):
        _check(return_probabilities=True, postprocess="device")


def test_unknown_postprocess_is_refused():
    for bad in ("gpu", None, "", "Device", 1):
        with pytest.raises(ValueError, match="postprocess must be one of"):
            _check(postprocess=bad)


def test_earlier_refusals_keep_their_order():
    with pytest.raises(ValueError, match="decoder must be one of"):
        _check(decoder="greedy", postprocess="nonsense")
    with pytest.raises(ValueError, match="vocab_math"):
        _check(vocab_math="fp8", postprocess="nonsense")
    with pytest.raises(ValueError, match="beam_size"):
        _check(decoder="beam", postprocess="device")


def test_refine_generations_refuses_cpu_tensors_and_bad_arguments():
    from image_captioning_amd import ops, _lib
    rois, ws, consts = torch.zeros((1, 8, 4)), torch.ones((8, 3)), torch.zeros((1, 10), dtype=torch.float64)
    with pytest.raises(_lib.DcapError, match="GPU"):
        ops.refine_generations(rois, consts, 0.3, 10, word_scores=ws)


def test_refine_generations_is_declared(repo_root):
    from image_captioning_amd import _lib
    assert "dc_refine_generations_f64" in _lib.SYMBOLS and "dc_refine_generations_workspace_bytes" in _lib.SYMBOLS
    header = open(os.path.join(repo_root, "include", "dcap.h")).read()
    assert "#define DC_REFINE_CONSTS %d" % _lib.REFINE_CONSTS in header and "#define DC_REFINE_MAX_ROIS %d" % _lib.REFINE_MAX_ROIS in header
    assert "#define DC_ABI_VERSION 600" in header and _lib.ABI_VERSION == 600
    assert _lib.REFINE_MAX_ROIS == 8192


def test_refine_constants_are_unmold_generations_own():
    import numpy as np
    from image_captioning_amd import dense_model
    import types
    cfg = types.SimpleNamespace(IMAGE_SHAPE=np.array([320, 320, 3]))
    window, shape = (40, 0, 280, 320), (300, 400, 3)
    c = dense_model.refine_constants(window, cfg, shape)
    assert c.dtype == np.float64 and c.shape == (10,)
    assert list(c[:8]) == [40, 0, 280, 320, 320, 320, 40, 0]
    assert c[8] == min(shape[0] / (window[2] - window[0]), shape[1] / (window[3] - window[1])) == 1.25
    boxes = np.array([[50, 10, 100, 200]], np.int32)
    want, _ = dense_model.unmold_generations(boxes, shape, window)
    assert np.array_equal(((boxes - c[[6, 7, 6, 7]]) * c[8]).astype(np.int32), want)
