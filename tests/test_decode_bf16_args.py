"""The argument rules of vocab_math= (CaptionModelV1.check_decoder, generate, the joint model's generate_captions) and of bf16 operands in
ops.vocab_top1 / ops.vocab_topk: no GPU needed."""
import numpy as np
import pytest
import torch


def test_check_decoder_vocab_math_rules():
    from image_captioning_amd.text_generation_model import CaptionModelV1
    for vm in (None, "f32"):                                   # accepted wherever the decoder is, whatever the model computes in
        CaptionModelV1.check_decoder("prefix", None, vm)
        CaptionModelV1.check_decoder("prefix", True, vm, "f32")
        CaptionModelV1.check_decoder("incremental", False, vm)
        CaptionModelV1.check_decoder("incremental", False, vm, "bf16")
    CaptionModelV1.check_decoder("incremental", False, "bf16", "bf16")
    CaptionModelV1.check_decoder("incremental", False)         # the two-argument form of earlier callers
    with pytest.raises(ValueError, match="vocab_math"):
        CaptionModelV1.check_decoder("incremental", False, "fp16", "bf16")
    with pytest.raises(ValueError, match="vocab_math"):
        CaptionModelV1.check_decoder("prefix", False, "bf16", "bf16")
    with pytest.raises(ValueError, match="vocab_math"):
        CaptionModelV1.check_decoder("prefix", None, "bf16", "bf16")
    with pytest.raises(ValueError, match="vocab_math.*compute_dtype"):
        CaptionModelV1.check_decoder("incremental", False, "bf16", "f32")
    with pytest.raises(ValueError, match="vocab_math.*compute_dtype"):
        CaptionModelV1.check_decoder("incremental", False, "bf16")
    with pytest.raises(ValueError, match="return_probabilities=False"):      # the earlier rules come first
        CaptionModelV1.check_decoder("incremental", True, "bf16", "bf16")
    with pytest.raises(ValueError, match="decoder"):
        CaptionModelV1.check_decoder("beam", False, "bf16", "bf16")


@pytest.mark.parametrize("dtype", ["f32", None])
def test_models_refuse_the_bf16_vocabulary_before_touching_the_device(dtype):
    from image_captioning_amd.text_generation_model import CaptionModelV1
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    stub, joint = object.__new__(CaptionModelV1), object.__new__(DenseImageCapRCNN)
    if dtype is not None:
        stub.compute_dtype = joint.compute_dtype = dtype
    feat, img = np.zeros((2, 7, 7, 256), np.float32), [np.zeros((8, 8, 3), np.uint8)]
    with pytest.raises(ValueError, match="vocab_math.*compute_dtype"):
        CaptionModelV1.generate(stub, feat, return_probabilities=False, decoder="incremental", vocab_math="bf16")
    with pytest.raises(ValueError, match="vocab_math.*compute_dtype"):
        DenseImageCapRCNN.generate_captions(joint, img, return_probabilities=False, decoder="incremental", vocab_math="bf16")
    if dtype is not None:
        with pytest.raises(ValueError, match="vocab_math.*compute_dtype"):
            CaptionModelV1.decode_greedy(stub, feat, vocab_math="bf16")
    stub.compute_dtype = joint.compute_dtype = "bf16"
    with pytest.raises(ValueError, match="vocab_math"):
        CaptionModelV1.generate(stub, feat, return_probabilities=False, decoder="prefix", vocab_math="bf16")
    with pytest.raises(ValueError, match="vocab_math"):
        DenseImageCapRCNN.generate_captions(joint, img, return_probabilities=False, decoder="prefix", vocab_math="bf16")
    with pytest.raises(ValueError, match="vocab_math"):
        CaptionModelV1.generate(stub, feat, return_probabilities=False, decoder="incremental", vocab_math="bfloat16")
    with pytest.raises(ValueError, match="vocab_math"):
        CaptionModelV1.decode_greedy(stub, feat, vocab_math="half")


def test_bf16_vocab_ops_refuse_cpu_tensors():
    from image_captioning_amd import ops, _lib
    X, W, b = torch.zeros(4, 32, dtype=torch.bfloat16), torch.zeros(32, 8, dtype=torch.bfloat16), torch.zeros(8)
    with pytest.raises(_lib.DcapError):
        ops.vocab_top1(X, W, b)
    with pytest.raises(_lib.DcapError):
        ops.vocab_topk(X, W, b, 3)
    with pytest.raises(_lib.DcapError):
        ops.vocab_top1(X, W, b, tile=256)


def test_the_abi_declares_the_bf16_vocabulary_entry_points():
    from image_captioning_amd import _lib
    for name in ("dc_vocab_top1_bf16", "dc_vocab_topk_bf16", "dc_vocab_top1_bf16_workspace_bytes", "dc_vocab_topk_bf16_workspace_bytes",
                 "dc_vocab_topk_bf16_tile"):
        assert name in _lib.SYMBOLS
    assert _lib.VocabTop1Bf16Desc._fields_[:-1] == _lib.VocabTop1Desc._fields_ and _lib.VocabTop1Bf16Desc._fields_[-1][0] == "tile"
    assert _lib.VocabTopkBf16Desc._fields_[:-1] == _lib.VocabTopkDesc._fields_ and _lib.VocabTopkBf16Desc._fields_[-1][0] == "tile"


def test_tile_choice_and_workspace_queries_launch_nothing():
    """dc_vocab_topk_bf16_tile and the workspace queries answer on a machine without a GPU; the 256-column tile keeps a cell per 64-column
    wave slice, the 128-column tile one per tile."""
    from image_captioning_amd import ops, _lib
    lib = _lib.load()
    assert ops.vocab_topk_bf16_tile(3000, 50000, 1024) == 256 and ops.vocab_topk_bf16_tile(1, 24, 256) == 128
    assert lib.dc_vocab_topk_bf16_tile(0, 10, 8) == 0
    for k in (1, 8):
        assert lib.dc_vocab_topk_bf16_workspace_bytes(1000, 50000, 1024, k, 128) == (1000 * 391 * (k + 1) * 8 + 255) // 256 * 256
        assert lib.dc_vocab_topk_bf16_workspace_bytes(1000, 50000, 1024, k, 256) == (1000 * 782 * (k + 1) * 8 + 255) // 256 * 256
    assert lib.dc_vocab_topk_bf16_workspace_bytes(1000, 50000, 1024, 1, 64) == 0
    assert lib.dc_vocab_top1_bf16_workspace_bytes(37, 1001, 256, 0) == lib.dc_vocab_topk_bf16_workspace_bytes(37, 1001, 256, 1, 0)
