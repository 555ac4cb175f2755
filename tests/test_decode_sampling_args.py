"""The argument rules of decoder='sampling' (check_decoder of both caption models, generate, decode_sampling, the joint model's
generate_captions) and of ops.vocab_sample, the declarations of its entry points, and the sampler's specification itself (the float64
restatement of tests/_sampling_ref.py follows the Gumbel-max identity): no GPU needed."""
import os

import numpy as np
import pytest
import torch

import _sampling_ref as S

BAD_SEEDS = (None, True, -1, 2 ** 32, 2.5)
BAD_TEMPERATURES = (0, 0.0, -1.0, float("nan"), float("inf"), "1.0", True)
BAD_TOP_K = (0, 9, True, 2.5)


def test_v1_check_decoder_sampling_rules():
    from image_captioning_amd.text_generation_model import CaptionModelV1
    assert "sampling" in CaptionModelV1.DECODERS
    assert CaptionModelV1.check_decoder("sampling", False, seed=0) == (1.0, None, 0)
    assert CaptionModelV1.check_decoder("sampling", False, seed=np.int64(2 ** 32 - 1), temperature=0.5, top_k=np.int32(8)) == (0.5, 8, 2 ** 32 - 1)
    assert CaptionModelV1.check_decoder("sampling", False, None, None, None, "logprob", None, "device", 2, 1, 7) == (2.0, 1, 7)
    assert CaptionModelV1.check_decoder("incremental", False) is None
    for s in BAD_SEEDS:
        with pytest.raises(ValueError, match="decoder='sampling' needs seed"):
            CaptionModelV1.check_decoder("sampling", False, seed=s)
    for t in BAD_TEMPERATURES:
        with pytest.raises(ValueError, match="temperature"):
            CaptionModelV1.check_decoder("sampling", False, seed=1, temperature=t)
    for k in BAD_TOP_K:
        with pytest.raises(ValueError, match="top_k"):
            CaptionModelV1.check_decoder("sampling", False, seed=1, top_k=k)
    for rp in (True, None):
        with pytest.raises(ValueError, match="decoder='sampling' returns no word probabilities: pass return_probabilities=False"):
            CaptionModelV1.check_decoder("sampling", rp, seed=1)
    with pytest.raises(ValueError, match="decoder='beam'"):                     # beam_size and end_id stay beam-only
        CaptionModelV1.check_decoder("sampling", False, beam_size=3, seed=1)
    with pytest.raises(ValueError, match="decoder='beam'"):
        CaptionModelV1.check_decoder("sampling", False, end_id=2, seed=1)
    CaptionModelV1.check_decoder("sampling", False, "bf16", "bf16", seed=1)     # vocab_math: the rule of 'incremental'
    with pytest.raises(ValueError, match="vocab_math.*compute_dtype"):
        CaptionModelV1.check_decoder("sampling", False, "bf16", "f32", seed=1)
    CaptionModelV1.check_decoder("sampling", False, postprocess="device", seed=1)
    with pytest.raises(ValueError, match="postprocess must be one of"):         # every earlier refusal comes before the sampling ones
        CaptionModelV1.check_decoder("sampling", False, postprocess="gpu")
    with pytest.raises(ValueError, match="vocab_math"):
        CaptionModelV1.check_decoder("sampling", False, "fp16", seed=None)
    with pytest.raises(ValueError, match="decoder must be one of"):
        CaptionModelV1.check_decoder("sample", False, seed=1)


def test_sampling_arguments_are_refused_with_the_other_decoders():
    from image_captioning_amd.text_generation_model import CaptionModelV1
    from image_captioning_amd.text_generation_model_v2 import CaptionModelV2
    for kw in (dict(seed=1), dict(temperature=0.7), dict(top_k=3), dict(seed=1, temperature=1.0, top_k=2)):
        for dec, more in (("prefix", dict()), ("incremental", dict()), ("beam", dict(beam_size=3))):
            with pytest.raises(ValueError, match="only for decoder='sampling'"):
                CaptionModelV1.check_decoder(dec, None if dec == "prefix" else False, **more, **kw)
            with pytest.raises(ValueError, match="only for decoder='sampling'"):
                CaptionModelV2.check_decoder(dec, **more, **kw)


def test_v2_check_decoder_sampling_rules():
    from image_captioning_amd.text_generation_model_v2 import CaptionModelV2
    assert CaptionModelV2.check_decoder("sampling", seed=3) == (1.0, None, 3)
    assert CaptionModelV2.check_decoder("sampling", None, [1, 2], "prob", 0.25, 5, 9) == (0.25, 5, 9)
    assert CaptionModelV2.check_decoder("incremental") is None
    for s in BAD_SEEDS:
        with pytest.raises(ValueError, match="decoder='sampling' needs seed"):
            CaptionModelV2.check_decoder("sampling", seed=s)
    for t in BAD_TEMPERATURES:
        with pytest.raises(ValueError, match="temperature"):
            CaptionModelV2.check_decoder("sampling", seed=1, temperature=t)
    for k in BAD_TOP_K:
        with pytest.raises(ValueError, match="top_k"):
            CaptionModelV2.check_decoder("sampling", seed=1, top_k=k)
    with pytest.raises(ValueError, match="decoder='beam'"):
        CaptionModelV2.check_decoder("sampling", beam_size=2, seed=1)
    with pytest.raises(ValueError, match="decoder must be one of"):
        CaptionModelV2.check_decoder("sample", seed=1)


BAD = ([dict()] + [dict(seed=s) for s in BAD_SEEDS[1:]] + [dict(seed=1, temperature=t) for t in BAD_TEMPERATURES] +
       [dict(seed=1, top_k=k) for k in BAD_TOP_K])


@pytest.mark.parametrize("kw", BAD, ids=[",".join("%s=%r" % i for i in kw.items()) or "no seed" for kw in BAD])
def test_models_refuse_bad_sampling_arguments_before_touching_the_device(kw):
    """The stubs have no attributes at all: a refusal that came after anything read `self` would be an AttributeError."""
    from image_captioning_amd.text_generation_model import CaptionModelV1
    from image_captioning_amd.text_generation_model_v2 import CaptionModelV2
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    feat = np.zeros((2, 7, 7, 256), np.float32)
    with pytest.raises(ValueError):
        CaptionModelV1.generate(object.__new__(CaptionModelV1), feat, return_probabilities=False, decoder="sampling", **kw)
    with pytest.raises(ValueError):
        CaptionModelV2.generate(object.__new__(CaptionModelV2), feat, decoder="sampling", **kw)
    for pp in ("host", "device"):
        with pytest.raises(ValueError):
            DenseImageCapRCNN.generate_captions(object.__new__(DenseImageCapRCNN), [np.zeros((8, 8, 3), np.uint8)], return_probabilities=False,
                                                decoder="sampling", postprocess=pp, **kw)
    args = dict(kw)
    seed = args.pop("seed", None)
    with pytest.raises(ValueError):
        CaptionModelV1.decode_sampling(object.__new__(CaptionModelV1), feat, seed, **args)
    with pytest.raises(ValueError):
        CaptionModelV2.decode_sampling(object.__new__(CaptionModelV2), feat, seed, **args)


def test_return_probabilities_is_refused_by_generate():
    from image_captioning_amd.text_generation_model import CaptionModelV1
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    for rp in (True, None):
        with pytest.raises(ValueError, match="return_probabilities=False"):
            CaptionModelV1.generate(object.__new__(CaptionModelV1), np.zeros((2, 7, 7, 256), np.float32), return_probabilities=rp,
                                    decoder="sampling", seed=1)
        with pytest.raises(ValueError, match="return_probabilities=False"):
            DenseImageCapRCNN.generate_captions(object.__new__(DenseImageCapRCNN), [np.zeros((8, 8, 3), np.uint8)], return_probabilities=rp,
                                                decoder="sampling", seed=1)


def test_vocab_sample_refuses_cpu_tensors_and_bad_arguments():
    from image_captioning_amd import ops, _lib
    X, W = torch.zeros((4, 32)), torch.zeros((32, 16))
    with pytest.raises(_lib.DcapError, match="GPU"):
        ops.vocab_sample(X, W, seed=1)
    with pytest.raises(TypeError):                                              # seed is required; nothing positional after bias
        ops.vocab_sample(X, W)
    with pytest.raises(TypeError):
        ops.vocab_sample(X, W, None, 1.0, seed=1)
    for t in BAD_TEMPERATURES + (1e-60,):                                       # (1e-60: 1 / temperature is not a finite float32)
        with pytest.raises(_lib.DcapError, match="temperature"):
            ops.vocab_sample(X, W, seed=1, temperature=t)
    for k in BAD_TOP_K + (17,):
        with pytest.raises(_lib.DcapError, match="top_k"):
            ops.vocab_sample(X, W, seed=1, top_k=k)
    with pytest.raises(_lib.DcapError, match="top_k"):                          # top_k above V
        ops.vocab_sample(X, W[:, :3], seed=1, top_k=4)
    for s in BAD_SEEDS:
        with pytest.raises(_lib.DcapError, match="seed"):
            ops.vocab_sample(X, W, seed=s)
    for o in (None, True, -1, 2 ** 32, 2.5):
        with pytest.raises(_lib.DcapError, match="offset"):
            ops.vocab_sample(X, W, seed=1, offset=o)


def test_vocab_sample_is_declared():
    from image_captioning_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dcap.h")).read()
    for line in ("size_t dc_vocab_sample_workspace_bytes(int M, int V, int top_k);",
                 "size_t dc_vocab_sample_bf16_workspace_bytes(int M, int V, int K, int top_k, int tile);",
                 "int    dc_vocab_sample_f32(const dc_vocab_sample_desc* d, void* workspace, size_t workspace_bytes, void* stream);",
                 "int    dc_vocab_sample_bf16(const dc_vocab_sample_bf16_desc* d, void* workspace, size_t workspace_bytes, void* stream);"):
        assert line in header, line
        assert line.split("(")[0].split()[-1] in _lib.SYMBOLS
    assert "#define DC_ABI_VERSION 600" in header
    names = [n for n, _ in _lib.VocabSampleDesc._fields_]
    assert names[:len(_lib.VocabTop1Desc._fields_)] == [n for n, _ in _lib.VocabTop1Desc._fields_]
    assert names[-4:] == ["inv_t", "seed", "offset", "top_k"]
    names = [n for n, _ in _lib.VocabSampleBf16Desc._fields_]
    assert names[:len(_lib.VocabTop1Bf16Desc._fields_)] == [n for n, _ in _lib.VocabTop1Bf16Desc._fields_]
    assert names[-5:] == ["tile", "inv_t", "seed", "offset", "top_k"]


def test_restated_philox_matches_the_single_word_form():
    """Word 0 of the pair is tests/test_gpu_kernels.py::_philox2x32's value (the dropout masks' generator), on a few fixed counters."""
    def single(c0, c1, key):
        for _ in range(10):
            p = 0xD256D193 * c0
            c0, c1 = ((p >> 32) ^ key ^ c1) & 0xFFFFFFFF, p & 0xFFFFFFFF
            key = (key + 0x9E3779B9) & 0xFFFFFFFF
        return c0, c1
    cs = [(0, 0, 0), (1, 2, 3), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (12345, 2 ** 31, 99)]
    for c0, c1, key in cs:
        r0, r1 = S.philox2x32_pair(c0, c1, key)
        assert (int(r0), int(r1)) == single(c0, c1, key)
    u_lo, u_hi = (0 + 0.5) * 2.0 ** -23, ((2 ** 23 - 1) + 0.5) * 2.0 ** -23
    assert u_lo == 2.0 ** -24 and u_hi == 1 - 2.0 ** -24 and np.float32(u_hi) == u_hi


@pytest.mark.parametrize("tau", (1.0, 2.0))
def test_restated_noise_follows_gumbel_max(tau):
    """The specification, not the kernel: 8192 rows of the same 12 logits (steps of 1/512 within +-2), each drawn with the restated noise;
    the chi-square statistic of the counts against softmax(z / tau) has 11 degrees of freedom, and must lie below that distribution's
    1 - 1e-6 quantile, 48.87.  (Seed 2024, offset 77: 14.84 at tau = 1 and 12.61 at tau = 2.)"""
    V, n = 12, 8192
    z = np.random.default_rng(5).integers(-1024, 1025, V) / 512.0
    y = S.perturbed(np.tile(z, (n, 1)), tau, seed=2024, offset=77)
    ids, _ = S.choose(y)
    p = np.exp(z * S.inv_t(tau))
    p /= p.sum()
    counts = np.bincount(ids, minlength=V)
    chi2 = float(((counts - n * p) ** 2 / (n * p)).sum())
    print("tau %g: chi-square %.2f" % (tau, chi2))
    assert chi2 < 48.87
    # and the noise is a function of (seed, offset + row, column) alone
    g = S.noise(2024, 77, np.arange(8), np.arange(V))
    assert np.array_equal(g[3:], S.noise(2024, 80, np.arange(5), np.arange(V)))
    assert np.array_equal(g[:, 4:9], S.noise(2024, 77, np.arange(8), np.arange(4, 9)))
    assert np.array_equal(S.noise(1, 2 ** 32 - 2, np.arange(4), np.arange(V))[2:], S.noise(1, 0, np.arange(2), np.arange(V)))
