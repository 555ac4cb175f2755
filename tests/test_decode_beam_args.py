"""The argument rules of Model 3's beam decoder (CaptionModelV1.check_decoder, generate, decode_beam, the joint model's generate_captions)
and of ops.beam_step: no GPU needed."""
import numpy as np
import pytest
import torch


def test_check_decoder_beam_rules():
    from image_captioning_amd.text_generation_model import CaptionModelV1
    assert "beam" in CaptionModelV1.DECODERS
    for k in range(1, 9):
        CaptionModelV1.check_decoder("beam", False, beam_size=k)
        CaptionModelV1.check_decoder("beam", False, beam_size=k, score="prob", end_id=2)
    CaptionModelV1.check_decoder("beam", False, None, None, beam_size=np.int64(3), score="logprob", end_id=np.int32(1))
    for k in (None, 0, 9, True, 2.5):
        with pytest.raises(ValueError, match="decoder='beam'.*beam_size"):
            CaptionModelV1.check_decoder("beam", False, beam_size=k)
    with pytest.raises(ValueError, match="decoder='beam'.*beam_size"):         # the missing beam_size is reported before anything else
        CaptionModelV1.check_decoder("beam", True, "bf16", "f32", score="p", end_id=0)
    for e in (0, -1, -7, True, 2.5):
        with pytest.raises(ValueError, match="end_id"):
            CaptionModelV1.check_decoder("beam", False, beam_size=3, end_id=e)
    with pytest.raises(ValueError, match="score"):
        CaptionModelV1.check_decoder("beam", False, beam_size=3, score="lengthnorm")
    for rp in (True, None):
        with pytest.raises(ValueError, match="return_probabilities=False"):
            CaptionModelV1.check_decoder("beam", rp, beam_size=3)
    for dec, rp in (("prefix", None), ("incremental", False)):
        with pytest.raises(ValueError, match="beam_size"):
            CaptionModelV1.check_decoder(dec, rp, beam_size=3)
        with pytest.raises(ValueError, match="end_id"):
            CaptionModelV1.check_decoder(dec, rp, end_id=2)
    CaptionModelV1.check_decoder("beam", False, "bf16", "bf16", beam_size=3)
    CaptionModelV1.check_decoder("beam", False, "f32", "f32", beam_size=3)
    with pytest.raises(ValueError, match="vocab_math.*compute_dtype"):
        CaptionModelV1.check_decoder("beam", False, "bf16", "f32", beam_size=3)
    with pytest.raises(ValueError, match="vocab_math.*compute_dtype"):
        CaptionModelV1.check_decoder("beam", False, "bf16", beam_size=3)
    with pytest.raises(ValueError, match="vocab_math"):
        CaptionModelV1.check_decoder("beam", False, "fp16", "bf16", beam_size=3)


BAD = (dict(), dict(beam_size=0), dict(beam_size=9), dict(beam_size=True), dict(beam_size=2.5), dict(beam_size=3, end_id=0),
       dict(beam_size=3, end_id=-2), dict(beam_size=3, score="p"), dict(beam_size=3, return_probabilities=True),
       dict(beam_size=3, return_probabilities=None), dict(beam_size=3, vocab_math="bf16"), dict(beam_size=3, vocab_math="fp16"))


@pytest.mark.parametrize("kw", BAD, ids=[",".join("%s=%r" % i for i in kw.items()) or "no beam_size" for kw in BAD])
def test_generate_refuses_bad_beam_arguments_before_touching_the_device(kw):
    """Both stubs have no attributes at all: a refusal that came after anything read `self` would be an AttributeError."""
    from image_captioning_amd.text_generation_model import CaptionModelV1
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    kw = dict(dict(return_probabilities=False), **kw)
    with pytest.raises(ValueError):
        CaptionModelV1.generate(object.__new__(CaptionModelV1), np.zeros((2, 7, 7, 256), np.float32), decoder="beam", **kw)
    with pytest.raises(ValueError):
        DenseImageCapRCNN.generate_captions(object.__new__(DenseImageCapRCNN), [np.zeros((8, 8, 3), np.uint8)], decoder="beam", **kw)
    if "return_probabilities" not in kw or kw["return_probabilities"] is False:
        args = dict(kw)
        args.pop("return_probabilities")
        with pytest.raises(ValueError):
            CaptionModelV1.decode_beam(object.__new__(CaptionModelV1), np.zeros((2, 7, 7, 256), np.float32), args.pop("beam_size", None), **args)


def test_beam_arguments_are_refused_with_the_greedy_decoders():
    from image_captioning_amd.text_generation_model import CaptionModelV1
    from image_captioning_amd.dense_model import DenseImageCapRCNN
    for dec in ("prefix", "incremental"):
        for kw in (dict(beam_size=3), dict(end_id=2)):
            with pytest.raises(ValueError, match="decoder='beam'"):
                CaptionModelV1.generate(object.__new__(CaptionModelV1), np.zeros((2, 7, 7, 256), np.float32), return_probabilities=False,
                                        decoder=dec, **kw)
            with pytest.raises(ValueError, match="decoder='beam'"):
                DenseImageCapRCNN.generate_captions(object.__new__(DenseImageCapRCNN), [np.zeros((8, 8, 3), np.uint8)],
                                                    return_probabilities=False, decoder=dec, **kw)


def test_refine_generations_takes_caption_scores():
    """caption_scores replace the sum of log word scores as the NMS order: two heavily overlapping boxes, the survivor is the one the
    given scores prefer, whatever the word scores say."""
    from image_captioning_amd.config import Config
    from image_captioning_amd.dense_model import refine_generations

    class Cfg(Config):
        IMAGE_MIN_DIM = 128
        IMAGE_MAX_DIM = 128
    cfg = Cfg()
    rois = np.array([[.1, .1, .6, .6], [.11, .1, .6, .61], [.7, .7, .9, .9]])
    ws = np.array([[.9, .9], [.5, .5], [.4, .4]])
    window = (0, 0, 128, 128)
    _, keep = refine_generations(rois, ws, window, cfg)
    assert list(keep) == [0, 2]
    _, keep = refine_generations(rois, ws, window, cfg, caption_scores=np.array([-3., -1., -2.]))
    assert list(keep) == [1, 2]
    _, keep = refine_generations(rois, None, window, cfg, caption_scores=np.array([-1., -3., -0.5]))
    assert list(keep) == [2, 0]


def _step_args(R=2, k=2, steps=1):
    i = torch.zeros((steps, R, k), dtype=torch.int32)
    return [torch.zeros((k * R, k), dtype=torch.int32), torch.zeros((k * R, k)), None, torch.zeros((R, k)), i, i.clone(), 0, 1]


def test_beam_step_refuses_bad_arguments():
    from image_captioning_amd import ops, _lib
    R, k = 2, 2
    with pytest.raises(_lib.DcapError, match="GPU"):
        ops.beam_step(*_step_args())
    rows = lambda *U: [(torch.zeros((k * R, u)), torch.zeros((k * R, u))) for u in U]
    with pytest.raises(_lib.DcapError, match="GPU"):
        ops.beam_step(*_step_args(), rows=rows(8, 12))
    with pytest.raises(_lib.DcapError, match="at most 4 row sets"):
        ops.beam_step(*_step_args(), rows=rows(8, 8, 8, 8, 8))
    a, b = torch.zeros((k * R, 8)), torch.zeros((k * R, 8))
    for bad in ([(a, a)], [(a, b), (b, a.clone())], [(a, b), (a.clone(), b)], [(a, b), (torch.zeros((k * R, 4)), b.view(-1)[:k * R * 4].view(k * R, 4))]):
        with pytest.raises(_lib.DcapError, match="alias"):
            ops.beam_step(*_step_args(), rows=bad)
    base = torch.zeros((k * R * 8 + 4,))
    off = base[1:1 + k * R * 8].view(k * R, 8)                            # 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16
    with pytest.raises(_lib.DcapError, match="aligned"):
        ops.beam_step(*_step_args(), rows=[(off, b)])
    with pytest.raises(_lib.DcapError, match="aligned"):
        ops.beam_step(*_step_args(), rows=[(a, off)])
    with pytest.raises(_lib.DcapError, match="U % 4"):
        ops.beam_step(*_step_args(), rows=rows(6))
    with pytest.raises(_lib.DcapError, match=r"\[k\*R,U\]"):
        ops.beam_step(*_step_args(), rows=[(a, torch.zeros((k * R, 12)))])
    with pytest.raises(_lib.DcapError, match="finished_out"):
        ops.beam_step(*_step_args(), end_id=2)
    fin = torch.zeros((k * R,), dtype=torch.uint8)
    with pytest.raises(_lib.DcapError, match="finished_out must not alias"):
        ops.beam_step(*_step_args(), end_id=2, finished_in=fin, finished_out=fin)
    with pytest.raises(_lib.DcapError, match="end_id"):
        ops.beam_step(*_step_args(), end_id=-1, finished_out=fin)


def test_beam_step_is_declared():
    from image_captioning_amd import _lib
    assert "dc_beam_step_f32" in _lib.SYMBOLS and "dc_beam_select_f32" in _lib.SYMBOLS
    d = _lib.BeamStepDesc()
    assert len(d.U) == len(d.src) == len(d.dst) == _lib.BEAM_MAX_SETS == 4
    header = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "dcap.h")).read()
    assert "int    dc_beam_step_f32(const dc_beam_step_desc* d, void* stream);" in header and "#define DC_BEAM_MAX_SETS 4" in header
