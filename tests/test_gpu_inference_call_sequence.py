"""The three inference entry points over the shared trunk -- DenseImageCapRCNN.generate_captions, ROITagRCNN.generate_roi_tags and
MaskRCNN.detect -- do the device work they did when each carried its own copy of the front (mold, upload, encoder pass, proposals,
RoIAlign) and of the result packing: every call to a public function of ops, by name and in order (_op_recorder.Recorder), and every
Tensor.cpu / .item / .numpy / .tolist (_decode_cases.record_host_syncs), against literal lists recorded from those copies.  Two markers
stand in the op lists for what Recorder cannot see: FORWARD where EncoderPlan.forward is called (the image upload and the encoder pass,
which replays its captured graph here: the models are built once and their plans settled), UPLOAD where the refine constants
(float64 [B, REFINE_CONSTS] on the host) go to the device.
The order invariant of postprocess='device': UPLOAD comes before FORWARD -- the stream is idle then and nothing waits on that copy.
Models: the smallest the suite builds (_decode_cases.joint_model, test_gpu_roitag_model.make_tag, test_gpu_maskrcnn_model.make_model),
one 96 x 128 image, one call to warm, one call recorded."""
import pytest
import torch

import _decode_cases as D
from _op_recorder import Recorder
import test_gpu_maskrcnn_model as MASK
import test_gpu_roitag_model as TAG

FORWARD, UPLOAD = "plan.forward", "upload:refine_consts"


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_MODELS = {}


def model_and_image(kind):
    """One model per entry point, its encoder plan settled (one eager pass, one captured: every later pass replays)."""
    if kind not in _MODELS:
        from image_captioning_amd import synth
        if kind == "captions":
            model = D.joint_model()[0]
        elif kind == "tags":
            model = TAG.make_tag("inference", Wt=TAG.tag_weights(spread=5.0, bias=0.0), POST_NMS_ROIS_INFERENCE=50, DETECTION_MAX_INSTANCES=10)[0]
        else:
            model = MASK.make_model()[0]
        img = synth.images(7, 1, 96, 128)[0]
        molded = torch.as_tensor(model.mold_inputs([img])[0])
        for _ in range(2):
            model.plan().forward(molded)
        _MODELS[kind] = (model, img)
    return _MODELS[kind]


def _captions(**kw):
    return "captions", lambda m, img: m.generate_captions([img], **kw)


def _tags(**kw):
    return "tags", lambda m, img: m.generate_roi_tags([img], **kw)


def _detect(**kw):
    return "detect", lambda m, img: m.detect([img], **kw)


GREEDY = dict(decoder="incremental", return_probabilities=False)
BEAM = dict(decoder="beam", beam_size=3, return_probabilities=False)
CASES = {
    "captions-greedy-host": _captions(**GREEDY),
    "captions-greedy-device": _captions(postprocess="device", **GREEDY),
    "captions-greedy-device-mold": _captions(postprocess="device", mold="device", **GREEDY),
    "captions-beam-host": _captions(**BEAM),
    "captions-beam-device": _captions(postprocess="device", **BEAM),
    "captions-prefix-host": _captions(decoder="prefix", return_probabilities=True),
    "tags-host": _tags(),
    "tags-host-mold": _tags(mold="device"),
    "tags-device": _tags(postprocess="device"),
    "tags-device-mold": _tags(postprocess="device", mold="device"),
    "detect-host": _detect(),
    "detect-device": _detect(postprocess="device"),
    "detect-device-mold": _detect(postprocess="device", mold="device"),
}
# postprocess='device' with an ops.refine_generations behind it (detect's device half pastes masks: it has no such constants)
REFINES_ON_DEVICE = {c for c in CASES if "-device" in c and not c.startswith("detect")}


def run_case(name, monkeypatch):
    """-> (op names with the two markers, host synchronisations) of the second call."""
    from image_captioning_amd import _lib
    kind, call = CASES[name]
    model, img = model_and_image(kind)
    call(model, img)
    p = model.plan()
    with monkeypatch.context() as mp, Recorder(model) as rec:
        forward, to = p.forward, torch.Tensor.to
        mp.setattr(p, "forward", lambda *a, **k: (rec.seq.append(FORWARD), forward(*a, **k))[1], raising=False)

        def to_device(self, *a, **k):
            if not self.is_cuda and self.dtype == torch.float64 and self.dim() == 2 and self.shape[1] == _lib.REFINE_CONSTS:
                rec.seq.append(UPLOAD)
            return to(self, *a, **k)
        mp.setattr(torch.Tensor, "to", to_device)
        syncs = D.record_host_syncs(mp)
        call(model, img)
    torch.cuda.synchronize()
    return rec.seq, syncs


# ---- the expected sequences: literals recorded from the per-entry-point copies, composed from their named pieces ----------------------
T = 5                                                          # joint_model's PADDING_SIZE: decode steps
MOLD = ["pack_resize_batch", "resize_pad_packed"]              # mold='device': the raw bytes packed on the host, resampled on the device
FRONT = [FORWARD, "rpn_proposals", "roi_align_pyramid"]
DEVICE_FRONT = [UPLOAD] + FRONT                                # postprocess='device' of the two models that refine on the device
HEAD = ["gemm", "bn_relu_fwd"] * 2                             # the shared RoI head
# Model 3 on one image's RoIs: the head, zf and zdf, the two packed recurrent kernels; per token the embedding-gather GEMM, LSTM-1, the z2
# GEMM, LSTM-2, the Dense-1024, then the selection
SETUP = HEAD + ["gemm", "gemm", "lstm_pack_urec", "lstm_pack_urec"]
STEP = ["gemm", "lstm_step", "gemm", "lstm_step", "gemm"]
GREEDY_DECODE = SETUP + (STEP + ["vocab_top1"]) * T
BEAM_DECODE = SETUP + (STEP + ["vocab_topk", "beam_step"]) * T + ["beam_backtrace"]
# the reference's loop: the head once, then per token the whole decoder over the prefix, the softmax and the argmax
PREFIX_DECODE = HEAD + ["gemm", "gemm", "lstm_seq_fwd", "gemm", "lstm_seq_fwd", "gemm", "gemm", "gemm", "softmax_ce", "argmax_rows"] * T
TAGS = HEAD + ["gemm", "tag_scores"]
DETECT = HEAD + ["gemm", "gemm", "class_select"]               # class logits, box deltas, the winners' six words
MASKS = ["roi_align_pyramid"] + ["conv2d"] * 4 + ["mask_head_tail"]
COPY = ["cpu", "numpy"]                                        # one device-to-host copy as the models write it: t.cpu().numpy()

EXPECTED = {
    # host: the decoder's results and the proposals come down; device: the one packed buffer
    "captions-greedy-host": (FRONT + GREEDY_DECODE, COPY * 2),
    "captions-greedy-device": (DEVICE_FRONT + GREEDY_DECODE + ["refine_generations"], COPY),
    "captions-greedy-device-mold": (MOLD + DEVICE_FRONT + GREEDY_DECODE + ["refine_generations"], COPY),
    "captions-beam-host": (FRONT + BEAM_DECODE, COPY * 2),
    "captions-beam-device": (DEVICE_FRONT + BEAM_DECODE + ["refine_generations"], COPY),
    # (per token the probabilities, the ids and the word scores; then the proposals)
    "captions-prefix-host": (FRONT + PREFIX_DECODE, COPY * (3 * T + 1)),
    # host: proposals, probabilities and scores come down
    "tags-host": (FRONT + TAGS, COPY * 3),
    "tags-host-mold": (MOLD + FRONT + TAGS, COPY * 3),
    "tags-device": (DEVICE_FRONT + TAGS + ["refine_generations"], COPY),
    "tags-device-mold": (MOLD + DEVICE_FRONT + TAGS + ["refine_generations"], COPY),
    # the selection comes down, the detections go up; then the class masks (host) or the pasted bytes (device)
    "detect-host": (FRONT + DETECT + MASKS, COPY * 2),
    "detect-device": (FRONT + DETECT + MASKS + ["mask_paste"], COPY * 2),
    "detect-device-mold": (MOLD + FRONT + DETECT + MASKS + ["mask_paste"], COPY * 2),
}


def upload_precedes_forward(seq):
    """The order invariant: the one upload of the refine constants is issued before the image upload and the encoder pass."""
    return seq.count(UPLOAD) == 1 and seq.count(FORWARD) == 1 and seq.index(UPLOAD) < seq.index(FORWARD)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_inference_call_issues_the_recorded_ops_and_host_copies(gpu, monkeypatch, case):
    seq, syncs = run_case(case, monkeypatch)
    print("\n%s\n  ops   %r\n  syncs %r" % (case, seq, syncs))
    assert (seq, syncs) == EXPECTED[case], case
    if case in REFINES_ON_DEVICE:
        assert upload_precedes_forward(seq), seq
    else:
        assert UPLOAD not in seq
