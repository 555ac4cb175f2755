"""The joint train step (image_captioning_amd/dense_model.py) issues the op calls it issued as one 200-line method, now that it is a
driver over named phases: every call the step makes to a public function of ops, by name and in order, `name@side` when the model's side
stream is current, and every range handed to the gradient exchange as `ready:<layer>`, against literal lists composed from the pieces of
the step (RPN backward per pyramid level, decoder forward, one FPN layer, ...).  The step leaves nothing behind on the caption model,
and with an exchange attached the early regulariser passes, the ranges that travel and the gap passes cover the bucket exactly once.
Every case: the smallest joint model of the suite, the encoder plan already replaying (the lists hold the step behind it), one step to
warm, one step recorded."""
import numpy as np
import pytest
import torch

from _joint_cases import joint_inputs, make_joint
from _op_recorder import Recorder, StubExchange

S, V, T = 128, 24, 5


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- the cases: (model, step) with step() = one call of the public API ------------------------------------------------------------
def _train(serial=False, all_layers=False, dp=False, T=T, **kw):
    model, cfg, _ = make_joint(S, V, T, 1, **kw)
    if all_layers:
        model.set_trainable(model.LAYER_REGEX["all"])
    model.compile(1e-4)
    model.use_step_graph = False
    model.use_side_stream = not serial
    if dp:
        model.grad_sync = StubExchange()
    inputs = joint_inputs(S, V, T)
    return model, inputs, lambda: model.train_on_batch_device(inputs)


def _eval():
    model, cfg, _ = make_joint(S, V, T, 1)
    inputs = joint_inputs(S, V, T)
    return model, inputs, lambda: model.test_on_batch_device(inputs)


def _host_shuffle():
    model, cfg, _ = make_joint(S, V, T, 1)
    inputs = joint_inputs(S, V, T)
    # (shuffle receives the index array itself, dense_model.detection_targets: the identity permutation np.arange(n) applied to it)
    return model, inputs, lambda: model.forward_backward(inputs, shuffle=lambda idx: idx[np.arange(len(idx))])


def _given():
    model, cfg, _ = make_joint(S, V, T, 1)
    inputs = joint_inputs(S, V, T)
    model.forward_backward(inputs, shuffle=None)
    tg = model.last_targets
    return model, inputs, lambda: model.forward_backward(inputs, shuffle=None, targets=(tg["rois"], tg["caps"]))


CASES = {
    "train": lambda: _train(rois=12),
    "train-serial": lambda: _train(serial=True, rois=12),
    "train-bf16": lambda: _train(T=8, rois=16, compute_dtype="bf16", conv_math="bf16"),
    "train-all": lambda: _train(all_layers=True, rois=12),
    "eval": _eval,
    "host-shuffle": _host_shuffle,
    "given": _given,
    "dp": lambda: _train(dp=True, rois=12),
    "dp-serial": lambda: _train(dp=True, serial=True, rois=12),
}


def run_case(name):
    """-> (model, Recorder of the second step, that step's return value)."""
    model, inputs, step = CASES[name]()
    p = model.plan()
    p.forward(model._images_u8(inputs[0]))                 # the encoder pass: eager here, captured by the warm step, replayed by the recorded one
    step()
    with Recorder(model) as rec:
        out = step()
    torch.cuda.synchronize()
    return model, rec, out


# ---- the expected sequences: literals, composed from the named pieces of the step ---------------------------------------------------
class Pieces(object):
    """The pieces of the step as op names, in fp32 (exact products everywhere) or for the bf16 model (bf16 storage, conv_math='bf16'):
    there a product's operands are cast (to_bf16) unless their producer wrote the bf16 copy or an earlier product of the step cached it."""

    def __init__(self, bf16):
        g = "gemm_bf16" if bf16 else "gemm"
        cast = ["to_bf16"] if bf16 else []
        # RPN backward of one pyramid level: head weight gradient (20 channels: fp32), head bias, head data gradient, ReLU, shared 3x3 weight
        # gradient and bias, data gradient into dP.  bf16: the ReLU writes dsh's bf16 copy, the level's map has one from the forward; the
        # rotated shared kernel is cast at level 0 and reused by the other four (_cast_cached)
        head = ["conv2d_wgrad", "colsum", "gemm", "relu_bwd"]
        if bf16:
            level = lambda first: head + ["wgrad_bf16_supported", "conv2d_wgrad_bf16", "colsum", "conv_bf16_supported"] + (cast if first else []) + ["conv2d_bf16"]
        else:
            level = lambda first: head + ["conv2d_wgrad", "colsum", "conv2d"]
        self.rpn_backward = ["zero_fill", "rpn_loss_grad", "conv_weight_dgrad_pack"] + level(True) + level(False) * 4
        self.device_sample = ["detection_targets", "roi_align_pyramid", "caption_tables"]
        # decoder forward: the RoI head (two GEMM + BN/ReLU layers), zf, the embedding-gather GEMM, LSTM-1, z2, LSTM-2, zdf, the Dense-1024, the fused
        # vocabulary loss.  bf16: X, hact0, f (once for zf and zdf), h1 and h2 are cast
        self.decoder_forward = ((cast + [g, "bn_relu_fwd"]) * 2 + cast + [g, g, "lstm_seq_fwd"] + cast + [g, "lstm_seq_fwd", g] + cast + [g]
                                + ["vocab_ce_supported", "vocab_ce"])
        # decoder backward, cut where a layer's gradients are final.  bf16: dz_d1, dzd_f, dz2, dz1, dzf and the two dacc are cast; without
        # dropout masks the recurrent kernels' gradients are bf16 GEMMs of their own
        du = [g] if bf16 else []
        self.decoder_backward = [("imgcap_lstm_d2", [g, g]),
                                 ("imgcap_lstm_d1", ["relu_bwd"] + cast + [g, "colsum", "fold_time"] + cast + [g]),
                                 ("imgcap_lstm2", [g, g, "lstm_seq_bwd"] + cast + du + [g, "colsum"]),
                                 ("imgcap_lstm1", [g, "lstm_seq_bwd"] + cast + du + [g, "colsum", "fold_time"] + cast + [g]),
                                 ("mrcnn_class_conv2 mrcnn_class_bn2", [g, "bn_relu_bwd"] + cast + [g]),
                                 ("mrcnn_class_conv1 mrcnn_class_bn1", [g, "bn_relu_bwd"] + cast + [g]),
                                 (None, [g])]                                  # dX
        self.roi_backward = ["roi_align_pyramid_bwd", "scatter2_add"]
        # one FPN output layer: rotated kernel, weight gradient, bias | data gradient (bf16: dP and the rotated kernel are cast); one lateral
        if bf16:
            self.fpn_output = (["conv_weight_dgrad_pack", "wgrad_bf16_supported", "to_bf16", "conv2d_wgrad_bf16", "colsum"], ["conv_bf16_supported", "to_bf16", "conv2d_bf16"])
            self.fpn_lateral = ["wgrad_bf16_supported", "conv2d_wgrad_bf16", "colsum"]
        else:
            self.fpn_output = (["conv_weight_dgrad_pack", "conv2d_wgrad", "colsum"], ["conv2d"])
            self.fpn_lateral = ["conv2d_wgrad", "colsum"]
        self.top_down = ["downsample2x_sum"] * 3


def _side(seq):
    return [n + "@side" for n in seq]


def _no_exchange(layers):
    return []


def _exchange(layers):
    """Data parallel: every layer's range gets its regulariser pass, then travels."""
    return [n for layer in layers.split() for n in ("l2_reg", "ready:" + layer)]


RPN = "rpn_conv_shared rpn_head"


def _backward(a, ready):
    """Decoder backward, RoIAlign backward, the four FPN output layers, the top-down sums, the four laterals."""
    seq = []
    for layers, ops_ in a.decoder_backward:
        seq += ops_ + (ready(layers) if layers else [])
    seq += a.roi_backward
    for level in (2, 3, 4, 5):
        seq += a.fpn_output[0] + ready("fpn_p%d" % level) + a.fpn_output[1]
    seq += a.top_down
    for level in (2, 3, 4, 5):
        seq += a.fpn_lateral + ready("fpn_c%dp%d" % (level, level))
    return seq


def _forked(a, ready=_no_exchange):
    """The RPN backward (with an exchange: and its ranges' travel) on the side stream, issued before the proposals; joined behind the decoder backward."""
    return _side(a.rpn_backward + ready(RPN)) + ["rpn_proposals"] + a.device_sample + a.decoder_forward + ["mean"] + _backward(a, ready)


def _serial(a, ready=_no_exchange):
    """The RPN backward in place behind the decoder forward; its ranges travel right before the decoder backward."""
    return ["rpn_proposals"] + a.device_sample + a.decoder_forward + a.rpn_backward + ["mean"] + ready(RPN) + _backward(a, ready)


def _host(a):
    """Host sample: the RPN backward behind the proposals (and their pinned copy), then RoIAlign on the uploaded sample; one regulariser pass."""
    return ["rpn_proposals"] + a.rpn_backward + ["roi_align_pyramid"] + a.decoder_forward + ["mean"] + _backward(a, _no_exchange) + ["l2_reg"]


# the trainable ResNet (layers = "all", one block in stage 4), fp32: per BatchNorm the shared helper, then the convolution's weight gradient
BN = ["bn_bwd", "colsum", "colsum", "mul"]
BN_CONV = BN + ["conv2d_wgrad"]
BLOCK = (["relu_bwd"] + BN_CONV + ["gemm", "relu_bwd"] + BN_CONV + ["conv_weight_dgrad_pack", "conv2d", "relu_bwd"] + BN_CONV + ["gemm"])     # 2c, 2b, 2a, dx
PROJECTION = BN_CONV + ["gemm"]                                # a stage's first block: its shortcut convolution
STRIDED = ["zero_fill", "scatter2_add"]                        # ... which reads every other pixel in stages 3..5


def _stage(blocks, strided):
    """The lateral's data gradient into dC, then the blocks last to first."""
    return ["gemm"] + BLOCK * (blocks - 1) + BLOCK + PROJECTION + (STRIDED if strided else [])


STEM = ["maxpool3x3s2_same_bwd", "relu_bwd"] + BN + ["mold_image_padded", "conv2d_wgrad", "zero_fill"]
TRUNK = _stage(3, True) + _stage(2, True) + _stage(4, True) + _stage(3, False) + STEM
FUSED_OPTIMIZER = ["reg_sumsq", "amsgrad_step"]                # regulariser, mask and clip norm inside the optimizer's two passes
PLAIN_OPTIMIZER = ["sumsq", "amsgrad_step"]
F32, BF16 = Pieces(False), Pieces(True)

EXPECTED = {
    "train": _forked(F32) + FUSED_OPTIMIZER,
    "train-serial": _serial(F32) + FUSED_OPTIMIZER,
    "train-bf16": _forked(BF16) + FUSED_OPTIMIZER,
    "train-all": _forked(F32) + TRUNK + FUSED_OPTIMIZER,
    "eval": ["rpn_proposals"] + F32.device_sample + F32.decoder_forward + ["mean"] + ["zero_fill"] * 5 + ["rpn_loss_grad", "l2_reg"],
    "host-shuffle": _host(F32),
    "given": _host(F32),
    "dp": _forked(F32, _exchange) + ["l2_reg"] + PLAIN_OPTIMIZER,             # (every range went early: the tail is the loss term alone)
    "dp-serial": _serial(F32, _exchange) + ["l2_reg"] + PLAIN_OPTIMIZER,
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_joint_step_issues_the_recorded_op_calls(gpu, case):
    model, rec, _ = run_case(case)
    assert rec.seq == EXPECTED[case], case
    cm = model.caption_model
    assert cm.grad_sync is None                            # the caption model's own value: the joint step leaves nothing behind on it
    assert not hasattr(model, "_targets_given")
    if case.startswith("dp"):
        n = model.store.flat.numel()
        seen = model.grad_sync.seen
        assert len(seen) == len(set(seen)) and set(seen) <= set(rec.reg)        # every range that travelled got its regulariser pass first
        pos = 0
        for lo, hi in sorted(rec.reg):                     # early passes + gap passes: the bucket, exactly once
            assert lo == pos and hi > lo, (lo, hi, pos)
            pos = hi
        assert pos == n
