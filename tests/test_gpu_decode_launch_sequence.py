"""The decode drivers (image_captioning_amd/decoding.py) issue exactly the op calls of the per-model loops they replaced: every call the
decoders make to the public functions of ops, by name and in order, against literal lists recorded from those loops; and a model that
alternates its decoders keeps its scratch buffers: a _buf entry that every call in between left at the same shape has the same address
after a call of the second round as after that call of the first.  For Model 3 that is every entry (its greedy and beam buffers have
their own key prefixes).  The v2 decoders share the prefix `dec_`, so their row-shaped entries (dec_h0/c0/h1/c1, dec_zw, dec_z2/h2/c2,
dec_cat) are re-made at R and at k*R rows by turns, in the loops recorded from as here; every other entry must stay.
Shapes: the smallest with a first, a middle and a last step (T = 3), more than one RoI and more than one beam."""
import pytest
import torch

from _decode_cases import _feat, v1_model

OPS = ("gemm", "gemm_bf16", "bn_relu_fwd", "lstm_pack_urec", "lstm_step", "gather_rows", "vocab_top1", "vocab_topk", "beam_select", "beam_step",
       "beam_backtrace")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _v1_calls(dtype):
    """Model 3 (V=1000, T=3, B=4, 512 units) -> (model, {name: call})."""
    model = v1_model(1000, 3, 4, 30, compute_dtype=dtype)
    feat = torch.tensor(_feat(31, 4), device="cuda:0")
    vm = "bf16" if dtype == "bf16" else None
    calls = {"greedy": lambda: model.decode_greedy(feat, vocab_math=vm), "beam": lambda: model.decode_beam(feat, 2, vocab_math=vm)}
    if dtype == "f32":
        calls["beam_end"] = lambda: model.decode_beam(feat, 2, end_id=2)
    return model, calls


def _v2_calls(inject):
    """The v2 decoder (V=1000, Tw=4, 256 units, R=3, 3 steps) -> (model, {name: call})."""
    from image_captioning_amd import synth
    from image_captioning_amd.text_generation_model_v2 import DenseCapConfig, build_model
    cfg = DenseCapConfig(1000, synth.embedding_matrix(3, 1000))
    cfg.PADDING_SIZE = 4
    model = build_model((7, 7, 256), (4,), cfg, 256, inject, seed=0)
    feat = torch.tensor(_feat(8, 3), device="cuda:0")
    return model, {"greedy": lambda: model.decode_greedy(feat, steps=3), "beam": lambda: model.decode_beam(feat, 2, steps=3)}


def _steps(step, select, n=3):
    return (step + select) * n


# Model 3: the RoI head (two GEMM + BN/ReLU layers), the per-RoI halves zf and zdf, the two packed recurrent kernels; per token the
# embedding-gather GEMM, LSTM-1, the z2 GEMM, LSTM-2, the Dense-1024, then the selection.  A bf16 model runs every GEMM on the bf16 pipe.
def _v1_expected(g):
    setup = [g, "bn_relu_fwd", g, "bn_relu_fwd", g, g, "lstm_pack_urec", "lstm_pack_urec"]
    step = [g, "lstm_step", g, "lstm_step", g]
    beam = setup + _steps(step, ["vocab_topk", "beam_step"]) + ["beam_backtrace"]
    return {"greedy": setup + _steps(step, ["vocab_top1"]), "beam": beam, "beam_end": beam}


# v2: the folded RoI head (two GEMMs), then inject -- the constant half of the inject LSTM's input, the packed recurrent kernel; per token
# the embedding-gather GEMM, the word LSTM, the inject GEMM and its zero-state step -- or merge -- f gathered into the concat buffer, the
# packed kernel; per token the embedding-gather GEMM, the word LSTM, h_word gathered into the concat buffer; then the selection.
def _v2_expected(inject):
    setup = ["gemm", "gemm", "gemm" if inject else "gather_rows", "lstm_pack_urec"]
    step = ["gemm", "lstm_step"] + (["gemm", "lstm_step"] if inject else ["gather_rows"])
    return {"greedy": setup + _steps(step, ["vocab_top1"]), "beam": setup + _steps(step, ["vocab_topk", "beam_step"]) + ["beam_backtrace"]}


CASES = {"v1-f32": (lambda: _v1_calls("f32"), _v1_expected("gemm")), "v1-bf16": (lambda: _v1_calls("bf16"), _v1_expected("gemm_bf16")),
         "v2-inject": (lambda: _v2_calls(True), _v2_expected(True)), "v2-merge": (lambda: _v2_calls(False), _v2_expected(False))}


def record_ops(call):
    """The names of the ops functions `call` goes through, in order."""
    from image_captioning_amd import ops
    seen, saved = [], {name: getattr(ops, name) for name in OPS}
    try:
        for name, orig in saved.items():
            setattr(ops, name, (lambda o, n: lambda *a, **k: (seen.append(n), o(*a, **k))[1])(orig, name))
        call()
    finally:
        for name, orig in saved.items():
            setattr(ops, name, orig)
    return seen


def run_case(make):
    """Warm every decoder once, then two rounds of all of them in turn: ({name: recorded ops of round 1}, per call in the order made,
    both rounds, {key: (address, shape)} of the model's buffers after it)."""
    model, calls = make()
    for call in calls.values():
        call()
    seqs, after = {}, []
    for r in range(2):
        for name, call in calls.items():
            if r == 0:
                seqs[name] = record_ops(call)
            else:
                call()
            after.append({key: (buf.data_ptr(), tuple(buf.shape)) for key, buf in model._bufs.items()})
    torch.cuda.synchronize()
    return seqs, after


def moved_buffers(after):
    """[(call index of round 1, key)]: entries whose address after a call differs a round later although no call between changed their shape."""
    n = len(after) // 2
    return [(i, key) for i in range(n) for key, (ptr, shape) in after[i].items()
            if all(after[j].get(key, (0, None))[1] == shape for j in range(i, i + n + 1)) and after[i + n][key][0] != ptr]


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_decoders_issue_the_recorded_op_calls_and_keep_their_buffers(gpu, case):
    make, expected = CASES[case]
    seqs, after = run_case(make)
    for name, seq in seqs.items():
        assert seq == expected[name], (case, name)
    assert moved_buffers(after) == []
    if case.startswith("v1"):                              # nothing changes shape there: every entry, literally
        assert after[len(seqs):] == after[:len(seqs)]
