"""What the decode test files (test_gpu_decode.py, _v2.py, _bf16.py, _beam_v1.py, _launch_sequence.py) share: device uploads, the
exactly representable vocabulary operands, the Model-3 and joint-model factories and the recorder of host synchronisations.  A plain
module (imported as `import _decode_cases as D`), no fixtures; the package is imported inside the functions, as in the test files."""
import numpy as np
import torch


def _dev(a, dt=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")


def _exact_operands(rng, Mr, K, V):
    """X, W, bias on coarse binary grids (X in steps of 1/8 within +-1, W in steps of 1/256 within +-1/16, bias in steps of 1/2048): every
    product and every partial sum of X W + bias is exact in fp32 at these sizes, so the logits are exact (exact ties included) whatever
    the summation order and a comparison with float64 measures the kernel's own reduction (max / argmax / sum of exp), not GEMM rounding
    (~1e-6 relative at K = 256 on N(0,1) data).  At most 5 significant bits each: exact in bf16 too."""
    X = (rng.integers(-8, 9, (Mr, K)) / 8.0).astype(np.float32)
    W = (rng.integers(-16, 17, (K, V)) / 256.0).astype(np.float32)
    b = (rng.integers(-1024, 1025, V) / 2048.0).astype(np.float32)
    return X, W, b


def _feat(seed, R):
    return np.random.default_rng(seed).standard_normal((R, 7, 7, 256)).astype(np.float32)


def v1_model(V, T, batch, seed, units=512, compute_dtype="f32", scale=1.0):
    """The Model-3 decoder (CaptionModelV1, inference mode) on synthetic weights; scale multiplies the vocabulary kernel (more peaked word
    distributions: clearer decisions)."""
    from image_captioning_amd import synth
    from image_captioning_amd.text_generation_model import DenseCapConfig, CaptionModelV1
    cfg = DenseCapConfig(V, synth.embedding_matrix(33, V), batch)
    cfg.PADDING_SIZE = T
    model = CaptionModelV1([7, 7, 256], cfg, units, 'inference', seed=seed, compute_dtype=compute_dtype)
    if scale != 1.0:
        model.load_weights({'imgcap_lstm_d2/kernel': model.get_weights_dict()['imgcap_lstm_d2/kernel'] * np.float32(scale)})
    return model


def joint_model(S=128, V=24, T=5, blocks=1, compute_dtype=None):
    """The joint model (DenseImageCapRCNN, inference mode) on synthetic weights -> (model, cfg, weights).  compute_dtype None: the
    constructor's own default, without the keyword."""
    from image_captioning_amd import synth
    from image_captioning_amd.config import Config
    from image_captioning_amd.dense_model import DenseImageCapRCNN

    class Cfg(Config):
        NAME = "joint"
        IMAGES_PER_GPU = 1
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
        POST_NMS_ROIS_TRAINING = 60
        TRAIN_ROIS_PER_IMAGE = 12
        PADDING_SIZE = T
        VOCABULARY_SIZE = V
        EMBEDDING_SIZE = 300
        RECURRENT_DROPOUT = 0.0
    cfg = Cfg()
    Wt = dict(synth.encoder_weights(0, blocks), **synth.rpn_weights(4))
    Wt['rpn_conv_shared/kernel'] = Wt['rpn_conv_shared/kernel'] * np.float32(0.05)
    Wt['rpn_bbox_pred/kernel'] = Wt['rpn_bbox_pred/kernel'] * np.float32(0.3)
    Wt.update(synth.head_weights(1))
    Wt['mrcnn_class_conv1/kernel'] = Wt['mrcnn_class_conv1/kernel'] * np.float32(0.05)
    Wt.update(synth.v1_weights(2, V))
    Wt['imgcap_embedding_layer/embeddings'] = synth.embedding_matrix(3, V)
    cfg.EMBEDDING_WEIGHTS = Wt['imgcap_embedding_layer/embeddings']
    cfg.POST_NMS_ROIS_INFERENCE = 40
    cfg.DETECTION_MAX_INSTANCES = 10
    kw = {} if compute_dtype is None else dict(compute_dtype=compute_dtype)
    model = DenseImageCapRCNN("inference", cfg, "logs", stage4_blocks=blocks, **kw)
    model.set_weights(Wt)
    return model, cfg, Wt


def record_host_syncs(monkeypatch):
    """From here to monkeypatch.undo(), every Tensor.cpu / .item / .numpy / .tolist call appends its name to the returned list."""
    calls = []
    for name in ("cpu", "item", "numpy", "tolist"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda o, n: lambda self, *a, **k: (calls.append(n), o(self, *a, **k))[1])(orig, name))
    return calls
