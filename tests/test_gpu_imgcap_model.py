"""The whole-image captioner on the device (image_captioning_amd.whole_image) against the float64 restatement tests/_imgcap_ref.py:
the as-written batch, exact zero-padding of the 1000-unit LSTM, captured against eager steps, the beam search against gen_captions as
written, and the chain from an image to its captions on the tiny encoder configuration."""
import numpy as np
import pytest

import _imgcap_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SMALL = dict(input_dim=64, word_dim=32, language_units=32, merged_units=40)
CFG = dict(embedding_dim=32, vocabulary_size=52, max_caption_length=4, batch_size=37)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from image_captioning_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max()) / max(1e-30, float(np.abs(want).max()))


def _model(cfg=CFG, seed=0, **sizes):
    from image_captioning_amd.whole_image.model import create_model
    sizes = dict(SMALL, **sizes)
    model = create_model(cfg, seed=seed, **sizes)
    Wt = {k: v.astype(np.float64) for k, v in model.get_weights_dict().items()}
    return model, Wt


def _batch(seed, B, T, F, V):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, F)).astype(np.float32), rng.integers(0, V, (B, T)).astype(np.int32), rng.integers(0, V, B).astype(np.int32)


def test_as_written_batch_against_the_restatement(gpu):
    """predict, loss, accuracy, every gradient, three Adam steps at B = 37 (ragged against the 32-row LSTM step blocks), merged LSTM 40
    held as 64; the tolerances of tests/test_gpu_models.py::test_v2_as_written_batch."""
    model, Wt = _model()
    assert model.Ump == 64 and model.Ulp == 32
    assert [tuple(w.shape) for w in model.get_weights()] == [(52, 32), (64, 32), (32,), (32, 128), (32, 128), (128,), (32, 32), (32,),
                                                             (64, 160), (40, 160), (160,), (40, 52), (52,)]
    feat, words, tgt = _batch(1, 37, 4, 64, 52)
    onehot = np.eye(52)[tgt]
    probs = model.predict([feat, words])
    want_p = R.predict(Wt, feat, words)
    print("probs abs err %.3e, log err %.3e" % (np.abs(probs - want_p).max(), np.abs(np.log(probs + 1e-30) - np.log(want_p + 1e-30)).max()))
    assert probs.shape == (37, 52) and probs.dtype == np.float32
    assert np.abs(probs - want_p).max() < 1e-5
    assert np.abs(np.log(probs + 1e-30) - np.log(want_p + 1e-30)).max() < 1e-3
    opt = R.Adam()
    for step in range(3):
        loss, acc, G, _ = R.loss_and_grads(Wt, feat, words, tgt)
        t_loss, t_acc = model.test_on_batch([feat, words], onehot)
        got_loss, got_acc = model.train_on_batch([feat, words], onehot if step != 1 else tgt)          # one-hot rows and int32 ids
        print("step %d: loss %.6f (want %.6f), acc %.4f (want %.4f)" % (step, got_loss, loss, got_acc, acc))
        assert abs(t_loss - got_loss) <= 1e-6 * max(1.0, abs(loss)) and t_acc == got_acc        # the same batch, before the update
        assert abs(got_loss - loss) < 1e-4 * max(1.0, abs(loss))
        assert abs(got_acc - acc) < 1e-6                      # a count over 37, in float32
        Gp = {k: model.store.grad[k].cpu().numpy() for k in G}
        for k in G:
            g = model._strip(k, Gp[k])
            print("  %-40s rel_err %.3e" % (k, rel_err(g, G[k])))
            assert rel_err(g, G[k]) < 2e-4 or np.abs(G[k]).max() < 1e-12, (k, step)
            assert np.all(Gp[k][model.padding_mask(k)] == 0), k
        Wt = opt.step(Wt, G)
        now = model.get_weights_dict()
        for k in G:
            print("  %-40s weight err %.3e" % (k, np.abs(now[k] - Wt[k]).max()))
            assert np.abs(now[k] - Wt[k]).max() < 2e-5, (k, step)
    assert model.optimizer.iterations == 3
    # device tensors for all three inputs give the same step as host arrays
    a, _ = _model()
    b, _ = _model()
    la = a.train_on_batch([feat, words], tgt)
    lb = b.train_on_batch([torch.tensor(feat, device=gpu), torch.tensor(words, device=gpu)], torch.tensor(tgt, device=gpu))
    assert la == lb and torch.equal(a.store.flat, b.store.flat)
    # metrics=() skips the accuracy pass and returns the loss alone
    c, _ = _model()
    c.compile(optimizer='adam', loss='categorical_crossentropy', metrics=())
    assert c.train_on_batch([feat, words], tgt) == la[0] and torch.equal(c.store.flat, a.store.flat)


def test_padding_of_the_1000_unit_lstm_is_exact(gpu, tmp_path):
    from image_captioning_amd.hdf5_lite import H5File
    cfg = dict(embedding_dim=32, vocabulary_size=64, max_caption_length=3, batch_size=5)
    model, Wt = _model(cfg, seed=2, merged_units=1000)
    assert model.Ump == 1024
    feat, words, tgt = _batch(3, 5, 3, 64, 64)
    Wr, want_losses, _ = R.train_steps(Wt, [(feat, words, tgt)] * 3)
    for step in range(3):
        loss, _ = model.train_on_batch([feat, words], tgt)
        print("step %d: loss %.6f (want %.6f)" % (step, loss, want_losses[step]))
        assert abs(loss - want_losses[step]) < 1e-4 * max(1.0, abs(want_losses[step]))
    n_pad = 0
    for k in model.weight_names:
        pad = torch.tensor(model.padding_mask(k), device=gpu)
        n_pad += int(pad.sum())
        assert torch.all(model.store.w[k][pad] == 0), k
        assert torch.all(model.store.grad[k][pad] == 0), k
    assert n_pad == 24 * (64 * 4 + 1024 * 4 + 4 + 64) + 1000 * 24 * 4        # kernel, recurrent (rows and columns), bias, softmax rows
    shapes = {k: tuple(v.shape) for k, v in zip(model.weight_names, model.get_weights())}
    assert shapes["merged_model_lstm/kernel"] == (64, 4000) and shapes["merged_model_lstm/recurrent_kernel"] == (1000, 4000)
    assert shapes["merged_model_lstm/bias"] == (4000,) and shapes["merged_model_softmax/kernel"] == (1000, 64)
    # Keras HDF5 under the reference's layer names, and back into a fresh model bit for bit
    path = str(tmp_path / "weights-01.hdf5")
    model.save_weights(path)
    f = H5File(path)
    assert sorted(f.keys()) == sorted(R.LAYERS)
    assert f["merged_model_lstm"]["merged_model_lstm"]["recurrent_kernel:0"].shape == (1000, 4000)
    fresh, _ = _model(cfg, seed=9, merged_units=1000)
    before = fresh.predict([feat, words])
    fresh.load_weights(path)
    assert np.array_equal(fresh.predict([feat, words]), model.predict([feat, words])) and not np.array_equal(before, fresh.predict([feat, words]))
    assert torch.equal(fresh.store.flat, model.store.flat)
    other, _ = _model(cfg, seed=10, merged_units=1000)
    other.set_weights(model.get_weights())
    assert torch.equal(other.store.flat, model.store.flat)


def _run_steps(monkeypatch, graph):
    monkeypatch.setenv("DCAP_STEP_GRAPH", "1" if graph else "0")
    model, _ = _model(seed=4)
    model.use_step_graph = True                             # (opt-in for this model, as for the v2 decoders)
    losses = []
    for step in range(4):
        feat, words, tgt = _batch(20 + step, 37, 4, 64, 52)             # the inputs change every step
        losses.append(model.train_on_batch([feat, words], tgt))
    captured = [cs.last for cs in model._steps.values()]
    return losses, model.store.flat.clone(), model.optimizer.iterations, captured


def test_captured_step_is_bit_equal_to_the_eager_step(gpu, monkeypatch):
    """Four steps with DCAP_STEP_GRAPH=1 (two eager, the capture, one replay) against DCAP_STEP_GRAPH=0: losses, accuracies and the
    whole bucket identical."""
    le, fe, ie, ce = _run_steps(monkeypatch, False)
    lg, fg, ig, cg = _run_steps(monkeypatch, True)
    assert ce == [] and cg == ["replay"]
    assert ie == ig == 4
    assert le == lg
    assert torch.equal(fe, fg)


class _Exchange(object):
    """A gradient hook without `.world` (KerasLikeModel._captured_step counts it as an exchange: the step runs eagerly): counts its calls,
    keeps what it was handed and returns `scale`."""

    def __init__(self, scale):
        self.scale, self.calls = scale, []

    def __call__(self, flat_grad):
        self.calls.append(flat_grad)
        return self.scale


def test_eager_step_runs_the_gradient_exchange_and_applies_its_scale(gpu, monkeypatch):
    """An attached exchange is called once per step with the gradient bucket, between backward and update, and the step stays eager
    although graphs are asked for; with scale 1.0 two steps leave every weight bit-equal to a twin without the hook; the scale 0.5
    reaches the update: one step equals a twin's whose bucket was halved by hand before optimizer.apply (a power of two: exact)."""
    batches = [_batch(50 + i, 5, 4, 64, 52) for i in range(2)]
    monkeypatch.setenv("DCAP_STEP_GRAPH", "1")
    hooked, _ = _model(seed=4)
    hooked.use_step_graph = True
    hooked.grad_sync = _Exchange(1.0)
    for i, (feat, words, tgt) in enumerate(batches):
        hooked.train_on_batch_device([feat, words], tgt)
        assert len(hooked.grad_sync.calls) == i + 1 and hooked.grad_sync.calls[i] is hooked.store.flat_grad
    assert all(cs.graph is None for cs in hooked._steps.values())
    monkeypatch.setenv("DCAP_STEP_GRAPH", "0")
    plain, _ = _model(seed=4)
    for feat, words, tgt in batches:
        plain.train_on_batch_device([feat, words], tgt)
    assert plain.optimizer.iterations == hooked.optimizer.iterations == 2
    for k in plain.weight_names:
        assert torch.equal(plain.store.w[k], hooked.store.w[k]), k

    feat, words, tgt = batches[0]
    half, _ = _model(seed=4)
    half.grad_sync = _Exchange(0.5)
    half.train_on_batch_device([feat, words], tgt)
    assert len(half.grad_sync.calls) == 1
    twin, _ = _model(seed=4)
    twin._forward_train(*twin._batch([feat, words], tgt), want_grad=True)
    twin._backward()
    twin.store.flat_grad.mul_(0.5)
    twin.optimizer.apply(twin.store)
    one, _ = _model(seed=4)
    one.train_on_batch_device([feat, words], tgt)
    assert torch.equal(half.store.flat, twin.store.flat)
    assert not torch.equal(half.store.flat, one.store.flat)


# ---- beam search -----------------------------------------------------------------------------------------------------------------------
SEARCH_SEED, SEARCH_SCALE = 38, 8.0          # chosen on the CPU with the float64 model: see test_search_seed_has_no_near_ties


def _search_model(seed=SEARCH_SEED):
    """The small model with the restatement's weights of `seed`, the softmax kernel scaled for distinct probabilities."""
    model, _ = _model(seed=0)
    Wt = R.init_weights(seed, n_in=64, E=32, V=52, word=32, u_lang=32, u_merged=40, scale=SEARCH_SCALE)
    model.set_weights({k: v for k, v in Wt.items()})
    feats = np.random.default_rng(seed + 1).standard_normal((3, 64)).astype(np.float32)
    return model, Wt, feats


@pytest.mark.parametrize("R_", [1, 3])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_generate_equals_gen_captions_as_written(gpu, k, R_):
    """generate against the NumPy gen_captions restatement driven by the device model's own predict on batches of exactly k * R rows:
    tokens and scores equal; no two candidates of one image within 1e-6 of each other at any step, so no order depends on a tie rule."""
    model, _, feats = _search_model()
    feats = feats[:R_]
    calls = []

    def predict(inp):
        calls.append(inp[0].shape[0])
        return model.predict(inp)

    want_t, want_s, gap = R.gen_captions_batched(predict, feats, 1, 4, k)
    assert set(calls) == {k * R_} and len(calls) == 3
    assert gap > 1e-6, gap
    tokens, scores = model.generate(feats, beam_size=k, start_id=1, score="prob")
    print("k %d R %d: min gap %.3e, max |score - want| %.3e" % (k, R_, gap, np.abs(scores - want_s).max()))
    assert tokens.dtype == np.int32 and tokens.shape == (R_, k, 4) and scores.dtype == np.float32 and scores.shape == (R_, k)
    assert np.array_equal(tokens, want_t)
    assert np.array_equal(scores, want_s)


def test_generate_logprob(gpu):
    model, _, feats = _search_model()
    want_t, want_s, gap = R.gen_captions_batched(model.predict, feats, 1, 4, 3, log_score=True)
    assert gap > 1e-5, gap
    tokens, scores = model.generate(feats, beam_size=3, start_id=1, score="logprob")
    assert np.array_equal(tokens, want_t)
    # a sum of three float32 logarithms of probabilities that agree to a few ulps: 1e-5 relative to max(1, |score|), the bound the
    # v2 beam test uses for the same sum
    assert np.all(np.abs(scores - want_s) < 1e-5 * np.maximum(1.0, np.abs(want_s)))
    one, _ = model.generate(feats[0], beam_size=3, start_id=1, score="logprob")           # a single vector is a batch of one
    assert np.array_equal(one[0], tokens[0])


def test_search_seed_has_no_near_ties():
    """The seed above, checked with the float64 model alone (runs without the device model: nothing here touches the GPU)."""
    Wt = R.init_weights(SEARCH_SEED, n_in=64, E=32, V=52, word=32, u_lang=32, u_merged=40, scale=SEARCH_SCALE)
    feats = np.random.default_rng(SEARCH_SEED + 1).standard_normal((3, 64)).astype(np.float32)
    pred = lambda inp: R.predict(Wt, inp[0], inp[1]).astype(np.float32)
    for k in (1, 3, 5):
        assert R.gen_captions_batched(pred, feats, 1, 4, k)[2] > 1e-5
    assert R.gen_captions_batched(pred, feats, 1, 4, 3, log_score=True)[2] > 1e-4


# ---- from an image to its captions ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_encoder(gpu):
    """The encoder configuration of tests/test_gpu_models.py::test_image_level_features_with_rpn_proposals."""
    from image_captioning_amd import synth
    from image_captioning_amd.generate_roi_features import InferenceConfig, load_model
    S = 256

    class Cfg(InferenceConfig):
        IMAGE_MIN_DIM = S
        IMAGE_MAX_DIM = S
        POST_NMS_ROIS_INFERENCE = 200
    Wt = dict(synth.encoder_weights(0, 2), **synth.rpn_weights(4))
    Wt['rpn_conv_shared/kernel'] = Wt['rpn_conv_shared/kernel'] * np.float32(0.02)
    Wt['rpn_bbox_pred/kernel'] = Wt['rpn_bbox_pred/kernel'] * np.float32(0.3)
    return load_model(weights=Wt, config=Cfg(), stage4_blocks=2), synth.images(3, 2, S, S)


@pytest.mark.parametrize("mold", ["host", "device"])
def test_image_to_captions(gpu, tiny_encoder, mold):
    from image_captioning_amd.generate_roi_features import generate_features
    from image_captioning_amd.whole_image.pipeline import Tokenizer
    from image_captioning_amd.whole_image.predict import caption_images, make_caption_human_readable
    enc, imgs = tiny_encoder
    host = generate_features(imgs[0], enc, mold=mold)
    dev = generate_features(imgs[0], enc, mold=mold, device_features=True)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (12544,)
    assert host.dtype == np.float32 and np.array_equal(dev.cpu().numpy(), host)
    assert np.abs(host).max() > 0
    res = enc.generate_captions([imgs[1]], image_level=True, mold=mold)
    assert list(res[0]) == ["image_features"] and np.array_equal(res[0]["image_features"].cpu().numpy(), generate_features(imgs[1], enc, mold=mold))

    tok = Tokenizer(num_words=52)
    tok.fit_on_texts(["__START__ " + " ".join("w%d" % i for i in range(j, j + 12)) + " __END__" for j in range(40)])
    model, _ = _model(dict(CFG, max_caption_length=4), seed=6, input_dim=12544)
    caps = caption_images([imgs[0], imgs[1]], enc, model, tok, num_captions=3, mold=mold)
    vecs = np.stack([generate_features(im, enc, mold=mold) for im in imgs])
    tokens, scores = model.generate(vecs, beam_size=3, start_id=tok.word_index["start"])
    i2w = {v: k for k, v in tok.word_index.items()}
    assert len(caps) == 2 and all(len(c) == 3 for c in caps)
    for r in range(2):
        assert [t for t, _ in caps[r]] == [make_caption_human_readable(tokens[r, q], i2w) for q in range(3)]
        assert [s for _, s in caps[r]] == [float(s) for s in scores[r]]
        assert all(t.startswith("start") for t, _ in caps[r])
