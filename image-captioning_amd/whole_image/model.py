"""The whole-image captioner of the reference (image captioning/model.py:7-91) behind its own interface: create_model(config_dict)
returns a Keras-like object with the reference's layers under the reference's names

    image_model_fc            Dense(12544 -> E, relu), then RepeatVector(T)
    language_model_embedding  Embedding(V, 256)            (no mask_zero: id 0 is an ordinary word, pre-padding zeros are real steps)
    language_model_lstm       LSTM(256, return_sequences)
    language_model_td         TimeDistributed(Dense(E))
    merged_model_lstm         LSTM(1000) over concatenate([image, language])
    merged_model_softmax      Dense(V, softmax)

whose predict / train_on_batch / test_on_batch / fit_generator take the reference's batch ([feat [B,12544], words int [B,T]], one-hot
[B,V]), int32 ids [B] as targets, and device tensors for all three.  Every arithmetic step is one of the library's kernels:

  * word LSTM: the x-projection is ONE embedding-gather GEMM over the time-major ids, then ops.lstm_seq_fwd without a mask;
  * concatenate + RepeatVector are never materialised: merged_model_lstm/kernel is split into its image rows and its language rows,
    zi = relu(feat W_fc + b) W_img + bias is computed once per sample and enters the language half's GEMM as a row-periodic residual;
    backward, ops.fold_time(dz) is the sum over time that d(W_img), d(bias) and d(image vector) need;
  * every LSTM is HELD at its units rounded up to a multiple of 32 (1000 -> 1024: the fused step kernels take multiples of 32) with zero
    kernel / recurrent / bias entries per gate block for the extra units and zero rows of the Dense kernel that follows.  Such a unit
    stays exactly 0 (c = f 0 + i tanh(0), h = o tanh(0)), its gradients are exactly 0 and Adam moves it by exactly 0; get_weights /
    save_weights strip the padding, set_weights / load_weights add it -- files and arrays have Keras' shapes;
  * Dense(V) + softmax + categorical cross-entropy: ops.vocab_ce (mean over the batch), accuracy from one ops.vocab_top1 on the same
    activations (metrics=() skips it); the trainable embedding's gradient: ops.embedding_grad;
  * one flat ParamStore bucket, Keras' Adam in one launch, the whole step through step_graph when use_step_graph is set (opt-in, as for
    the v2 decoders; eager and replayed steps give the same bits).

generate(): test.py:23-64 gen_captions for R images at once on the device (decoding.beam).
"""
import numpy as np
import torch

from .. import decoding, ops, synth
from ..keras_like import KerasLikeModel, target_ids
from ..params import ParamStore

INPUT_DIM, WORD_DIM, LANGUAGE_UNITS, MERGED_UNITS = 12544, 256, 256, 1000
# Keras' model.weights order (layers by depth, then by creation)
LAYERS = ("language_model_embedding", "image_model_fc", "language_model_lstm", "language_model_td", "merged_model_lstm", "merged_model_softmax")
LSTM_UNIT = 32          # the fused LSTM step kernels take units that are multiples of 32


def held_units(units):
    return (int(units) + LSTM_UNIT - 1) // LSTM_UNIT * LSTM_UNIT


def _pad_gates(a, u, up):
    """[..., 4u] -> [..., 4up]: each gate block's u entries at the head of its up-wide block, zeros behind."""
    a = np.asarray(a, np.float32)
    out = np.zeros(a.shape[:-1] + (4 * up,), np.float32)
    for g in range(4):
        out[..., g * up:g * up + u] = a[..., g * u:(g + 1) * u]
    return out


def _strip_gates(a, u, up):
    return np.concatenate([a[..., g * up:g * up + u] for g in range(4)], axis=-1)


def _pad_rows(a, up):
    a = np.asarray(a, np.float32)
    out = np.zeros((up,) + a.shape[1:], np.float32)
    out[:a.shape[0]] = a
    return out


def check_vocabulary(V):
    if int(V) != V or V < 4 or V % 4:
        raise ValueError("vocabulary_size must be a positive multiple of 4 (16-byte rows of merged_model_softmax/kernel), got %r: "
                         "pipeline.generate_config rounds it up; the extra ids never occur as targets" % (V,))
    return int(V)


def check_generate(V, beam_size, start_id, score):
    """generate()'s argument rules (no GPU needed): beam_size an integer in 1..ops.TOPK_MAX and at most V, a known score rule, and a
    start_id in [0, V) -- the id of the tokenizer's 'start'; there is no default, since it depends on the corpus."""
    decoding.check_decoder("beam", beam_size, score)
    if int(beam_size) > V:
        raise ValueError("beam_size %d exceeds the vocabulary (%d words)" % (beam_size, V))
    if start_id is None or isinstance(start_id, bool) or int(start_id) != start_id or not 0 <= start_id < V:
        raise ValueError("generate needs start_id, the id of the caption's first word in [0, %d) "
                         "(tokenizer.word_index['start']), got %r" % (V, start_id))
    return int(beam_size), int(start_id)


def create_model(config_dict, compile_model=True, input_dim=INPUT_DIM, word_dim=WORD_DIM, language_units=LANGUAGE_UNITS,
                 merged_units=MERGED_UNITS, device=None, seed=0):
    """model.create_model with the reference's config keys (embedding_dim, vocabulary_size, max_caption_length, batch_size); the layer
    sizes the reference hard-codes are keyword arguments with its values as defaults.  compile_model: categorical_crossentropy, 'adam'
    (Keras' defaults), metrics=['accuracy']."""
    model = WholeImageCaptioner(config_dict, input_dim, word_dim, language_units, merged_units, device, seed)
    if compile_model:
        model.compile(loss='categorical_crossentropy', optimizer='adam', metrics=['accuracy'])
    return model


class WholeImageCaptioner(KerasLikeModel):
    def __init__(self, config_dict, input_dim=INPUT_DIM, word_dim=WORD_DIM, language_units=LANGUAGE_UNITS, merged_units=MERGED_UNITS,
                 device=None, seed=0):
        self.config = dict(config_dict)
        self.V = check_vocabulary(self.config["vocabulary_size"])
        self.E, self.T = int(self.config["embedding_dim"]), int(self.config["max_caption_length"])
        self.F, self.D, self.Ul, self.Um = int(input_dim), int(word_dim), int(language_units), int(merged_units)
        if self.E < 4 or self.E % 4 or self.D < 4 or self.D % 4 or self.F < 1 or self.Ul < 1 or self.Um < 1 or self.T < 1:
            raise ValueError("embedding_dim and the word width must be positive multiples of 4 (16-byte rows), the other sizes >= 1; got "
                             "embedding_dim %d, word width %d, input %d, LSTMs %d / %d, max_caption_length %d"
                             % (self.E, self.D, self.F, self.Ul, self.Um, self.T))
        self.Ulp, self.Ump = held_units(self.Ul), held_units(self.Um)
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        W = synth.whole_image_weights(seed, self.V, self.E, self.F, self.D, self.Ul, self.Um)
        self.keras_shapes = {k: tuple(v.shape) for k, v in W.items()}
        self.weight_names = list(W)                     # Keras' model.weights order
        st = ParamStore(self.device)
        for k in self.weight_names:
            st.add(k, self._pad(k, W[k]), True)
        self.store = st.finalize()
        self.metrics = ()
        self._init_runtime()
        self._weights_changed()

    # ---- Keras' shapes <-> the held (padded) ones ------------------------------------------------------------------------------------
    def _pad(self, name, a):
        layer, w = name.split("/")
        a = np.asarray(a, np.float32)
        for lstm, after, u, up in (("language_model_lstm", "language_model_td", self.Ul, self.Ulp),
                                   ("merged_model_lstm", "merged_model_softmax", self.Um, self.Ump)):
            if layer == lstm:
                a = _pad_gates(a, u, up)
                return _pad_rows(a, up) if w == "recurrent_kernel" else a
            if layer == after and w == "kernel":
                return _pad_rows(a, up)
        return a

    def _strip(self, name, a):
        layer, w = name.split("/")
        for lstm, after, u, up in (("language_model_lstm", "language_model_td", self.Ul, self.Ulp),
                                   ("merged_model_lstm", "merged_model_softmax", self.Um, self.Ump)):
            if layer == lstm:
                return np.ascontiguousarray(_strip_gates(a[:u] if w == "recurrent_kernel" else a, u, up))
            if layer == after and w == "kernel":
                return np.ascontiguousarray(a[:u])
        return a

    def padding_mask(self, name):
        """Boolean array of the held shape of `name`: True on the entries that belong to padded units."""
        ones = np.ones(self.keras_shapes[name], np.float32)
        return self._pad(name, ones) == 0

    def compile(self, optimizer='adam', loss='categorical_crossentropy', metrics=()):
        if loss != 'categorical_crossentropy':
            raise ValueError("the whole-image captioner trains on 'categorical_crossentropy' (model.py:88), got %r" % (loss,))
        metrics = tuple(metrics or ())
        if any(m != 'accuracy' for m in metrics):
            raise ValueError("metrics: 'accuracy' or none, got %r" % (metrics,))
        self.metrics = metrics
        KerasLikeModel.compile(self, optimizer, loss)

    def get_weights_dict(self):
        return {k: self._strip(k, self.store.w[k].detach().cpu().numpy()) for k in self.weight_names}

    def get_weights(self):
        """keras.Model.get_weights: the arrays in model.weights order, Keras' shapes."""
        d = self.get_weights_dict()
        return [d[k] for k in self.weight_names]

    def set_weights(self, weights):
        """keras.Model.set_weights (a list in get_weights' order) or a {'<layer>/<weight>': array} dict, Keras' shapes."""
        if not isinstance(weights, dict):
            weights = list(weights)
            if len(weights) != len(self.weight_names):
                raise ValueError("set_weights: %d arrays expected, got %d" % (len(self.weight_names), len(weights)))
            weights = dict(zip(self.weight_names, weights))
        self.load_weights(weights)

    def _stored_shape(self, name):                      # load_weights: files hold Keras' shapes, the model the padded ones
        return self.keras_shapes[name]

    _to_held = _pad

    # ---- engine ----------------------------------------------------------------------------------------------------------------------
    def _image_half(self, feat, p):
        """a = relu(feat W_fc + b) [R,E] and zi = a W_img + bias [R,4Um]: the merged LSTM's input from the image, once per sample."""
        w, R = self.store.w, feat.shape[0]
        a = ops.gemm(feat, w["image_model_fc/kernel"], shift=w["image_model_fc/bias"], relu=True, out=self._buf(p + 'a', (R, self.E)))
        zi = ops.gemm(a, w["merged_model_lstm/kernel"][:self.E], shift=w["merged_model_lstm/bias"], out=self._buf(p + 'zi', (R, 4 * self.Ump)))
        return a, zi

    def _stack(self, zi, R, ids_tm, n, T, p):
        """The T-step stack over n time-major sequences (row t * n + i; sequence i belongs to image i % R): -> the merged LSTM's last
        state [n,Um] (a view of its h sequence)."""
        w, Ul, Um = self.store.w, self.Ulp, self.Ump
        zx = ops.gemm(w["language_model_embedding/embeddings"], w["language_model_lstm/kernel"], gather=ids_tm,
                      shift=w["language_model_lstm/bias"], out=self._buf(p + 'zx', (T * n, 4 * Ul)))
        h_seq, _ = ops.lstm_seq_fwd(zx, w["language_model_lstm/recurrent_kernel"], None, n, T,
                                    self._buf(p + 'h_seq', (T * n, Ul)), self._buf(p + 'c_seq', (T * n, Ul)))
        td = ops.gemm(h_seq, w["language_model_td/kernel"], shift=w["language_model_td/bias"], out=self._buf(p + 'td', (T * n, self.E)))
        z2 = ops.gemm(td, w["merged_model_lstm/kernel"][self.E:], residual=zi, res_rows=R, out=self._buf(p + 'z2', (T * n, 4 * Um)))
        h2, _ = ops.lstm_seq_fwd(z2, w["merged_model_lstm/recurrent_kernel"], None, n, T,
                                 self._buf(p + 'h2', (T * n, Um)), self._buf(p + 'c2', (T * n, Um)))
        return h2[(T - 1) * n:]

    def _forward(self, feat, ids_tm, targets=None, want_probs=False, want_grad=False):
        """feat [B,F], ids_tm int32 [T*B] (time-major), targets int32 [B] or None -> (loss_rows or None, probs or None)."""
        w, g = self.store.w, self.store.grad
        B = feat.shape[0]
        T = ids_tm.numel() // B
        a, zi = self._image_half(feat, '')
        top = self._stack(zi, B, ids_tm, B, T, '')
        Wv, bv = w["merged_model_softmax/kernel"], w["merged_model_softmax/bias"]
        loss_rows = probs = dlog = None
        if want_probs:
            logits = ops.gemm(top, Wv, shift=bv, out=self._buf('logits', (B, self.V)))
            probs = self._buf('probs', (B, self.V))
            ops.softmax_ce(logits, None, probs)
        if targets is not None:
            loss_rows = self._buf('loss_rows', (B,))
            dlog = self._buf('dlogits', (B, self.V)) if want_grad else None
            ops.vocab_ce(top, Wv, bv, targets, loss_rows=loss_rows, dlogits=dlog, dbias=g["merged_model_softmax/bias"] if want_grad else None,
                         grad_scale=1.0 / B)
        self._ctx = (feat, ids_tm, B, T, a, top, dlog)
        return loss_rows, probs

    _forward_train = _forward          # (the name KerasLikeModel's train step calls)

    def _loss_and_metrics(self, loss_rows, feat, ids_tm, targets):
        """After _forward on this batch -> float32 device tensor [1 + len(metrics)]: the batch's mean loss, then Keras' categorical accuracy."""
        w, B, top = self.store.w, loss_rows.shape[0], self._ctx[5]
        out = self._buf('loss_acc', (1 + len(self.metrics),))
        ops.mean(loss_rows, out=out[0:1])
        if self.metrics:
            best = ops.vocab_top1(top, w["merged_model_softmax/kernel"], w["merged_model_softmax/bias"], tokens=self._buf('best', (B,), torch.int32))
            hit = torch.eq(best, targets, out=self._buf('hit', (B,), torch.bool))        # (bookkeeping on B flags, not model arithmetic)
            ops.mean(self._buf('hit_f', (B,)).copy_(hit), out=out[1:2])
        return out

    _step_loss = _loss_and_metrics     # the train step's loss tensor: [loss, accuracy]

    def _backward(self):
        """Gradients of every weight into the flat gradient bucket (every view is fully overwritten: the bucket needs no zeroing)."""
        w, g = self.store.w, self.store.grad
        feat, ids_tm, B, T, a, top, dlog = self._ctx
        E, Ul, Um, bufs = self.E, self.Ulp, self.Ump, self._bufs
        ops.gemm(top, dlog, a_trans=True, out=g["merged_model_softmax/kernel"])           # (the bias gradient came with the forward)
        dtop = ops.gemm(dlog, w["merged_model_softmax/kernel"], b_trans=True, out=self._buf('dtop', (B, Um)))
        dz2, _ = ops.lstm_seq_bwd(bufs['z2'], w["merged_model_lstm/recurrent_kernel"], None, bufs['h2'], bufs['c2'], B, T, dh_last=dtop,
                                  dz=self._buf('dz2', (T * B, 4 * Um)), dU=g["merged_model_lstm/recurrent_kernel"])
        gk = g["merged_model_lstm/kernel"]
        ops.gemm(bufs['td'], dz2, a_trans=True, out=gk[E:])
        dzi = ops.fold_time(dz2, T, B, self._buf('dzi', (B, 4 * Um)))                     # the image half was broadcast over time
        ops.gemm(a, dzi, a_trans=True, out=gk[:E])
        ops.colsum(dzi, out=g["merged_model_lstm/bias"])
        da = ops.gemm(dzi, w["merged_model_lstm/kernel"][:E], b_trans=True, out=self._buf('da', (B, E)))
        ops.relu_bwd(da, a, da)
        ops.gemm(feat, da, a_trans=True, out=g["image_model_fc/kernel"])
        ops.colsum(da, out=g["image_model_fc/bias"])
        dtd = ops.gemm(dz2, w["merged_model_lstm/kernel"][E:], b_trans=True, out=self._buf('dtd', (T * B, E)))
        ops.gemm(bufs['h_seq'], dtd, a_trans=True, out=g["language_model_td/kernel"])
        ops.colsum(dtd, out=g["language_model_td/bias"])
        dh_seq = ops.gemm(dtd, w["language_model_td/kernel"], b_trans=True, out=self._buf('dh_seq', (T * B, Ul)))
        dzx, _ = ops.lstm_seq_bwd(bufs['zx'], w["language_model_lstm/recurrent_kernel"], None, bufs['h_seq'], bufs['c_seq'], B, T, dh_seq=dh_seq,
                                  dz=self._buf('dzx', (T * B, 4 * Ul)), dU=g["language_model_lstm/recurrent_kernel"])
        ops.gemm(w["language_model_embedding/embeddings"], dzx, a_trans=True, gather=ids_tm, out=g["language_model_lstm/kernel"])
        ops.colsum(dzx, out=g["language_model_lstm/bias"])
        dx = ops.gemm(dzx, w["language_model_lstm/kernel"], b_trans=True, out=self._buf('dx', (T * B, self.D)))
        ops.embedding_grad(dx, ids_tm, g["language_model_embedding/embeddings"])

    # Replaying the step from a captured hipGraph is OPT-IN for this model, as for the v2 decoders: at the reference's batch (100 samples,
    # T = 10, V = 8192, the 1024-unit LSTM) the eager step is GPU-bound, 1.384 ms against 1.413 ms replayed with its three input copies
    # (tools/imgcap_bench.py, profiles/imgcap_bench.json).
    use_step_graph = False

    # train_step(feat, ids_tm, targets): KerasLikeModel's, on device tensors (feat [B,F], ids_tm int32 [T*B], targets int32 [B]); returns the
    # DEVICE tensor [loss, accuracy].  A captured step's batch reaches it through three device-to-device copies and one word (lr_t).
    def _step_key(self, feat, ids_tm, targets):
        return tuple(feat.shape), ids_tm.numel(), self.metrics

    def _stage_batch(self, cs, new, feat, ids_tm, targets):
        if new:
            cs.ids, cs.targets = torch.empty_like(ids_tm), torch.empty_like(targets)
        cs.feat.copy_(feat)
        cs.ids.copy_(ids_tm)
        cs.targets.copy_(targets)
        return (cs.feat, cs.ids, cs.targets), {}, self._stage_lr_t(cs, new)

    # ---- Keras surface ---------------------------------------------------------------------------------------------------------------
    def _ids_tm(self, words):
        """words [B,T] (numpy or torch, any integer type) -> (int32 device tensor [T*B] time-major, B)."""
        if isinstance(words, torch.Tensor):
            wd = words.to(self.device, torch.int32)
        else:
            a = np.asarray(words)
            if a.ndim != 2:
                raise ValueError("words must be [B,T] ids, got shape %s" % (a.shape,))
            if a.size and (a.min() < 0 or a.max() >= self.V):
                raise ValueError("word ids must lie in [0, %d)" % self.V)
            wd = torch.tensor(np.ascontiguousarray(a.astype(np.int32)), device=self.device)
        if wd.dim() != 2 or wd.shape[1] < 1:
            raise ValueError("words must be [B,T] ids, got shape %s" % (tuple(wd.shape),))
        return wd.t().contiguous().view(-1), wd.shape[0]

    def _targets(self, y):
        """one-hot [B,V] (the reference's generator) or ids [B], numpy or torch -> int32 device tensor [B]."""
        if isinstance(y, torch.Tensor):
            y = y.to(self.device)
            return (y.argmax(-1) if y.dim() == 2 else y).to(torch.int32).contiguous()
        return torch.tensor(np.ascontiguousarray(target_ids(y, 1, self.V)), device=self.device)

    def _batch(self, inputs, targets=None):
        feat, words = inputs
        feat = self._dev_feat(feat)
        ids_tm, B = self._ids_tm(words)
        if feat.dim() != 2 or tuple(feat.shape) != (B, self.F):
            raise ValueError("image features must be [%d,%d], got %s" % (B, self.F, tuple(feat.shape)))
        tg = None if targets is None else self._targets(targets)
        if tg is not None and tuple(tg.shape) != (B,):
            raise ValueError("one target per sample (%d), got shape %s" % (B, tuple(tg.shape)))
        return feat, ids_tm, tg

    def predict_device(self, inputs):
        feat, ids_tm, _ = self._batch(inputs)
        return self._forward(feat, ids_tm, want_probs=True)[1]

    def predict(self, inputs, verbose=0):
        """[feat [B,F], words [B,T]] -> the next word's probabilities float32 [B,V] (numpy)."""
        return self.predict_device(inputs).cpu().numpy()

    def train_on_batch_device(self, inputs, targets):
        """train_on_batch without the host round trip: float32 device tensor [loss, accuracy] ([loss] with metrics=())."""
        return self.train_step(*self._batch(inputs, targets))

    def test_on_batch_device(self, inputs, targets):
        feat, ids_tm, tg = self._batch(inputs, targets)
        loss_rows, _ = self._forward(feat, ids_tm, tg)
        return self._loss_and_metrics(loss_rows, feat, ids_tm, tg)

    def _losses_to_api(self, v):
        """train_on_batch / test_on_batch: [loss, accuracy] as Keras returns them with metrics=['accuracy'] (the loss alone without)."""
        return [float(x) for x in v] if self.metrics else float(v[0])

    # ---- beam search on the device (test.py:23-64) -----------------------------------------------------------------------------------
    check_generate = staticmethod(check_generate)

    def _decode_call(self, feat, k, start_id):
        """The decoding.Decode of one generate() call over the n = k*R beam-major rows.  Padding is in front and unmasked, so a prefix's
        LSTM state is no extension of its parent's: the carried 'state' is the PREFIX ROWS themselves -- int32 ids as float32 bit
        patterns in a [n, T rounded up to 4] row set, which ops.beam_step gathers behind the parents bit for bit -- and every step
        shifts the new word in and re-runs the T-step stack, as the reference does.  zi is computed once per image, before the loop."""
        R, T = feat.shape[0], self.T
        n, Tp = k * R, (self.T + 3) // 4 * 4
        _, zi = self._image_half(feat, 'dec_')
        tok = torch.full((n,), start_id, dtype=torch.int32, device=self.device)
        live = torch.ones((n,), dtype=torch.uint8, device=self.device)
        states = [[self._buf('dec_prefix%d' % q, (n, Tp))] for q in range(2)]
        ids_tm = self._buf('dec_ids', (T * n,), torch.int32)
        w = self.store.w

        def step(tok, mask, prev, cur):
            rows = cur[0].view(torch.int32)
            if prev is None:
                rows.zero_()
            else:
                rows[:, :T - 1].copy_(prev[0].view(torch.int32)[:, 1:T])
            rows[:, T - 1].copy_(tok)
            ids_tm.view(T, n).copy_(rows[:, :T].t())                    # time-major for the gather GEMM (copies, no arithmetic)
            return self._stack(zi, R, ids_tm, n, T, 'dec_')

        return decoding.Decode(self._buf, 'dec_', tok, live, None, states, step, (w["merged_model_softmax/kernel"], w["merged_model_softmax/bias"]))

    def generate(self, features, beam_size=5, start_id=None, score="prob"):
        """gen_captions (test.py:23-64) for the R image vectors of features [R,F] (or one [F]) at once: from the prefix [start_id], every
        hypothesis proposes its beam_size most probable next words (ops.vocab_topk over the beam_size * R rows), a candidate scores the
        hypothesis' score + p (score='prob', the reference's rule: the SUM of the word probabilities) or + log p ('logprob'), the
        beam_size best of the beam_size^2 survive (ops.beam_step), until the prefix holds max_caption_length ids; no end token.
        Returns numpy: tokens int32 [R,beam_size,T] (the start id first) and scores float32 [R,beam_size], best first (the reference
        lists them ascending).  No host synchronisation inside the loop; one device-to-host copy at the end."""
        k, start_id = check_generate(self.V, beam_size, start_id, score)
        feat = self._dev_feat(features)
        feat = feat[None] if feat.dim() == 1 else feat
        if feat.dim() != 2 or feat.shape[1] != self.F:
            raise ValueError("image features must be [R,%d], got %s" % (self.F, tuple(feat.shape)))
        R, steps = feat.shape[0], self.T - 1
        if steps < 1:
            raise ValueError("max_caption_length must be at least 2 to generate")
        out = decoding.beam(R, k, steps, self.device, lambda: self._decode_call(feat, k, start_id), score == "logprob")
        toks, sc = decoding.beam_views(out.cpu().numpy(), R, k, steps)
        tokens = np.concatenate([np.full((R, k, 1), start_id, np.int32), toks], axis=2)
        return tokens, sc.copy()
