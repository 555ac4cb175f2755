"""Float64 NumPy restatement of the whole-image captioner (image captioning/model.py:7-91, pipeline.py:85-141, test.py:23-64) on Keras 2.1
semantics: the model's forward and backward with Keras' Adam, gen_captions as written (fed by a `predict` callable), the Tokenizer and
the data generator.  Shared by tests/test_imgcap_ref.py (CPU) and the GPU tests; nothing here imports the package.

Weights are a dict under the reference's layer names: image_model_fc/{kernel,bias}, language_model_embedding/embeddings,
language_model_lstm/{kernel,recurrent_kernel,bias}, language_model_td/{kernel,bias}, merged_model_lstm/{kernel,recurrent_kernel,bias},
merged_model_softmax/{kernel,bias}.  Keras 2.1 LSTM defaults: gate order i, f, c, o; hard-sigmoid gates; tanh candidate and output."""
import collections

import numpy as np

F64 = np.float64
KERAS_EPS = 1e-7
LAYERS = ("image_model_fc", "language_model_embedding", "language_model_lstm", "language_model_td", "merged_model_lstm", "merged_model_softmax")
FILTERS = '!"#$%&()*+,-./:;<=>?@[\\]^_`{|}~\t\n'          # keras.preprocessing.text.Tokenizer's default


def hard_sigmoid(z):
    return np.clip(0.2 * z + 0.5, 0.0, 1.0)


def hard_sigmoid_grad(z):
    y = 0.2 * z + 0.5
    return np.where((y >= 0.0) & (y <= 1.0), 0.2, 0.0)          # tf.clip_by_value passes the gradient on [min, max]


def glorot(rng, n_in, n_out):
    lim = np.sqrt(6.0 / (n_in + n_out))
    return rng.uniform(-lim, lim, (n_in, n_out))


def orthogonal(rng, rows, cols):
    a = rng.standard_normal((max(rows, cols), min(rows, cols)))
    q, r = np.linalg.qr(a)
    q = q * np.sign(np.diag(r))
    return q.T if rows < cols else q


def init_weights(seed, n_in, E, V, word, u_lang, u_merged, scale=1.0):
    """Keras 2.1's default initialisers (glorot_uniform kernels, orthogonal recurrent kernels, zero biases with unit_forget_bias,
    uniform(-0.05, 0.05) embeddings), float32 values.  scale multiplies the softmax kernel (sharper distributions for search tests)."""
    rng = np.random.default_rng(seed)
    W = collections.OrderedDict()

    def lstm(name, d, u):
        W[name + "/kernel"] = glorot(rng, d, 4 * u)
        W[name + "/recurrent_kernel"] = orthogonal(rng, u, 4 * u)
        b = np.zeros(4 * u)
        b[u:2 * u] = 1.0
        W[name + "/bias"] = b

    W["image_model_fc/kernel"], W["image_model_fc/bias"] = glorot(rng, n_in, E), np.zeros(E)
    W["language_model_embedding/embeddings"] = rng.uniform(-0.05, 0.05, (V, word))
    lstm("language_model_lstm", word, u_lang)
    W["language_model_td/kernel"], W["language_model_td/bias"] = glorot(rng, u_lang, E), np.zeros(E)
    lstm("merged_model_lstm", 2 * E, u_merged)
    W["merged_model_softmax/kernel"], W["merged_model_softmax/bias"] = glorot(rng, u_merged, V) * scale, np.zeros(V)
    return collections.OrderedDict((k, v.astype(np.float32)) for k, v in W.items())


def mm(a, b):
    """a @ b with the products of every output element added one by one in the order of the contraction index, whatever the shapes:
    BLAS picks its summation order by shape, and the zero-padding test below compares two shapes bit for bit."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    out = np.zeros((a.shape[0], b.shape[1]))
    for k in range(a.shape[1]):
        out += a[:, k:k + 1] * b[k:k + 1, :]
    return out


# ---- LSTM(return_sequences), no mask -------------------------------------------------------------------------------------------------
def lstm_forward(x, W, U, b):
    """x [B,T,D] -> H [B,T,u] and the cache of lstm_backward."""
    B, T, _ = x.shape
    u = U.shape[0]
    h, c = np.zeros((B, u)), np.zeros((B, u))
    H, steps = np.zeros((B, T, u)), []
    for t in range(T):
        z = mm(x[:, t], W) + mm(h, U) + b
        i, f, g, o = hard_sigmoid(z[:, :u]), hard_sigmoid(z[:, u:2 * u]), np.tanh(z[:, 2 * u:3 * u]), hard_sigmoid(z[:, 3 * u:])
        cn = f * c + i * g
        tc = np.tanh(cn)
        hn = o * tc
        steps.append((z, i, f, g, o, c, h, tc))
        h, c = hn, cn
        H[:, t] = h
    return H, (x, W, U, steps)


def lstm_backward(dH, cache):
    """dH [B,T,u] -> (dx [B,T,D], dW, dU, db)."""
    x, W, U, steps = cache
    B, T, _ = x.shape
    u = U.shape[0]
    dx, dW, dU, db = np.zeros(x.shape), np.zeros(W.shape), np.zeros(U.shape), np.zeros(4 * u)
    dh_next, dc_next = np.zeros((B, u)), np.zeros((B, u))
    for t in reversed(range(T)):
        z, i, f, g, o, cp, hp, tc = steps[t]
        dh = dH[:, t] + dh_next
        dcn = dh * o * (1.0 - tc * tc) + dc_next
        dz = np.concatenate([dcn * g * hard_sigmoid_grad(z[:, :u]), dcn * cp * hard_sigmoid_grad(z[:, u:2 * u]),
                             dcn * i * (1.0 - g * g), dh * tc * hard_sigmoid_grad(z[:, 3 * u:])], axis=1)
        dW += mm(x[:, t].T, dz)
        dU += mm(hp.T, dz)
        db += dz.sum(0)
        dx[:, t] = mm(dz, W.T)
        dh_next = mm(dz, U.T)
        dc_next = dcn * f
    return dx, dW, dU, db


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def forward(Wt, feat, words):
    """feat [B,F], words int [B,T] (pre-padded; id 0 is an ordinary word: no mask) -> (probs [B,V], cache)."""
    W = {k: np.asarray(v, F64) for k, v in Wt.items()}
    feat, words = np.asarray(feat, F64), np.asarray(words).astype(np.int64)
    B, T = words.shape
    pre = mm(feat, W["image_model_fc/kernel"]) + W["image_model_fc/bias"]
    a = np.maximum(pre, 0.0)
    emb = W["language_model_embedding/embeddings"][words]
    Hl, cl = lstm_forward(emb, W["language_model_lstm/kernel"], W["language_model_lstm/recurrent_kernel"], W["language_model_lstm/bias"])
    td = mm(Hl.reshape(B * T, -1), W["language_model_td/kernel"]).reshape(B, T, -1) + W["language_model_td/bias"]
    cat = np.concatenate([np.repeat(a[:, None], T, axis=1), td], axis=2)            # concatenate([RepeatVector(image), language])
    Hm, cm = lstm_forward(cat, W["merged_model_lstm/kernel"], W["merged_model_lstm/recurrent_kernel"], W["merged_model_lstm/bias"])
    top = Hm[:, -1]
    z = mm(top, W["merged_model_softmax/kernel"]) + W["merged_model_softmax/bias"]
    e = np.exp(z - z.max(-1, keepdims=True))
    probs = e / e.sum(-1, keepdims=True)
    return probs, dict(W=W, feat=feat, words=words, a=a, Hl=Hl, cl=cl, cm=cm, top=top, Hm=Hm)


def predict(Wt, feat, words):
    return forward(Wt, feat, words)[0]


def target_ids(y):
    y = np.asarray(y)
    return y.astype(np.int64) if y.ndim == 1 else y.argmax(-1)


def loss_rows(probs, ids):
    """K.categorical_crossentropy(one-hot, softmax output), TF backend: renormalise, clip to [1e-7, 1 - 1e-7], -log p_target."""
    p = probs / probs.sum(-1, keepdims=True)
    p = np.clip(p, KERAS_EPS, 1.0 - KERAS_EPS)
    return -np.log(p[np.arange(len(ids)), ids])


def loss_and_grads(Wt, feat, words, targets):
    """(loss, accuracy, {weight: gradient}, probs): the mean over the batch of the categorical cross-entropy and Keras' categorical
    accuracy; gradients of every weight (the embedding is trainable in the reference)."""
    probs, c = forward(Wt, feat, words)
    W, ids = c["W"], target_ids(targets)
    B, T = c["words"].shape
    E = W["image_model_fc/kernel"].shape[1]
    loss = loss_rows(probs, ids).mean()
    acc = float((probs.argmax(-1) == ids).mean())
    pt = probs[np.arange(B), ids]
    live = ((pt >= KERAS_EPS) & (pt <= 1.0 - KERAS_EPS)).astype(F64)                   # a clipped target probability passes no gradient
    dz = probs.copy()
    dz[np.arange(B), ids] -= 1.0
    dz *= (live / B)[:, None]
    G = {"merged_model_softmax/kernel": mm(c["top"].T, dz), "merged_model_softmax/bias": dz.sum(0)}
    dHm = np.zeros(c["Hm"].shape)
    dHm[:, -1] = mm(dz, W["merged_model_softmax/kernel"].T)
    dcat, G["merged_model_lstm/kernel"], G["merged_model_lstm/recurrent_kernel"], G["merged_model_lstm/bias"] = lstm_backward(dHm, c["cm"])
    da = dcat[:, :, :E].sum(1) * (c["a"] > 0)
    G["image_model_fc/kernel"], G["image_model_fc/bias"] = mm(c["feat"].T, da), da.sum(0)
    dtd = dcat[:, :, E:]
    G["language_model_td/kernel"] = mm(c["Hl"].reshape(B * T, -1).T, dtd.reshape(B * T, -1))
    G["language_model_td/bias"] = dtd.sum((0, 1))
    demb, G["language_model_lstm/kernel"], G["language_model_lstm/recurrent_kernel"], G["language_model_lstm/bias"] = \
        lstm_backward(mm(dtd.reshape(B * T, -1), W["language_model_td/kernel"].T).reshape(B, T, -1), c["cl"])
    ge = np.zeros(W["language_model_embedding/embeddings"].shape)
    np.add.at(ge, c["words"].reshape(-1), demb.reshape(B * T, -1))
    G["language_model_embedding/embeddings"] = ge
    return loss, acc, G, probs


class Adam(object):
    """keras.optimizers.Adam(lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=K.epsilon()=1e-7, decay=0, amsgrad=False), Keras 2.1."""

    def __init__(self, lr=0.001, b1=0.9, b2=0.999, eps=1e-7):
        self.lr, self.b1, self.b2, self.eps, self.t, self.m, self.v = lr, b1, b2, eps, 0, {}, {}

    def step(self, W, G):
        self.t += 1
        lr_t = self.lr * np.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        out = collections.OrderedDict()
        for k, p in W.items():
            g = np.asarray(G[k], F64)
            m = self.b1 * self.m.get(k, 0.0) + (1.0 - self.b1) * g
            v = self.b2 * self.v.get(k, 0.0) + (1.0 - self.b2) * g * g
            self.m[k], self.v[k] = m, v
            out[k] = np.asarray(p, F64) - lr_t * m / (np.sqrt(v) + self.eps)
        return out


def train_steps(Wt, batches):
    """Adam steps over [(feat, words, targets)] -> (weights after them, [loss], [accuracy])."""
    W, opt, losses, accs = collections.OrderedDict((k, np.asarray(v, F64)) for k, v in Wt.items()), Adam(), [], []
    for feat, words, targets in batches:
        loss, acc, G, _ = loss_and_grads(W, feat, words, targets)
        W = opt.step(W, G)
        losses.append(loss)
        accs.append(acc)
    return W, losses, accs


def pad_merged_units(Wt, units):
    """The same model with merged_model_lstm held at `units` >= its own: zero kernel / recurrent / bias entries per gate block for the
    extra units and zero rows of the softmax kernel."""
    W = collections.OrderedDict((k, np.asarray(v)) for k, v in Wt.items())
    u = W["merged_model_lstm/recurrent_kernel"].shape[0]

    def gates(a):
        out = np.zeros(a.shape[:-1] + (4 * units,), a.dtype)
        for g in range(4):
            out[..., g * units:g * units + u] = a[..., g * u:(g + 1) * u]
        return out

    W["merged_model_lstm/kernel"] = gates(W["merged_model_lstm/kernel"])
    W["merged_model_lstm/bias"] = gates(W["merged_model_lstm/bias"])
    rk = np.zeros((units, 4 * units), W["merged_model_lstm/recurrent_kernel"].dtype)
    rk[:u] = gates(W["merged_model_lstm/recurrent_kernel"])
    W["merged_model_lstm/recurrent_kernel"] = rk
    sk = np.zeros((units, W["merged_model_softmax/kernel"].shape[1]), W["merged_model_softmax/kernel"].dtype)
    sk[:u] = W["merged_model_softmax/kernel"]
    W["merged_model_softmax/kernel"] = sk
    return W


def unpad_merged_units(Gp, u):
    """The entries of pad_merged_units' shapes that belong to the first u units."""
    units = Gp["merged_model_lstm/recurrent_kernel"].shape[0]
    cols = np.concatenate([np.arange(g * units, g * units + u) for g in range(4)])
    G = dict(Gp)
    G["merged_model_lstm/kernel"] = Gp["merged_model_lstm/kernel"][:, cols]
    G["merged_model_lstm/bias"] = Gp["merged_model_lstm/bias"][cols]
    G["merged_model_lstm/recurrent_kernel"] = Gp["merged_model_lstm/recurrent_kernel"][:u][:, cols]
    G["merged_model_softmax/kernel"] = Gp["merged_model_softmax/kernel"][:u]
    return G


# ---- test.py:23-64 gen_captions ------------------------------------------------------------------------------------------------------
def pad_pre(seq, T):
    seq = list(seq)[-T:]
    return [0] * (T - len(seq)) + seq


def gen_captions(predict_fn, image_embedding, start, T, num_captions, log_score=False):
    """The reference's loop for ONE image, as written: every hypothesis is padded in front to T and run through predict on its own, its
    num_captions best next words (np.argsort(...)[-n:]) extend it, a candidate scores score + p (float32 arithmetic, as the device
    keeps scores; log_score: + log p), the list is sorted by score (list.sort: stable, ascending) and its last num_captions survive,
    until the prefix has T ids.  start: the ids of '__START__'.  Returns [(ids, score)] ascending, like the reference."""
    captions, scores = [list(start)], [np.float32(0.0)]
    both = None
    while len(captions[0]) < T:
        new_captions, new_scores = [], []
        for caption, score in zip(captions, scores):
            p = np.asarray(predict_fn([np.reshape(image_embedding, (1, -1)), np.asarray([pad_pre(caption, T)])]))[0]
            for w in np.argsort(p, kind="stable")[-num_captions:]:
                new_captions.append(caption + [int(w)])
                new_scores.append(np.float32(score) + (np.log(np.float32(p[w])) if log_score else np.float32(p[w])))
        both = sorted(zip(new_captions, new_scores), key=lambda x: x[1])[-num_captions:]
        captions, scores = [c for c, _ in both], [s for _, s in both]
    return both


def gen_captions_batched(predict_fn, feats, start_id, T, k, log_score=False):
    """gen_captions for R images at once with every predict call on exactly k * R rows, beam-major (hypothesis b of image r = row
    b * R + r; an image with fewer than k hypotheses repeats its first to fill) -- the batch shape a device search runs, so both see
    the same kernel instances.  Per image the arithmetic and the order are gen_captions'.  Returns (tokens int32 [R,k,T], scores
    float32 [R,k], best first; min_gap: the smallest score distance between two candidates of one image at any step)."""
    feats = np.asarray(feats)
    R = feats.shape[0]
    caps = [[[int(start_id)]] for _ in range(R)]
    scores = [[np.float32(0.0)] for _ in range(R)]
    min_gap = np.inf
    while len(caps[0][0]) < T:
        rows_f = np.concatenate([feats] * k, axis=0)
        rows_w = np.array([pad_pre(caps[r][b if b < len(caps[r]) else 0], T) for b in range(k) for r in range(R)], np.int32)
        P = np.asarray(predict_fn([rows_f, rows_w]))
        assert P.shape[0] == k * R
        for r in range(R):
            cand_c, cand_s = [], []
            for b, (caption, score) in enumerate(zip(caps[r], scores[r])):
                p = P[b * R + r]
                for w in np.argsort(p, kind="stable")[-k:]:
                    cand_c.append(caption + [int(w)])
                    cand_s.append(np.float32(score) + (np.log(np.float32(p[w])) if log_score else np.float32(p[w])))
            srt = np.sort(np.asarray(cand_s, F64))
            if len(srt) > 1:
                min_gap = min(min_gap, float(np.diff(srt).min()))
            both = sorted(zip(cand_c, cand_s), key=lambda x: x[1])[-k:]
            caps[r], scores[r] = [c for c, _ in both], [s for _, s in both]
    tokens = np.array([[caps[r][k - 1 - q] for q in range(k)] for r in range(R)], np.int32)
    sc = np.array([[scores[r][k - 1 - q] for q in range(k)] for r in range(R)], np.float32)
    return tokens, sc, min_gap


# ---- keras.preprocessing.text.Tokenizer (2.1) ----------------------------------------------------------------------------------------
def text_to_word_sequence(text, filters=FILTERS, lower=True, split=" "):
    if lower:
        text = text.lower()
    text = text.translate(str.maketrans(filters, split * len(filters)))
    return [w for w in text.split(split) if w]


class Tokenizer(object):
    def __init__(self, num_words=None):
        self.num_words, self.word_counts, self.word_index = num_words, collections.OrderedDict(), {}

    def fit_on_texts(self, texts):
        for text in texts:
            for w in text_to_word_sequence(text):
                self.word_counts[w] = self.word_counts.get(w, 0) + 1
        wcounts = sorted(self.word_counts.items(), key=lambda x: x[1], reverse=True)          # stable: first occurrence first on ties
        self.word_index = {w: i + 1 for i, (w, _) in enumerate(wcounts)}

    def texts_to_sequences(self, texts):
        out = []
        for text in texts:
            ids = [self.word_index.get(w) for w in text_to_word_sequence(text)]
            out.append([i for i in ids if i is not None and not (self.num_words and i >= self.num_words)])
        return out


# ---- pipeline.py:94-141 data_generator -----------------------------------------------------------------------------------------------
def data_generator(captions_ids, image_keys, features_of, batch_size, T, num_words):
    """The reference's loop over (tokenised caption, image) pairs: every prefix of every caption is a sample ([image vector, prefix
    pre-padded to T], one-hot next word), batch_size samples per yield; the lists are emptied only when a batch is yielded, so what a
    pass leaves over is dropped at `while True`'s next round -- exactly as the reference's counter and lists are reset there.
    features_of(key) -> the image vector."""
    while True:
        counter, imgs, sofar, nxt = 0, [], [], []
        for cap, key in zip(captions_ids, image_keys):
            for index in range(len(cap) - 1):
                one = np.zeros(num_words)
                one[cap[index + 1]] = 1
                imgs.append(features_of(key))
                sofar.append(pad_pre(cap[:index + 1], T))
                nxt.append(one)
                counter += 1
                if counter == batch_size:
                    yield [np.asarray(imgs), np.asarray(sofar, np.int32)], np.asarray(nxt)
                    counter, imgs, sofar, nxt = 0, [], [], []
