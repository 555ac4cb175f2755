"""The training pipeline of the reference (image captioning/pipeline.py): generate_config, get_tokenizer and the train / test / debug
generators, plus the slice of keras.preprocessing.text.Tokenizer they use (Keras is absent).  data_generator yields the reference's
layout and sample order -- every prefix of every caption, batch_size samples at a time -- but takes each image's vector from a per-image
cache (a dict, the <mode>_image_encoding.pkl file, or one encoder pass per image) instead of an encoder pass per sample."""
import collections
import os
import pickle

import numpy as np

from ..text_generation_model_v2 import pad_sequences
from .preprocess import encoding_path, read_captions, read_image_list

FILTERS = '!"#$%&()*+,-./:;<=>?@[\\]^_`{|}~\t\n'          # keras.preprocessing.text.Tokenizer's default filters


def text_to_word_sequence(text, filters=FILTERS, lower=True, split=" "):
    """keras.preprocessing.text.text_to_word_sequence: lower-case, every filter character becomes the split character, empty pieces
    dropped ('__START__' -> 'start')."""
    if lower:
        text = text.lower()
    text = text.translate(str.maketrans(filters, split * len(filters)))
    return [w for w in text.split(split) if w]


class Tokenizer(object):
    """keras.preprocessing.text.Tokenizer(num_words) as the reference uses it: fit_on_texts, texts_to_sequences, word_index, word_counts.
    Indices start at 1 and go by descending count, first occurrence first on ties (a stable sort of the insertion-ordered counts);
    texts_to_sequences drops unknown words and ids >= num_words."""

    def __init__(self, num_words=None, filters=FILTERS, lower=True, split=" "):
        self.num_words, self.filters, self.lower, self.split = num_words, filters, lower, split
        self.word_counts, self.word_index = collections.OrderedDict(), {}

    def fit_on_texts(self, texts):
        for text in texts:
            for w in text_to_word_sequence(text, self.filters, self.lower, self.split):
                self.word_counts[w] = self.word_counts.get(w, 0) + 1
        wcounts = sorted(self.word_counts.items(), key=lambda x: x[1], reverse=True)
        self.word_index = {w: i + 1 for i, (w, _) in enumerate(wcounts)}

    def texts_to_sequences(self, texts):
        out = []
        for text in texts:
            ids = (self.word_index.get(w) for w in text_to_word_sequence(text, self.filters, self.lower, self.split))
            out.append([i for i in ids if i is not None and not (self.num_words and i >= self.num_words)])
        return out


def _get_captions_text(data_dir, mode="all", dataset='flickr8k'):
    return [c for caps in read_captions(dataset=dataset, data_dir=data_dir, mode=mode).values() for c in caps]


def round_vocabulary(n):
    """The vocabulary the model is built with: n rounded up to a multiple of 4 (16-byte rows of the softmax kernel); the extra ids never
    occur as targets."""
    return max(4, (int(n) + 3) // 4 * 4)


def generate_config(data_dir, mode="all", dataset='flickr8k'):
    """pipeline.generate_config: embedding_dim 128, max_caption_length 10, batch_size 100, vocabulary_size = the number of distinct
    space-separated tokens of ALL captions -- rounded up to a multiple of 4 here -- and total_number_of_examples of `mode`."""
    config_dict = {"embedding_dim": 128, "vocabulary_size": -1, "max_caption_length": 10, "batch_size": 100, "total_number_of_examples": -1}
    tokens = set()
    for caption in _get_captions_text(data_dir, "all", dataset):
        tokens.update(caption.split(' '))
    config_dict["vocabulary_size"] = round_vocabulary(len(tokens))
    config_dict["total_number_of_examples"] = sum(len(c.split(' ')) - 1 for c in _get_captions_text(data_dir, mode, dataset))
    return config_dict


def get_tokenizer(config_dict, data_dir, dataset='flickr8k'):
    tokenizer = Tokenizer(num_words=config_dict["vocabulary_size"])
    tokenizer.fit_on_texts(_get_captions_text(data_dir, "all", dataset))
    return tokenizer


def train_generator(config_dict, data_dir, model, dataset, **kw):
    return data_generator(config_dict, data_dir, "train", model, dataset, **kw)


def test_generator(config_dict, data_dir, model, dataset, **kw):
    return data_generator(config_dict, data_dir, "test", model, dataset, **kw)


def debug_generator(config_dict, data_dir, model, dataset, **kw):
    return data_generator(config_dict, data_dir, "debug", model, dataset, **kw)


class FeatureCache(object):
    """One image vector per image: from feature_cache (a dict {image name: vector}), else from <mode>_image_encoding.pkl when it
    exists, else ONE encoder pass -- generate_features(load_image(path), model, device_features=True) -- whose result is kept."""

    def __init__(self, model=None, load_image=None, feature_cache=None, device=None, mold="host"):
        self.model, self.load_image, self.device, self.mold = model, load_image, device, mold
        self.cache = feature_cache if feature_cache is not None else {}
        self._dev = {}

    def host(self, name, path):
        if name not in self.cache:
            if self.model is None or self.load_image is None:
                raise KeyError("no cached image vector for %r and no (feature model, load_image) to compute it" % name)
            from ..generate_roi_features import generate_features
            self.cache[name] = generate_features(self.load_image(path), self.model, mold=self.mold, device_features=True)
        v = self.cache[name]
        return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)

    def dev(self, name, path):
        import torch
        if name not in self._dev:
            if name not in self.cache:
                self.host(name, path)
            v = self.cache[name]
            self._dev[name] = v if isinstance(v, torch.Tensor) else torch.tensor(np.asarray(v, np.float32), device=self.device)
        return self._dev[name]


def data_generator(config_dict, data_dir, mode, model, dataset, feature_cache=None, load_image=None, device_resident=False, device=None,
                   mold="host"):
    """pipeline.data_generator: an endless generator of ([image vectors [B,12544], prefixes int [B,T] pre-padded], one-hot float64
    [B,V]) in the reference's sample order: for every image of the mode's list and every caption of it, every prefix caption[:i + 1]
    with caption[i + 1] as the next word; batch_size samples per yield.  As in the reference the counter and the lists are reset at
    the top of every pass, so what a pass leaves over (fewer than batch_size samples) is dropped there.
    The image vector comes from FeatureCache (feature_cache=, the mode's pickle, or one encoder pass per IMAGE through `model` and
    load_image(path) -> uint8 [H,W,3]) instead of the reference's encoder pass per SAMPLE.
    device_resident=True: the image vectors as one device tensor [B,12544] and the targets as int32 ids [B] instead of [B,V] float64
    one-hot rows; the model's train_on_batch / fit_generator take both forms."""
    batch_size, T = config_dict["batch_size"], config_dict["max_caption_length"]
    tokenizer = get_tokenizer(config_dict, data_dir, dataset)
    image_list = read_image_list(dataset=dataset, mode=mode, data_dir=data_dir)
    image_captions = read_captions(dataset=dataset, data_dir=data_dir)
    if feature_cache is None and os.path.exists(encoding_path(data_dir, mode)):
        with open(encoding_path(data_dir, mode), "rb") as doc:
            feature_cache = pickle.load(doc)
    cache = FeatureCache(model, load_image, feature_cache, device, mold)
    names, paths, captions = [], [], []
    for name in image_list:
        for caption in image_captions[name]:
            names.append(name)
            paths.append(data_dir + dataset + '/' + name)
            captions.append(caption)
    captions = tokenizer.texts_to_sequences(captions)
    while True:
        imgs, sofar, nxt = [], [], []
        for caption, name, path in zip(captions, names, paths):
            for index in range(len(caption) - 1):
                imgs.append(cache.dev(name, path) if device_resident else cache.host(name, path))
                sofar.append(caption[:index + 1])
                nxt.append(caption[index + 1])
                if len(imgs) == batch_size:
                    words = pad_sequences(sofar, maxlen=T, padding="pre")
                    if device_resident:
                        import torch
                        yield [torch.stack(imgs), words], np.asarray(nxt, np.int32)
                    else:
                        onehot = np.zeros((batch_size, tokenizer.num_words))
                        onehot[np.arange(batch_size), nxt] = 1
                        yield [np.asarray(imgs), words], onehot
                    imgs, sofar, nxt = [], [], []
