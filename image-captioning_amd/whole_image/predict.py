"""image captioning/test.py (named predict here): captions for images from the feature model and the captioner, on the device."""
import numpy as np
import torch

START = "__START__"


def make_caption_human_readable(caption, index_to_word):
    return ' '.join(index_to_word.get(int(x), '') for x in caption)


def start_id(tokenizer):
    """The id of '__START__' as the tokenizer sees it (lower-cased, underscores filtered: 'start')."""
    ids = tokenizer.texts_to_sequences([START])[0]
    if len(ids) != 1:
        raise ValueError("the tokenizer does not know the caption start word %r (fit it on captions read by preprocess.read_captions)" % START)
    return ids[0]


def image_features(images, feature_model, mold="host"):
    """[R,12544] device tensor: one encoder pass per image, the mean over RoIs on the device."""
    from ..generate_roi_features import generate_features
    return torch.stack([generate_features(im, feature_model, mold=mold, device_features=True) for im in images])


def caption_images(images, feature_model, model, tokenizer, num_captions=5, mold="host", score="prob"):
    """test.predict / gen_captions for a batch of uint8 [H,W,3] images: image vectors from the device feature path, model.generate's beam
    search over all of them at once, ids decoded to words.  Returns per image [(caption text, score)] best first (the reference prints
    them ascending).  mold: 'host' | 'device' (where the images are resized)."""
    feats = image_features(images, feature_model, mold)
    tokens, scores = model.generate(feats, beam_size=num_captions, start_id=start_id(tokenizer), score=score)
    index_to_word = {v: k for k, v in tokenizer.word_index.items()}
    return [[(make_caption_human_readable(tokens[r, q], index_to_word), float(scores[r, q])) for q in range(tokens.shape[1])]
            for r in range(tokens.shape[0])]


def predict(image, feature_model, model, tokenizer, num_captions=5, mold="host"):
    """One image, as the reference's predict(): its num_captions captions, best first."""
    return caption_images([np.asarray(image)], feature_model, model, tokenizer, num_captions, mold)[0]
