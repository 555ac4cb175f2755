"""Tag vocabulary and tag encoding of the RoI tag classifier (roi_tag_classification/preprocess.py).

The reference picks the ADJ / NOUN tokens of a region phrase with NLTK's trained part-of-speech tagger (pos_tag(tokens,
tagset='universal')).  That model is data, not code, and is not part of this package: every function that needs it takes a `tagger`,
a callable from a token list to (token, universal tag) pairs -- nltk.tag.pos_tag with tagset='universal' where NLTK and its model are
installed, a lookup table otherwise.  tokenize_corpus (the corpus-wide tag count that builds the class list) is not provided for the
same reason; load_corpus takes the finished list."""
import numpy as np

from .treebank import word_tokenize

TAG_CLASSES = ("ADJ", "NOUN")


def load_corpus(tokens):
    """(tag_to_class_id, class_id_to_tag): class i is tokens[i]."""
    tokens = list(tokens)
    return {t: i for i, t in enumerate(tokens)}, dict(enumerate(tokens))


def encode_tag(tag, tag_to_class_id):
    """The tag's class id, -1 when it is not a class."""
    return tag_to_class_id.get(tag, -1)


def encode_region_tags(caption, tag_to_class_id, tagger):
    """A region phrase -> its multi-hot tag row, float64 [len(tag_to_class_id)]: the classes of its ADJ / NOUN tokens."""
    vector = np.zeros(len(tag_to_class_id))
    for token, tag in tagger(word_tokenize(caption.lower())):
        if tag in TAG_CLASSES and encode_tag(token, tag_to_class_id) != -1:
            vector[encode_tag(token, tag_to_class_id)] = 1
    return vector


def decode_tags(vector, class_id_to_tag):
    """A multi-hot (or thresholded probability) row -> its tags, in class order."""
    return [class_id_to_tag[i] for i in np.where(np.asarray(vector) > 0)[0]]
