"""The whole-image captioner's refusals, each by the name of what is wrong, before any GPU work (no GPU)."""
import numpy as np
import pytest

CFG = dict(embedding_dim=32, vocabulary_size=52, max_caption_length=4, batch_size=8)


def test_vocabulary_must_be_a_multiple_of_4():
    from image_captioning_amd.whole_image.model import check_vocabulary, create_model
    for V in (53, 54, 55, 2, 0):
        with pytest.raises(ValueError, match="vocabulary_size must be a positive multiple of 4"):
            create_model(dict(CFG, vocabulary_size=V))
    assert check_vocabulary(52) == 52 and check_vocabulary(8192) == 8192


def test_layer_widths_are_refused_by_name():
    from image_captioning_amd.whole_image.model import create_model
    with pytest.raises(ValueError, match="embedding_dim and the word width"):
        create_model(dict(CFG, embedding_dim=30))
    with pytest.raises(ValueError, match="embedding_dim and the word width"):
        create_model(CFG, word_dim=6)


def test_generate_refuses_bad_arguments_before_touching_the_gpu():
    from image_captioning_amd.whole_image.model import WholeImageCaptioner, check_generate
    assert WholeImageCaptioner.check_generate is check_generate
    assert check_generate(52, 5, 1, "prob") == (5, 1) and check_generate(52, 8, 0, "logprob") == (8, 0)
    for k in (9, 0, -1, None, 2.5, True):
        with pytest.raises(ValueError, match="beam_size in 1..8"):
            check_generate(52, k, 1, "prob")
    with pytest.raises(ValueError, match="beam_size 5 exceeds the vocabulary"):
        check_generate(4, 5, 1, "prob")
    with pytest.raises(ValueError, match="score must be one of"):
        check_generate(52, 5, 1, "likelihood")
    for s in (None, -1, 52, 1.5, True):
        with pytest.raises(ValueError, match="generate needs start_id"):
            check_generate(52, 5, s, "prob")


def test_device_features_needs_a_feature_model_with_image_level():
    from image_captioning_amd.generate_roi_features import generate_features

    class Plain(object):                       # the reference's signature: no image_level
        def generate_captions(self, images, verbose=0):
            return [{"features": np.ones((3, 7, 7, 256), np.float32)}]

    with pytest.raises(ValueError, match="image_level"):
        generate_features(np.zeros((8, 8, 3), np.uint8), Plain(), device_features=True)
    vec = generate_features(np.zeros((8, 8, 3), np.uint8), Plain())           # the default host path still serves such a model
    assert vec.shape == (12544,) and vec.dtype == np.float32 and np.all(vec == 1)


def test_the_start_word_must_be_known_to_the_tokenizer():
    from image_captioning_amd.whole_image.pipeline import Tokenizer
    from image_captioning_amd.whole_image.predict import start_id
    t = Tokenizer()
    t.fit_on_texts(["__START__ a dog __END__", "__START__ a cat __END__"])
    assert start_id(t) == t.word_index["start"] == 1
    empty = Tokenizer()
    empty.fit_on_texts(["a dog"])
    with pytest.raises(ValueError, match="start word"):
        start_id(empty)
