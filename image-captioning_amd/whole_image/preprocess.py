"""Caption and image-list readers of the reference (image captioning/preprocess.py:24-88) and the image-encoding files
(prepare_image_dataset, :91-103) written from the device feature path: one encoder pass per image, the [1000,7,7,256] RoI block reduced
on the GPU (generate_features(device_features=True)), 50 KB per image to the host."""
import json
import os
import pickle

import numpy as np

from ..treebank import word_tokenize

START = "__START__ "
END = " __END__"


def read_captions(dataset='flickr8k', data_dir='../dataset/', mode='all'):
    """{image name: ['__START__ <caption> __END__', ...]} in file order."""
    if dataset == 'flickr8k':
        return read_captions_flickr(data_dir, mode)
    return read_captions_mscoco(data_dir, mode)


def read_captions_mscoco(data_dir, mode):
    """captions_<mode>2014.json: captions lower-cased and word-tokenised (nltk's word_tokenize: treebank.py restates it)."""
    with open(os.path.join(data_dir, 'captions_' + mode + '2014.json'), 'r', encoding='utf-8') as doc:
        image_data = json.load(doc)
    image_map = {d['id']: d['file_name'] for d in image_data['images']}
    captions = {}
    for d in image_data['annotations']:
        caption = START + ' '.join(word_tokenize(d['caption'].lower())) + END
        captions.setdefault(image_map[d['image_id']], []).append(caption)
    return captions


def read_captions_flickr(data_dir, mode):
    """Flickr8k.token.txt: '<image>#<n>\\t<caption>' per line; mode other than 'all' keeps the images of that split's list."""
    with open(os.path.join(data_dir, "Flickr8k.token.txt")) as doc:
        lines = [x.strip() for x in doc.read().split('\n')]
    captions = {}
    for line in lines:
        if not line:                          # (the reference fails on the file's trailing newline; an empty line carries no caption)
            continue
        image_name = line.split('#')[0].strip()
        captions.setdefault(image_name, []).append(START + line.split('\t')[1].strip() + END)
    if mode == "all":
        return captions
    return {name: captions[name] for name in read_image_list(dataset='flickr8k', mode=mode, data_dir=data_dir)}


def read_image_list(dataset='flickr8k', mode='train', data_dir='../dataset/'):
    if dataset == 'flickr8k':
        return read_image_list_flickr(mode, data_dir)
    return read_image_list_mscoco(mode, data_dir)


def read_image_list_mscoco(mode='train', data_dir='../dataset/'):
    with open(os.path.join(data_dir, 'captions_' + mode + '2014.json'), 'r', encoding='utf-8') as doc:
        return [d['file_name'] for d in json.load(doc)['images']]


def read_image_list_flickr(mode='train', data_dir='../dataset/'):
    with open(os.path.join(data_dir, "Flickr_8k." + mode + "Images.txt"), 'r') as doc:
        return [x.strip() for x in doc.read().split('\n') if x.strip()]


def encoding_path(data_dir, mode):
    return os.path.join(data_dir, "model", mode + "_image_encoding.pkl")


def encode_image(model, image, mold="host"):
    """image: uint8 [H,W,3] array -> the 12 544-float image vector (numpy), reduced on the device."""
    from ..generate_roi_features import generate_features
    return generate_features(image, model, mold=mold, device_features=True).cpu().numpy()


def prepare_image_dataset(feature_model, load_image, data_dir='../dataset/', mode_list=("train", "test", "debug"), dataset='flickr8k', mold="host"):
    """Write <data_dir>/model/<mode>_image_encoding.pkl = {image name: float32 [12544]} for every mode: ONE encoder pass per image
    (the reference's data_generator re-runs the encoder for every (caption, prefix) sample instead).  load_image(name) -> uint8
    [H,W,3] (the reference reads JPEG paths with skimage, which is absent here).  The file is written once per mode, not once per
    image as the reference does.  Returns {mode: path}."""
    paths = {}
    for mode in mode_list:
        encoding = {name: encode_image(feature_model, load_image(name), mold) for name in read_image_list(dataset=dataset, mode=mode, data_dir=data_dir)}
        path = encoding_path(data_dir, mode)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as doc:
            pickle.dump({k: np.asarray(v, np.float32) for k, v in encoding.items()}, doc)
        paths[mode] = path
    return paths
