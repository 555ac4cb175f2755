"""Entry point of the RoI tag classifier, mirroring roi_tag_classification/train_roi_tags.py (RoiTagConfig :17-36,
VisualGenomeDataset :39-111, __main__ :114-196): the tag class list, the two datasets and the model, the COCO-pretrained backbone
loaded by name, train(layers="3+").

The part-of-speech tagger the reference takes from NLTK is a caller-supplied callable here (roi_tag_preprocess); a dataset may also
be given precomputed multi-hot rows per region, which need no tagger."""
import json
import os
import pickle
import time

import numpy as np

from .config import Config
from .dense_model import check_prefetch, check_rpn_targets_mode
from .roi_tag_model import ROITagRCNN
from .roi_tag_preprocess import decode_tags, encode_region_tags, load_corpus
from .utils import Dataset, check_mold


class RoiTagConfig(Config):
    NAME = "roitag_rcnn"
    GPU_COUNT = 1
    IMAGES_PER_GPU = 2
    STEPS_PER_EPOCH = 1000
    VALIDATION_STEPS = 50
    LEARNING_RATE = 0.001

    def __init__(self, num_classes):
        super(RoiTagConfig, self).__init__()
        self.NUM_CLASSES = num_classes


class VisualGenomeDataset(Dataset):
    def __init__(self, tags_to_class_id, class_ids_to_tag, tagger=None):
        """tagger: tokens -> (token, universal POS tag) pairs (roi_tag_preprocess); None for a dataset whose regions carry precomputed
        tag rows (add_image(..., tags=[row per region]))."""
        super(VisualGenomeDataset, self).__init__()
        self.tag_to_class_id = tags_to_class_id
        self.class_id_to_tag = class_ids_to_tag
        self.tagger = tagger

    def load_visual_genome(self, data_dir, image_ids, image_meta_file, data_file):
        with open(data_file, 'r', encoding='utf-8') as doc:
            regions = {x['id']: x['regions'] for x in json.load(doc)}
        with open(image_meta_file, 'r', encoding='utf-8') as doc:
            meta = {x['image_id']: x for x in json.load(doc)}
        for i in image_ids:
            self.add_image("VisualGenome", image_id=i, path=os.path.join(data_dir, '{}.jpg'.format(i)),
                           width=meta[i]['width'], height=meta[i]['height'],
                           rois=[[d['y'], d['x'], d['y'] + d['height'], d['x'] + d['width']] for d in regions[i]],
                           captions=[[d['phrase']] for d in regions[i]])

    def image_reference(self, image_id):
        return "https://cs.stanford.edu/people/rak248/VG_100K/{}.jpg".format(self.image_info[image_id]["id"])

    def _tag_rows(self, info):
        if info.get('tags') is not None:
            rows = np.asarray(info['tags'], np.float64).reshape(len(info['rois']), -1)
            if rows.shape[1] != len(self.tag_to_class_id):
                raise ValueError("precomputed tag rows are %d wide, the class list has %d classes" % (rows.shape[1], len(self.tag_to_class_id)))
            return list(rows)
        return [self.encode_region_tags(caption[0]) for caption in info['captions']]

    def load_rois_and_tags(self, image_id):
        """rois [N,4]; tags [N,NUM_CLASSES] multi-hot (:84-95) -- every region is kept, one without a tag as an all-zero row."""
        info = self.image_info[image_id]
        return np.array(info['rois']), np.array(self._tag_rows(info))

    def load_original_rois_and_tags(self, image_id):
        """rois [N,4]; per region its tags as one comma-separated string (:97-107)."""
        info = self.image_info[image_id]
        return np.array(info['rois']), [', '.join(decode_tags(row, self.class_id_to_tag)) for row in self._tag_rows(info)]

    def encode_region_tags(self, caption):
        if self.tagger is None:
            raise ValueError("this dataset has no part-of-speech tagger: pass tagger= or give the regions precomputed tag rows")
        return encode_region_tags(caption, self.tag_to_class_id, self.tagger)


def load_tag_classes(class_id_to_tag_file, tag_to_class_id_file, tokens=None):
    """(tag_to_class_id, class_id_to_tag) from the reference's two pickles (:136-152); when they are missing they are written from
    `tokens`, the finished tag list (the reference counts it with NLTK's tagger, which this package does not carry)."""
    if os.path.exists(class_id_to_tag_file) and os.path.exists(tag_to_class_id_file):
        with open(class_id_to_tag_file, 'rb') as f:
            class_id_to_tag = pickle.load(f)
        with open(tag_to_class_id_file, 'rb') as f:
            tag_to_class_id = pickle.load(f)
        return tag_to_class_id, class_id_to_tag
    if tokens is None:
        raise FileNotFoundError("%s / %s are missing and no tag list was given to build them from" % (class_id_to_tag_file, tag_to_class_id_file))
    tag_to_class_id, class_id_to_tag = load_corpus(list(tokens))
    for path, obj in ((class_id_to_tag_file, class_id_to_tag), (tag_to_class_id_file, tag_to_class_id)):
        with open(path, 'wb') as f:
            pickle.dump(obj, f, protocol=pickle.HIGHEST_PROTOCOL)
    return tag_to_class_id, class_id_to_tag


def main(root_dir=None, init_with='coco', epochs=200, layers="3+", tagger=None, tokens=None, rpn_targets="host", mold="host", prefetch=0,
         optimizer=None):
    """tagger / tokens: see VisualGenomeDataset and load_tag_classes; rpn_targets, mold, prefetch, optimizer: ROITagRCNN.train's."""
    check_rpn_targets_mode(rpn_targets)
    check_mold(mold)
    check_prefetch(prefetch)
    root_dir = root_dir or os.getcwd()
    model_dir = os.path.join(root_dir, "logs_dense_img_cap")
    coco_model_path = os.path.join(root_dir, "../mask_rcnn_coco.npz")
    image_meta_file_path = '../dataset/image_data.json'
    data_file_path = '../dataset/region_descriptions.json'
    with open(image_meta_file_path, 'r', encoding='utf-8') as f:
        image_ids_list = [m['image_id'] for m in json.load(f)]
    train_image_ids, val_image_ids = image_ids_list[:90000], image_ids_list[90000:100000]
    tag_to_class_id, class_id_to_tag = load_tag_classes('../dataset/class_id_to_tag.pickle', '../dataset/tag_to_class_id.pickle', tokens)
    config = RoiTagConfig(len(class_id_to_tag))
    config.display()
    datasets = []
    for ids in (train_image_ids, val_image_ids):
        ds = VisualGenomeDataset(tag_to_class_id, class_id_to_tag, tagger)
        ds.load_visual_genome('../dataset/visual genome/', ids, image_meta_file_path, data_file_path)
        ds.prepare()
        datasets.append(ds)
    model = ROITagRCNN(mode="training", config=config, model_dir=model_dir)
    if init_with == "last":
        model.load_weights(model.find_last()[1], by_name=True)
    else:
        model.load_weights(coco_model_path, by_name=True)
    print(model.summary())
    start_time = time.time()
    model.train(datasets[0], datasets[1], learning_rate=config.LEARNING_RATE, epochs=epochs, layers=layers, rpn_targets=rpn_targets, mold=mold,
                prefetch=prefetch, optimizer=optimizer)
    print(time.time() - start_time)


if __name__ == '__main__':
    main()
