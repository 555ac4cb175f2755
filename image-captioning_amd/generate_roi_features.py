"""Image-level features of the reference's feature_generation/ package
(feature_generation/generate_roi_features.py:60-75): ResNet-101 + FPN + RPN + ProposalLayer, PyramidROIAlign on
the POST_NMS_ROIS_INFERENCE proposals, mean over RoIs, flattened to 12 544 floats."""
import inspect
import os

import numpy as np

from . import utils
from .config import Config
from .modified_dense_model import DenseImageCapRCNN

ROOT_DIR = os.getcwd()
MODEL_DIR = os.path.join(ROOT_DIR, "logs")
MODEL_PATH = os.path.join(ROOT_DIR, "img_cap_dense.npz")      # the reference's img_cap_dense.h5, converted


DenseCapConfig = type("DenseCapConfig", (Config,), dict(NAME="dense image captioning", GPU_COUNT=1, IMAGES_PER_GPU=3, STEPS_PER_EPOCH=500,
                                                     VALIDATION_STEPS=50, EMBEDDING_SIZE=100, PADDING_SIZE=5, REDUCE_EMBEDDINGS=True))
InferenceConfig = type("InferenceConfig", (DenseCapConfig,), dict(GPU_COUNT=1, IMAGES_PER_GPU=1))

config = InferenceConfig()


def load_model(weights=None, model_path=None, **kw):
    model = DenseImageCapRCNN(mode="inference", model_dir=MODEL_DIR, config=kw.pop("config", config),
                              use_generated_rois=True, **kw)
    if weights is not None:
        model.set_weights(weights)
    else:
        model.load_weights(model_path or MODEL_PATH, by_name=True)
    return model


def generate_features(image, model, mold="host", device_features=False):
    """image: [H,W,3] uint8 array (the reference reads a JPEG path with skimage, which is absent here).
    mold='device': the image is resized on the GPU (DenseImageCapRCNN.generate_captions), the same features bit for bit.
    device_features=True: the same 12 544 floats as a float32 DEVICE tensor, reduced on the GPU (generate_captions(image_level=True),
    ops.row_mean: NumPy's summation order, the same bits) -- the [1000,7,7,256] block (50 MB) is not copied to the host to hand
    back 50 KB.  The feature model must take image_level= (ValueError otherwise: there is no host detour behind this switch)."""
    kw = {"mold": utils.check_mold(mold)} if mold != "host" else {}      # (feature models with the reference's plain signature keep working)
    if device_features:
        if "image_level" not in inspect.signature(model.generate_captions).parameters:
            raise ValueError("device_features=True needs a feature model whose generate_captions takes image_level= "
                             "(DenseImageCapRCNN); %s has none: use the default host path" % type(model).__name__)
        return model.generate_captions([np.asarray(image)], verbose=0, image_level=True, **kw)[0]['image_features']
    results = model.generate_captions([np.asarray(image)], verbose=0, **kw)
    return np.mean(results[0]['features'], axis=0).flatten()
