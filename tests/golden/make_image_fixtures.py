"""Generates the image fixtures of tests/test_host_logic.py: six seeded, photo-like 600 x 800 RGB JPEGs (the size of the
Visual Genome sample images the reference's dataset folder ships) under tests/golden/sample_images/, and
tests/golden/sample_images.json: for each, the decoded shape and a SHA-1 of the decoded RGB bytes as PIL decodes them, plus
the shape / window / scale resize_image gives for the reference's IMAGE_MIN_DIM = 800, IMAGE_MAX_DIM = 1024 and a SHA-1 of
the resized + padded pixels.  The JPEGs are committed: re-running this script re-encodes them, so only run it to replace
the fixtures on purpose:
    python tests/golden/make_image_fixtures.py
The test re-derives the same numbers from the committed files."""
import hashlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
IMAGES = os.path.join(HERE, "sample_images")
NAMES = ["%d.jpg" % i for i in range(6)]


def describe(path):
    from image_captioning_amd import utils
    img = utils.imread(path)
    out, window, scale, padding = utils.resize_image(img, min_dim=800, max_dim=1024, padding=True)
    return {"shape": list(img.shape), "sha1": hashlib.sha1(np.ascontiguousarray(img).tobytes()).hexdigest(),
            "resized_shape": list(out.shape), "window": [int(v) for v in window], "scale": float(scale),
            "resized_sha1": hashlib.sha1(np.ascontiguousarray(out).tobytes()).hexdigest(),
            "mean": float(img.mean()), "resized_mean": float(out[window[0]:window[2], window[1]:window[3]].mean())}


def synth_photo(seed, h=600, w=800):
    """Smooth colour gradients, a few soft-edged blobs and mild sensor-like noise: the spectrum of a photograph, so that the
    JPEG codec's every stage (DCT blocks, chroma subsampling, quantisation) is exercised, at a modest file size."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((h, w, 3), np.float32)
    for c in range(3):
        a, b, p = rng.uniform(-1, 1, 3)
        img[..., c] = 128 + 60 * np.sin(a * x / 97.0 + b * y / 71.0 + 6.28 * p)
    for _ in range(8):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(30, 160)
        m = np.clip(1.5 - np.hypot(y - cy, x - cx) / r, 0, 1)[..., None]
        img = img * (1 - m) + m * rng.uniform(0, 255, 3).astype(np.float32)
    img += rng.normal(0, 4, img.shape).astype(np.float32)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


if __name__ == "__main__":
    from PIL import Image
    os.makedirs(IMAGES, exist_ok=True)
    for i, name in enumerate(NAMES):
        buf = io.BytesIO()
        Image.fromarray(synth_photo(i)).save(buf, format="JPEG", quality=85)
        with open(os.path.join(IMAGES, name), "wb") as f:
            f.write(buf.getvalue())
    rows = {name: describe(os.path.join(IMAGES, name)) for name in NAMES}
    with open(os.path.join(HERE, "sample_images.json"), "w") as f:
        json.dump(rows, f, indent=1, sort_keys=True)
    print(json.dumps(rows, indent=1)[:1500])
