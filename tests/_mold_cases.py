"""What the train(mold="device") test files share (imported, never collected): the in-memory dataset of four raw images whose sizes
make the resize, the padding and the flip all do work, and the canvas a raw batch stands for, from PIL on the host."""
import numpy as np

import _resize_ref as R

MIN_DIM, MAX_DIM = 96, 128
# 75 x 100 -> 96 x 128 (up), 100 x 68 -> 128 x 87 (left padding 20, right 21: a flip moves the window by one column),
# 60 x 80 -> 96 x 128, 128 x 128 -> as it is
SIZES = [(75, 100), (100, 68), (60, 80), (128, 128)]


def make_dataset(T, V, boxes_of=lambda i: 7 if i == 0 else 2 + i % 3, sizes=SIZES, dtype=np.uint8, fail_on_load=None):
    """Image i is seeded noise of sizes[i] with boxes_of(i) boxes inside the 128 x 128 canvas and captions [start, w, w, end, 0...].
    The arrays are made once: load_image hands out the dataset's own.  .loads counts load_image calls; fail_on_load=n makes the n-th
    call and every later one raise (the generator skips up to five failing samples, then hands the error on)."""
    from image_captioning_amd.utils import Dataset

    class Toy(Dataset):
        loads = 0

        def load_image(self, image_id):
            self.loads += 1
            if fail_on_load is not None and self.loads >= fail_on_load:
                raise RuntimeError("load %d failed" % self.loads)
            return self.pixels[image_id]

        def load_captions_and_rois(self, image_id):
            r = np.random.RandomState(100 + image_id)
            n = boxes_of(image_id)
            y, x = r.randint(0, MAX_DIM // 2, n), r.randint(0, MAX_DIM // 2, n)
            boxes = np.stack([y, x, y + r.randint(8, MAX_DIM // 2, n), x + r.randint(8, MAX_DIM // 2, n)], axis=1).reshape(n, 4).astype(np.int64)
            caps = np.zeros((n, T), np.float32)
            caps[:, 0], caps[:, 1:3], caps[:, 3] = 1, r.randint(3, V, (n, 2)), 2
            return boxes, caps
    ds = Toy()
    ds.pixels = [np.random.default_rng(40 + i).integers(0, 256, (h, w, 3), dtype=np.uint8).astype(dtype) for i, (h, w) in enumerate(sizes)]
    for i in range(len(sizes)):
        ds.add_image("toy", image_id=i, path=None)
    ds.prepare()
    return ds


def canvases(raw, min_dim=MIN_DIM, max_dim=MAX_DIM):
    """uint8 [B,max_dim,max_dim,3]: np.pad(PIL resize) of each raw image, mirrored where flagged -- what load_image_gt makes on the host."""
    from image_captioning_amd import utils
    out = []
    for im, flip in zip(raw.images, raw.flips):
        nh, nw, window = utils.resize_geometry(im.shape, min_dim, max_dim, True)[:3]
        c = R.padded(R.pil_resize(im, nh, nw), max_dim, max_dim, window[0], window[1])
        out.append(c[:, ::-1] if flip else c)
    return np.stack(out)
