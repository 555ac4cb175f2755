"""PIL's 8-bit bilinear resample (ImagingResample) restated in NumPy integers, the shape pairs it is pinned to PIL on, and the expected
canvas of a resize-and-pad: what csrc/resize.hip implements, written once for the CPU and the GPU tests (imported, never collected)."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2

# (h, w) -> (new_h, new_w): up, down, mixed, identity on one axis, 21 taps, edge clamping everywhere, one source row
SHAPE_PAIRS = [((60, 80), (77, 102)), ((37, 53), (128, 96)), ((150, 201), (64, 86)), ((40, 64), (80, 64)), ((64, 40), (64, 90)),
               ((300, 17), (31, 170)), ((5, 7), (128, 128)), ((600, 800), (768, 1024)), ((1, 9), (3, 27)), ((97, 131), (96, 130))]


def coefficients(in_size, out_size):
    """Per output index: (xmin, int32 coefficients of its n taps), float64 arithmetic in the C code's order."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support, ss = 1.0 * fs, 1.0 / fs
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = []
        ww = 0.0
        for x in range(xmax - xmin):
            a = math.fabs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
            ww += w[-1]
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, np.array([int(0.5 + v * (1 << PRECISION_BITS)) for v in w], np.int32)))
    return out


def _pass(img, out_size, axis):
    """One separable pass along `axis` of a uint8 [h,w,c] array -> uint8."""
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for xx, (xmin, k) in enumerate(coefficients(src.shape[0], out_size)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, src[xmin:xmin + len(k)], axes=(0, 0))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_bilinear(img, new_h, new_w):
    """PIL.Image.fromarray(img).resize((new_w, new_h), BILINEAR): the horizontal pass into a uint8 intermediate, then the vertical."""
    return _pass(_pass(np.asarray(img), new_w, 1), new_h, 0)


def pil_resize(img, new_h, new_w):
    from PIL import Image
    bilinear = getattr(Image, "Resampling", Image).BILINEAR
    return np.asarray(Image.fromarray(img).resize((new_w, new_h), resample=bilinear))


def padded(resized, H, W, top, left):
    out = np.zeros((H, W, 3), np.uint8)
    out[top:top + resized.shape[0], left:left + resized.shape[1]] = resized
    return out
