"""Shared inputs of the Lanczos tests (tests/test_lanczos_cpu.py on the host, tests/test_gpu_preproc_exact.py on the device):
the size list, the image families, the Pillow reference and an int64 recomputation of the two passes WITHOUT the uint8 clamp."""
import numpy as np
import PIL.Image as Image

from rfx import lanczos

# (w, h, ow, oh)
SIZES = [
    (1, 1, 7, 5), (7, 5, 1, 1), (2, 3, 64, 48), (64, 48, 2, 3), (333, 217, 7, 5), (5, 7, 333, 217), (640, 480, 641, 479),
    (33, 31, 32, 32),
    (17, 9, 17, 40),          # vertical pass only
    (17, 9, 40, 9),           # horizontal pass only
    (1, 50, 3, 50), (50, 1, 50, 3),
    (1200, 13, 37, 13),       # ksize 197
    (13, 900, 13, 29), (16, 16, 15, 17),
    (21, 19, 21, 19),         # unchanged size: a copy
]
# the small ones: what the device tests run
SMALL = [(1, 1, 7, 5), (7, 5, 1, 1), (2, 3, 64, 48), (64, 48, 2, 3), (17, 9, 17, 40), (17, 9, 40, 9), (33, 31, 32, 32),
         (1200, 13, 37, 13)]
FAMILIES = ("noise", "binary", "checker", "stripes")


def image(family, h, w, c, seed=0):
    """uint8 (h, w, c).  noise: uniform bytes; binary: random 0/255; checker: one-pixel checkerboard; stripes: 3 wide x 2 high
    blocks of 0/255.  The two patterns are shifted by one per channel, so no two neighbouring channels are equal."""
    rng = np.random.RandomState(1000 + seed)
    y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    if family == "noise":
        a = rng.randint(0, 256, size=(h, w, c))
    elif family == "binary":
        a = rng.randint(0, 2, size=(h, w, c)) * 255
    elif family == "checker":
        a = ((y + x + ch) & 1) * 255
    elif family == "stripes":
        a = ((x // 3 + y // 2 + ch) & 1) * 255
    else:
        raise ValueError(family)
    return np.ascontiguousarray(a.astype(np.uint8))


def pillow(img, ow, oh):
    """PIL.Image.resize((ow, oh), LANCZOS) of a uint8 (h, w, c) array.  c = 1 / 3 as modes L / RGB; c = 2 / 4 channel by channel
    as mode L (Pillow premultiplies alpha for RGBA and LA, so those modes are another operation)."""
    c = img.shape[2]
    if c == 3:
        return np.asarray(Image.fromarray(img, "RGB").resize((ow, oh), resample=Image.LANCZOS))
    planes = [np.asarray(Image.fromarray(np.ascontiguousarray(img[:, :, k]), "L").resize((ow, oh), resample=Image.LANCZOS))
              for k in range(c)]
    return np.stack(planes, axis=2)


def unclamped(img, ow, oh):
    """The value `acc >> 22` of every output of each pass that runs, in int64 and BEFORE the clamp to 0..255, the input of the
    second pass being the clamped output of the first (as in Pillow).  -> {"h": array, "v": array} (only the passes that run)."""
    h, w, c = img.shape
    p = lanczos.plan(w, h, ow, oh)
    out = {}
    if p is None:
        return out
    half, bits = 1 << (lanczos.PRECISION_BITS - 1), lanczos.PRECISION_BITS
    cur = img.astype(np.int64)
    if p["need_h"]:
        acc = np.empty((h, ow, c), dtype=np.int64)
        for xx in range(ow):
            x0, n = p["bounds_h"][xx]
            acc[:, xx] = half + np.einsum("yjc,j->yc", cur[:, x0:x0 + n], p["kk_h"][xx, :n].astype(np.int64))
        out["h"] = acc >> bits
        cur = np.clip(out["h"], 0, 255)
    if p["need_v"]:
        acc = np.empty((oh, cur.shape[1], c), dtype=np.int64)
        for yy in range(oh):
            y0, n = p["bounds_v"][yy]
            acc[yy] = half + np.einsum("jxc,j->xc", cur[y0:y0 + n], p["kk_v"][yy, :n].astype(np.int64))
        out["v"] = acc >> bits
    return out
