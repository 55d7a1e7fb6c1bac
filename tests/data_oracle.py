"""Oracle of the training-data tests: the reference's image operations restated from Pillow's public calls (datasets/bedlam.py:216-242:
convert, rotate(-90, expand=True) for a closeup, ImageOps.mirror for a flip, ImageOps.contain, ImageOps.pad, normalize_rgb), and readers
of tests/golden/data_pipeline.npz (tests/golden/make_golden_data.py: the reference's own readers run on a synthetic fixture set)."""
import functools
import os
import pickle

import numpy as np
from PIL import Image, ImageOps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_pipeline.npz")
MIRROR, ROT90 = 1, 2
IMG_NORM_MEAN, IMG_NORM_STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def pil_oriented(arr, orient):
    """The oriented image as the reference makes it, in its order: the rotation, then the mirror."""
    img = Image.fromarray(arr)
    if orient & ROT90:
        img = img.rotate(-90, expand=True)
    if orient & MIRROR:
        img = ImageOps.mirror(img)
    return img


def pil_x(arr, orient, S):
    """[3, S, S] float32: what the reference's ``__getitem__`` returns for the decoded image ``arr`` [H, W, 3] uint8."""
    img = ImageOps.pad(ImageOps.contain(pil_oriented(arr, orient), (S, S)), size=(S, S))
    a = np.transpose(np.asarray(img).astype(np.float32) / 255., (2, 0, 1))
    a = (a - np.asarray(IMG_NORM_MEAN).reshape(3, 1, 1)) / np.asarray(IMG_NORM_STD).reshape(3, 1, 1)
    return a.astype(np.float32)


def orient_index_map(H, W, orient):
    """``(ys, xs)`` with ``oriented = src[ys, xs]`` for a stored ``[H, W]`` image: bit 1 of ``orient`` rotates by 90 degrees clockwise
    (``img.rotate(-90, expand=True)`` = ``Transpose.ROTATE_270``), bit 0 mirrors AFTER the rotation (``ImageOps.mirror``) -- the index
    map ``mhmr_preprocess_u8_batch_oriented`` reads through."""
    oW, oH = (H, W) if orient & ROT90 else (W, H)
    y, x = np.meshgrid(np.arange(oH), np.arange(oW), indexing="ij")
    if orient & MIRROR:
        x = oW - 1 - x
    return (H - 1 - x, y) if orient & ROT90 else (y, x)


def host_oriented(arr, orient):
    """The same orientation with numpy: np.rot90 clockwise, then a flip of the columns."""
    a = np.rot90(arr, k=-1) if orient & ROT90 else arr
    return np.ascontiguousarray(a[:, ::-1] if orient & MIRROR else a)


def make_image(H, W, seed=0):
    g = np.random.default_rng(seed + 1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([xx * 255.0 / max(W - 1, 1), yy * 255.0 / max(H - 1, 1), (3 * xx + 5 * yy) % 256], -1)
    return np.clip(0.5 * base + 0.5 * g.integers(0, 256, (H, W, 3)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def annotations(name):
    """``(annots, pixels)`` of dataset ``name`` as the generator made them: the annotation dict of the reference's format (fresh
    arrays on every call) and ``{imagename: uint8 [H, W, 3]}``."""
    g, annots, pixels, i = golden(), {}, {}, 0
    while f"{name}/annot/{i}/name" in g:
        p = f"{name}/annot/{i}/"
        humans = []
        for j in range(int(g[p + "n_humans"])):
            q = p + f"h{j}/"
            humans.append({k[len(q):]: (str(v) if v.dtype.kind == "U" else v.copy()) for k, v in g.items() if k.startswith(q)})
        n = str(g[p + "name"])
        annots[n] = {"focal": g[p + "focal"].copy(), "princpt": g[p + "princpt"].copy(), "size": g[p + "size"].copy(), "humans": humans}
        pixels[n] = g[f"{name}/pixels/{i}"]
        i += 1
    return annots, pixels


def batch(tag):
    """``(x, y)`` of the recorded batch ``tag`` ("bedlam/val_all", "bedlam/train_<seed>", "3dpw/all", ...), numpy arrays."""
    g, p = golden(), tag + "/y/"
    return g[tag + "/x"], {k[len(p):]: v for k, v in g.items() if k.startswith(p)}


def write_files(name, root, splits, image_subdir):
    """The pickle(s) and PNG files of dataset ``name`` under ``root``, laid out as the reference expects them -> the annotation folder."""
    annots, pixels = annotations(name)
    for split in splits:
        with open(os.path.join(root, f"{name}_{split}.pkl"), "wb") as f:
            pickle.dump(annots, f)
    for sub in image_subdir:
        for n, p in pixels.items():
            path = os.path.join(root, sub, n)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            Image.fromarray(p).save(path)
    return root
