"""Training data: annotation readers, the batch's ``y`` and a loader that yields what ``Trainer.train_n_iters`` iterates over
(DESIGN.md section 27).  Drop-in for the reference's ``datasets/bedlam.py`` / ``threedpw.py`` / ``ehf.py`` sample path and ``collate_fn``.

The split of the work is not the reference's.  There ``__getitem__`` decodes, rotates, mirrors, resizes and normalises one image with
PIL and numpy and flips the annotations person by person.  Here

* ``AnnotatedImages.sample(i)`` is host only and decodes nothing: the path, the orient code (bit 0 = mirror, bit 1 = the closeup
  rotation), K and the persons that remain, in depth order;
* the pixels of a whole batch go through ONE ``Preprocessor.batch_oriented`` call, which reads each decoded image through its
  rotation / mirror (no oriented copy) and is bit-exact against Pillow;
* ``collate`` flips, pads and casts the annotations of the batch with numpy on flat per-batch arrays inside one pinned block that is
  copied once (B x P x 179 floats: a kernel launch would be pure latency);
* ``TrainLoader`` decodes on threads, one batch ahead of the training step.

``build_dataset`` (annotation files from the raw datasets, which needs the ``smplx`` package), crops other than 0 and the JPEG
re-encoding are not part of this module."""
from __future__ import annotations

import contextlib
import math
import os
import pickle
import random
from dataclasses import dataclass, field

import numpy as np
import torch

from . import pipeline
from .preprocess import contain_size

ORIENT_MIRROR, ORIENT_ROT90 = 1, 2                      # the bits of Preprocessor.batch_oriented's orient

#: the body-pose joints a mirror exchanges (datasets/bedlam.py:290) as a permutation of the 21 joints
_BODY_PAIRS = ((0, 1), (3, 4), (6, 7), (9, 10), (12, 13), (15, 16), (17, 18), (19, 20))
_BODY_PERM = np.arange(21)
for _a, _b in _BODY_PAIRS:
    _BODY_PERM[_a], _BODY_PERM[_b] = _b, _a
#: keys whose axis-angle rows change sign in y and z under a mirror, and the key each one is stored under afterwards
_FLIP_POSE = {"smplx_root_pose": "smplx_root_pose", "smplx_jaw_pose": "smplx_jaw_pose", "smplx_body_pose": "smplx_body_pose",
              "smplx_left_hand_pose": "smplx_right_hand_pose", "smplx_right_hand_pose": "smplx_left_hand_pose",
              "smplx_leye_pose": "smplx_reye_pose", "smplx_reye_pose": "smplx_leye_pose"}


@dataclass
class Sample:
    """One drawn image: what ``collate`` and ``Preprocessor.batch_oriented`` need, nothing decoded."""
    imagename: str
    path: str
    orient: int                                          # ORIENT_* bits
    K: np.ndarray                                        # [3, 3] float64, of the img_size x img_size input (mirrored if the image is)
    humans: list = field(default_factory=list)           # the persons that remain, in order; NOT yet flipped (collate does that)
    index: int = 0                                       # position in the dataset's imagenames

    @property
    def flip(self):
        return bool(self.orient & ORIENT_MIRROR)

    @property
    def filename(self):                                  # how pipeline.describe names the sample in a decoding error
        return self.path


class AnnotatedImages:
    """A set of images with the annotation format the reference's datasets share:
    ``{imagename: {"focal": [2], "princpt": [2], "size": [width, height], "humans": [{key: ndarray | str, ...}, ...]}}``.

    ``annots``: that dict or the path of a pickle of it; ``image_dir``: where the image names are relative to.  The rules that differ
    between the datasets are arguments: ``camera`` ("scale": focal / (max(size) / img_size), datasets/bedlam.py:208-213; "fov": through the
    field of view of the padded image, threedpw.py:191-202), ``depth_rules`` (in training drop persons with ``transl_z <= 0.01``; always
    sort by depth, stably), ``rotate_closeup``, ``flip`` (mirror half of the training samples), ``gender`` = (source key, id key, {name: id}).
    In training ``sample`` ignores its index and draws image, flip and crop from ``rng`` in the reference's order, so a seeded run picks what
    the reference picks under ``random.seed``."""

    def __init__(self, annots, image_dir, img_size=512, name="images", split="test", training=False, n_iter=None, subsample=1, n=-1,
                 extension="png", res=None, camera="fov", depth_rules=False, rotate_closeup=False, flip=0, crops=(0,), gender=None, seed=None):
        if isinstance(annots, (str, bytes, os.PathLike)):
            with open(annots, "rb") as f:
                annots = pickle.load(f)
        if extension not in ("png", "jpg"):
            raise ValueError("extension is 'png' or 'jpg'")
        if camera not in ("scale", "fov"):
            raise ValueError("camera is 'scale' or 'fov'")
        if extension == "jpg":                           # datasets/bedlam.py:67-78: the annotation keys follow the re-encoded files
            annots = {(k[:-3] + "jpg" if res is None else k[:-4] + f"_{res}.jpg"): v for k, v in annots.items()}
        self.annots, self.image_dir, self.img_size, self.name, self.split = annots, image_dir, img_size, name, split
        self.training, self.n_iter, self.subsample, self.crops, self.flip = training, n_iter, subsample, list(crops), flip
        self.camera, self.depth_rules, self.rotate_closeup, self.gender = camera, depth_rules, rotate_closeup, gender
        self.rng = random.Random(seed)
        self.imagenames = sorted(self.annots)
        if n >= 0:
            self.imagenames = self.imagenames[:n]
        if subsample > 1:
            self.imagenames = self.imagenames[::subsample]

    def __len__(self):
        if self.training and self.n_iter is not None:
            return self.n_iter
        return len(self.imagenames)

    def __repr__(self):
        return f"{self.name}: split={self.split} - N={len(self.imagenames)}"

    def seed(self, seed):
        self.rng.seed(seed)

    def _camera(self, annot):
        S = self.img_size
        real_width, real_height = annot["size"]
        K = np.eye(3)
        if self.camera == "scale":
            princpt = annot["princpt"].copy()
            K[[0, 1], [-1, -1]] = S * np.asarray([princpt[0] / real_width, princpt[1] / real_height])
            K[[0, 1], [0, 1]] = annot["focal"].copy() / (max([real_width, real_height]) / S)
            return K
        K[[0, 1], [-1, -1]] = S * (annot["princpt"].copy() / [real_width, real_height])
        width, height = contain_size(int(real_width), int(real_height), S)        # the size ImageOps.contain gives, before the pad
        max_size_init = real_width if width > height else real_height
        fovx = np.degrees(2 * np.arctan(max_size_init / (2 * annot["focal"][0].copy())))
        fovy = np.degrees(2 * np.arctan(max_size_init / (2 * annot["focal"][1].copy())))
        K[0, 0] = S / (2 * np.tan(np.radians(fovx) / 2))
        K[1, 1] = S / (2 * np.tan(np.radians(fovy) / 2))
        return K

    def sample(self, i, flip=None) -> Sample:
        """The ``i``-th image (in training: one drawn from ``rng``).  ``flip`` forces the mirror instead of drawing it (the draw is still
        made, so the generator stays in step)."""
        rng = self.rng
        if self.training:
            i = rng.choices(range(len(self.imagenames)))[0]
        imagename = self.imagenames[i]
        annot = self.annots[imagename]
        K = self._camera(annot)
        orient = ORIENT_ROT90 if self.rotate_closeup and "closeup" in imagename and self.split != "test" else 0
        drawn = self.flip and rng.choice([0, 1]) and self.training
        if flip is not None:
            drawn = bool(flip) and bool(self.flip) and self.training
        if drawn:
            orient |= ORIENT_MIRROR
            K[0, -1] = self.img_size - K[0, -1]
        crop = rng.choice(self.crops) if self.training else 0
        if crop != 0:
            raise NameError("only crop 0 (contain + pad) exists")
        humans = list(annot["humans"])
        if self.depth_rules:
            if self.training:
                humans = [h for h in humans if h["smplx_transl"][-1] > 0.01]     # in front of the camera
            humans = sorted(humans, key=lambda h: h["smplx_transl"][-1])         # stable, as the reference's sorted()
        if self.gender is not None:
            src, dst, ids = self.gender
            humans = [dict(h, **{dst: np.asarray(ids[h[src]])}) for h in humans]
        return Sample(imagename, os.path.join(self.image_dir, imagename), orient, K, humans, i)


def BEDLAM(split="training", training=False, img_size=512, root_dir=os.path.join("data", "BEDLAM"), n_iter=None, subsample=1, extension="png",
           crops=(0,), flip=1, res=None, n=-1, annotations_dir="data", annots=None, seed=None):
    """datasets/bedlam.py: closeup sequences are rotated, training samples are mirrored half of the time, persons behind the camera are
    dropped in training and the rest sorted by depth; every person is 'neutral' (gender id 0)."""
    assert split in ("training", "validation")
    return AnnotatedImages(annots if annots is not None else os.path.join(annotations_dir, f"bedlam_{split}.pkl"),
                           os.path.join(root_dir, split), img_size, "bedlam", split, training, n_iter, subsample, n, extension, res,
                           camera="scale", depth_rules=True, rotate_closeup=True, flip=flip, crops=crops,
                           gender=("smplx_gender", "smplx_gender_id", {"neutral": 0}), seed=seed)


def THREEDPW(split="test", training=False, img_size=512, root_dir=os.path.join("data", "3DPW"), subsample=1, annotations_dir="data",
             annots=None, **kwargs):
    """datasets/threedpw.py: no augmentation, no filter, no sort; SMPL genders male = 1, female = 2."""
    assert split in ("test",)
    return AnnotatedImages(annots if annots is not None else os.path.join(annotations_dir, f"3dpw_{split}.pkl"),
                           os.path.join(root_dir, "imageFiles"), img_size, "3dpw", split, False, None, subsample, camera="fov",
                           gender=("smpl_gender", "smpl_gender_id", {"male": 1, "female": 2}))


def EHF(split="test", training=False, img_size=512, root_dir=os.path.join("data", "EHF"), annotations_dir="data", annots=None, **kwargs):
    """datasets/ehf.py: one person per image, given as vertices; no augmentation and no gender."""
    assert split in ("test",)
    return AnnotatedImages(annots if annots is not None else os.path.join(annotations_dir, f"ehf_{split}.pkl"), root_dir, img_size, "ehf",
                           split, False, None, 1, camera="fov")


def _flip_persons(blocks, rows):
    """The mirror of datasets/bedlam.py:266-311 on the person rows ``rows`` of the flat ``[B * P, ...]`` arrays ``blocks`` (in place)."""
    if "smplx_transl" in blocks:
        blocks["smplx_transl"][rows, 0] *= -1
    flipped = {}
    for src, dst in _FLIP_POSE.items():
        if src in blocks:
            v = blocks[src][rows]
            if src == "smplx_body_pose":
                v = v[:, _BODY_PERM]
            v[..., 1:3] *= -1                            # y and z of the axis-angle
            flipped[dst] = v
    for dst, v in flipped.items():
        blocks[dst][rows] = v


def collate(samples, device=None):
    """The ``y`` of the reference's ``collate_fn`` (datasets/bedlam.py:365-426) for a list of ``Sample``: ``imagename`` (numpy strings),
    ``K [B, 3, 3]``, ``n_humans [B]``, ``valid_humans [B, P]`` and every ndarray key of the persons zero-padded to ``[B, P, *shape]``, all
    float32, P = the largest person count of the batch.  A batch without any person has no person keys and ``valid_humans [B, 0]``.
    Mirrored samples are flipped here.  Everything numeric is written into one block (pinned when ``device`` is a GPU) and copied to
    ``device`` once; the tensors of ``y`` are views of that copy."""
    B = len(samples)
    counts = [len(s.humans) for s in samples]
    P = max(counts)
    shapes = {}
    for s in samples:
        for h in s.humans:
            for k, v in h.items():
                if isinstance(v, np.ndarray):
                    shapes[k] = v.shape
    layout, total = {}, 0
    for k, shape in [("K", (B, 3, 3)), ("n_humans", (B,)), ("valid_humans", (B, P))] + [(k, (B * P,) + sh) for k, sh in shapes.items()]:
        layout[k] = (total, shape)
        total += int(np.prod(shape))
    device = torch.device(device) if device is not None else torch.device("cpu")
    block = torch.zeros(max(total, 1), dtype=torch.float32, pin_memory=device.type == "cuda")
    flat = block.numpy()
    view = {k: flat[o:o + int(np.prod(sh))].reshape(sh) for k, (o, sh) in layout.items()}
    view["K"][:] = np.stack([s.K for s in samples])
    view["n_humans"][:] = counts
    view["valid_humans"][:] = np.arange(P)[None, :] < np.asarray(counts)[:, None]
    if shapes:
        rows = np.concatenate([b * P + np.arange(n) for b, n in enumerate(counts)])
        persons = [h for s in samples for h in s.humans]
        for k in shapes:
            view[k][rows] = np.stack([h[k] for h in persons])
        flipped = np.concatenate([b * P + np.arange(n) for b, n in enumerate(counts) if samples[b].flip] + [np.zeros(0, np.int64)]).astype(np.int64)
        if flipped.size:
            _flip_persons({k: view[k] for k in shapes}, flipped)
    dev_block = block.to(device, non_blocking=True) if device.type == "cuda" else block
    y = {"imagename": np.stack([s.imagename for s in samples])}
    for k, (o, sh) in layout.items():
        y[k] = dev_block[o:o + int(np.prod(sh))].view((B, P) + tuple(sh[1:]) if k in shapes else tuple(sh))
    return y


class TrainLoader:
    """``for x, y in TrainLoader(dataset, batch_size, device)``: ``x [B, 3, S, S]`` float32 and ``y`` (``collate``) on ``device``, what
    ``Trainer.train_n_iters``, ``cache_features`` and ``evaluate`` take.  Samples are drawn in sampler order on one thread (so a seeded
    dataset draws what the reference draws), their files are decoded by PIL on ``workers`` threads (at most 16, whatever the machine shows),
    and each batch is one ``Preprocessor.batch_oriented`` call plus one ``collate``, staged while the step of the batch before it runs.
    Batches arrive in sampler order whatever the thread timing.  ``shuffle`` permutes the indices anew every epoch from ``seed``;
    ``decode`` (source path -> ``(uint8 [H, W, 3] tensor, size)``) and ``preprocessor`` can be injected."""

    def __init__(self, dataset, batch_size, device, workers=8, shuffle=False, drop_last=False, seed=None, decode=None, preprocessor=None):
        self.dataset, self.batch_size, self.device = dataset, int(batch_size), torch.device(device)
        if self.batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        self.workers, self.shuffle, self.drop_last = pipeline.clamp_workers(workers), bool(shuffle), bool(drop_last)
        self.decode = decode if decode is not None else pipeline.decode_image
        self.preprocessor = preprocessor
        self._order = random.Random(seed)

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def __iter__(self):
        if self.preprocessor is None:
            from .preprocess import Preprocessor
            self.preprocessor = Preprocessor(self.dataset.img_size, self.device)
        pre, dev = self.preprocessor, self.device
        stream = torch.cuda.current_stream(dev) if dev.type == "cuda" else None
        indices = list(range(len(self.dataset)))
        if self.shuffle:
            self._order.shuffle(indices)
        indices = indices[:len(self) * self.batch_size] if self.drop_last else indices

        def stage(items):                                # on the producer thread, on the stream of the iteration
            samples = [s for s, _ in items]
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
                return pre.batch_oriented([img for _, (img, _) in items], [s.orient for s in samples]), collate(samples, dev)

        batches = pipeline.run_batched((self.dataset.sample(i) for i in indices), lambda s: (s, self.decode(s.path)), stage,
                                       lambda staged, items: [staged] + [None] * (len(items) - 1), batch_size=self.batch_size,
                                       workers=self.workers)
        try:
            for _, _, _, staged, _ in batches:
                if staged is not None:
                    yield staged
        finally:
            batches.close()


__all__ = ["AnnotatedImages", "BEDLAM", "EHF", "Sample", "THREEDPW", "TrainLoader", "collate"]
