"""GPU input preprocessing: the step in front of ``Model.forward``.

Drop-in for the reference's ``demo.open_image`` (``demo.py:27-51``) with the resize / pad / normalise done by
``mhmr_preprocess_u8`` on the device, plus a batched ``get_camera_parameters`` (``demo.py:53-68``).  Image *decoding*
(JPEG/PNG -> uint8 RGB) stays with PIL on the host, as in the reference.

Host side = table construction only (a few KB per image size, cached):
  * ``contain_size`` / ``pad_offsets``: the geometry of ``ImageOps.contain`` + ``ImageOps.pad`` (Pillow, a dependency of the
    reference: ``requirements.txt``), restated from Pillow's documented behaviour;
  * ``resample_coeffs``: Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the bicubic filter (a = -0.5,
    support 2, widened by the down-scale factor; float64 weights normalised to 1, then quantised to 22 fractional bits);
  * ``norm_lut``: ``utils/image.py:12-24`` evaluated on the 256 possible byte values.
``tests/test_preprocess.py`` holds these bit-exact against the installed Pillow itself."""
from __future__ import annotations

import ctypes
import math
import threading
from functools import lru_cache

import numpy as np
import torch

from . import _lib

IMG_NORM_MEAN = [0.485, 0.456, 0.406]           # reference utils/image.py:9-10
IMG_NORM_STD = [0.229, 0.224, 0.225]
PRECISION_BITS = 32 - 8 - 2                     # Pillow's 8 bpc fixed point


def contain_size(W: int, H: int, S: int) -> tuple[int, int]:
    """Output (width, height) of ``ImageOps.contain(img, (S, S))`` (demo.py:40)."""
    im_ratio, dest_ratio = W / H, 1.0
    ow, oh = S, S
    if im_ratio != dest_ratio:
        if im_ratio > dest_ratio:
            nh = round(H / W * S)
            if nh != S:
                oh = nh
        else:
            nw = round(W / H * S)
            if nw != S:
                ow = nw
    return ow, oh


def pad_offsets(ow: int, oh: int, S: int) -> tuple[int, int]:
    """Paste position of ``ImageOps.pad(.., (S, S))`` with the default centring (demo.py:44)."""
    if (ow, oh) == (S, S):
        return 0, 0
    if ow != S:
        return round((S - ow) * 0.5), 0
    return 0, round((S - oh) * 0.5)


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@lru_cache(maxsize=256)
def resample_coeffs(in_size: int, out_size: int):
    """Pillow's coefficient tables for resizing ``in_size`` -> ``out_size`` samples with the bicubic filter over the whole
    axis.  Returns (kk int32 [out_size, ksize], bounds int32 [out_size, 2] = (first tap, tap count), ksize)."""
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return kk, bounds, ksize


def norm_lut() -> np.ndarray:
    """[3, 256] float32: ``normalize_rgb`` (utils/image.py:12-24) of every byte value, with the reference's own arithmetic
    (float32 divide by 255, float64 mean / std broadcast, cast back to float32)."""
    v = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)        # (W=1, H=256, 3)
    img = v.astype(np.float32) / 255.
    img = np.transpose(img, (2, 0, 1))
    img = (img - np.asarray(IMG_NORM_MEAN).reshape(3, 1, 1)) / np.asarray(IMG_NORM_STD).reshape(3, 1, 1)
    return np.ascontiguousarray(img.astype(np.float32).reshape(3, 256))


class Preprocessor:
    """``pre = Preprocessor(img_size, device); x = pre(img_u8)`` with ``img_u8`` a uint8 ``[H, W, 3]`` RGB tensor (host or
    device) -> ``[1, 3, S, S]`` float32 on the device, bit-identical to ``demo.open_image``'s tensor.  Asynchronous on the
    current stream; coefficient tables are cached per source size.  ``pre.batch([img_u8, ...])`` does the same for a list of images
    of any sizes in two launches and one host-to-device copy -> ``[B, 3, S, S]``, the tensor ``Model.forward`` takes."""

    def __init__(self, img_size: int, device=torch.device("cuda")):
        self.S = int(img_size)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MhmrError("Preprocessor needs a HIP device: there is no CPU fallback")
        self.lut = torch.from_numpy(norm_lut()).to(self.device)
        self._tables = {}
        # batch(): two pinned staging buffers used in turn (descriptors + the host images of one call; the event says when the copy
        # out of it has run), their device copy, and the workspace the images' tmp slices are carved from; all grow on demand
        self._pinned = [[None, None], [None, None]]
        self._turn = 0
        self._staging = self._tmp = None
        self._batch_lock = threading.Lock()

    def _plan(self, H: int, W: int):
        key = (H, W)
        if key not in self._tables:
            if H > W * 100:
                raise ValueError("images taller than 100x their width take a different pass order in PIL; not supported")
            S = self.S
            ow, oh = contain_size(W, H, S)
            px, py = pad_offsets(ow, oh, S)
            kh, bh, ksh = resample_coeffs(W, ow)
            kv, bv, ksv = resample_coeffs(H, oh)
            y0 = int(bv[0, 0])
            rows = int(bv[-1, 0] + bv[-1, 1]) - y0
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            self._tables[key] = dict(ow=ow, oh=oh, px=px, py=py, kh=dev(kh), bh=dev(bh), ksh=ksh, kv=dev(kv), bv=dev(bv), ksv=ksv,
                                     y0=y0, rows=rows, tmp=torch.empty(rows * ow * 3, dtype=torch.uint8, device=self.device))
        return self._tables[key]

    def __call__(self, img_u8: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3:
            raise ValueError("expected a uint8 [H, W, 3] RGB image")
        img = img_u8.to(self.device, non_blocking=True).contiguous()
        H, W = int(img.shape[0]), int(img.shape[1])
        t = self._plan(H, W)
        S = self.S
        if out is None:
            out = torch.empty(1, 3, S, S, dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.numel() == 3 * S * S and out.dtype == torch.float32
        st = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(_lib.lib().mhmr_preprocess_u8(img.data_ptr(), H, W, t["kh"].data_ptr(), t["bh"].data_ptr(), t["ksh"], t["kv"].data_ptr(),
                                                 t["bv"].data_ptr(), t["ksv"], t["ow"], t["oh"], t["y0"], t["rows"], S, t["px"], t["py"],
                                                 self.lut.data_ptr(), t["tmp"].data_ptr(), out.data_ptr(), st), "mhmr_preprocess_u8")
        return out

    def batch(self, images, out: torch.Tensor | None = None) -> torch.Tensor:
        """``images``: a list of uint8 ``[H, W, 3]`` RGB tensors of any sizes, on the host, on the device or mixed -> ``[B, 3, S, S]``
        float32 on the device (written into ``out`` if given), image b bit-identical to ``self(images[b])``.  One
        ``mhmr_preprocess_u8_batch`` call: two launches however many images there are.  The host images and the descriptors travel in
        ONE pinned buffer and one non-blocking copy; device images are read where they are.  Asynchronous on the current stream;
        calls on one Preprocessor must all use the same stream (the staging buffers are reused in stream order).  The plan of every
        source size met stays cached (tables of a few KB and the one-image ``tmp`` of ``__call__``, rows x ow x 3 bytes): an endless
        stream of ever new sizes grows that cache; use a new Preprocessor per source, or clear ``_tables``, there."""
        B = len(images)
        if B == 0 or B > 65535:
            raise ValueError("expected 1 ... 65535 images")
        for img in images:
            if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
                raise ValueError("expected a uint8 [H, W, 3] RGB image")
        with self._batch_lock:
            return self._stage(images, None, out)

    def _stage(self, images, orient, out):
        """What ``batch`` (``orient`` None: ``PreImage`` descriptors, ``mhmr_preprocess_u8_batch``) and ``batch_oriented`` (``PreImageO``,
        ``mhmr_preprocess_u8_batch_oriented``) share: plans, staging layout, the pinned buffers used in turn, descriptors, the one copy
        and the launch.  The caller holds ``_batch_lock`` and has checked ``images`` and ``orient``."""
        B, S, dev = len(images), self.S, self.lut.device     # (the device with its index: self.device may be a bare "cuda")
        Desc, entry = (_lib.PreImage, "mhmr_preprocess_u8_batch") if orient is None else (_lib.PreImageO, "mhmr_preprocess_u8_batch_oriented")
        # the plan is keyed by (H, W) of the ORIENTED image: a rotated source's rows are the stored columns
        rot = [False] * B if orient is None else [bool(o & _lib.ORIENT_ROT90) for o in orient]
        plans = [self._plan(*((int(img.shape[1]), int(img.shape[0])) if r else (int(img.shape[0]), int(img.shape[1])))) for img, r in zip(images, rot)]
        if out is None:
            out = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
        if not (out.is_contiguous() and out.numel() == B * 3 * S * S and out.dtype == torch.float32 and out.device == dev):
            raise ValueError(f"out must be a contiguous float32 tensor of {B} x 3 x {S} x {S} elements on {dev}")
        up = lambda n: -(-n // 256) * 256
        # layout of the staging buffer: [B descriptors][host image 0][host image 1] ...; of the workspace: [tmp 0][tmp 1] ...
        off, img_off, tmp_off, tmp_bytes = up(B * ctypes.sizeof(Desc)), [], [], 0
        for img, t in zip(images, plans):
            img_off.append(None if img.is_cuda else off)
            if not img.is_cuda:
                off += up(img.numel())
            tmp_off.append(tmp_bytes)
            tmp_bytes += up(t["rows"] * t["ow"] * 3)
        slot = self._pinned[self._turn]
        self._turn ^= 1
        if slot[1] is not None:
            slot[1].synchronize()                      # the copy out of this buffer two calls ago
        if slot[0] is None or slot[0].numel() < off:
            slot[0] = torch.empty(off + off // 4, dtype=torch.uint8, pin_memory=True)
        if self._staging is None or self._staging.numel() < off:
            self._staging = torch.empty(off + off // 4, dtype=torch.uint8, device=dev)
        if self._tmp is None or self._tmp.numel() < tmp_bytes:
            self._tmp = torch.empty(tmp_bytes + tmp_bytes // 4, dtype=torch.uint8, device=dev)
        pin, staging = slot[0], self._staging
        desc, keep = (Desc * B)(), []
        for b, (img, t) in enumerate(zip(images, plans)):
            d, H, W = desc[b], int(img.shape[0]), int(img.shape[1])
            if img.is_cuda:
                img = img.to(dev).contiguous()
                keep.append(img)
                d.img = img.data_ptr()
            else:
                pin[img_off[b]:img_off[b] + img.numel()].view(H, W, 3).copy_(img)
                d.img = staging.data_ptr() + img_off[b]
            d.H, d.W, d.ow, d.oh, d.y0, d.rows, d.pad_x, d.pad_y, d.ksh, d.ksv = (H, W, t["ow"], t["oh"], t["y0"], t["rows"], t["px"],
                                                                                 t["py"], t["ksh"], t["ksv"])
            d.kh, d.bh, d.kv, d.bv = t["kh"].data_ptr(), t["bh"].data_ptr(), t["kv"].data_ptr(), t["bv"].data_ptr()
            d.tmp = self._tmp.data_ptr() + tmp_off[b]
            if orient is not None:
                d.orient = orient[b]
        pin[:ctypes.sizeof(desc)].copy_(torch.frombuffer(desc, dtype=torch.uint8))
        with torch.cuda.device(dev):
            staging[:off].copy_(pin[:off], non_blocking=True)
            if slot[1] is None:
                slot[1] = torch.cuda.Event()
            slot[1].record()
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(getattr(_lib.lib(), entry)(desc, staging.data_ptr(), B, S, self.lut.data_ptr(), out.data_ptr(), st), entry)
        del keep                                       # device inputs made contiguous here: freed in stream order, after the kernels
        return out.view(B, 3, S, S)

    def batch_oriented(self, images, orient, out: torch.Tensor | None = None) -> torch.Tensor:
        """``batch`` for sources that are to be rotated and / or mirrored first, as the training loaders orient them: ``orient[b]`` has
        bit 0 = mirror (``ImageOps.mirror``) and bit 1 = rotate by 90 degrees clockwise (``img.rotate(-90, expand=True)``), the mirror applied
        after the rotation.  Image b is bit-identical to ``batch`` on the oriented copy of ``images[b]``, but no such copy is made: one
        ``mhmr_preprocess_u8_batch_oriented`` call reads the stored pixels through the permutation.  Inputs (host, device or mixed),
        staging, stream rules and the plan cache are those of ``batch``; the plan of an image is keyed by its ORIENTED size."""
        B = len(images)
        orient = [int(o) for o in orient]
        if B == 0 or B > 65535 or len(orient) != B:
            raise ValueError("expected 1 ... 65535 images and one orient code per image")
        for img, o in zip(images, orient):
            if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
                raise ValueError("expected a uint8 [H, W, 3] RGB image")
            if o & ~(_lib.ORIENT_MIRROR | _lib.ORIENT_ROT90):
                raise ValueError("orient: bit 0 = mirror, bit 1 = rotate by 90 degrees clockwise")
        with self._batch_lock:
            return self._stage(images, orient, out)


_PRE = {}


def open_image(img_path, img_size, device=torch.device("cuda")):
    """Same contract as the reference's ``demo.open_image`` (demo.py:27-51) -> ``(x [1,3,S,S] float32 on device, PIL image)``;
    PIL only decodes, the resize / pad / normalise run in ``mhmr_preprocess_u8``."""
    from PIL import Image
    img_pil = Image.open(img_path).convert("RGB")
    key = (int(img_size), str(device))
    if key not in _PRE:
        _PRE[key] = Preprocessor(img_size, device)
    x = _PRE[key](torch.from_numpy(np.array(img_pil)))
    return x, img_pil.copy()


def get_camera_parameters(img_size, fov=60, p_x=None, p_y=None, device=torch.device("cuda"), batch: int = 1):
    """demo.py:53-68 for a whole batch: ``K [batch, 3, 3]``; ``p_x`` / ``p_y`` may be scalars or per-image sequences."""
    focal = img_size / (2 * np.tan(np.radians(fov) / 2))
    K = torch.eye(3).repeat(batch, 1, 1)
    K[:, 0, 0] = K[:, 1, 1] = focal
    if p_x is not None and p_y is not None:
        K[:, 0, 2] = torch.as_tensor(p_x, dtype=torch.float32) * img_size
        K[:, 1, 2] = torch.as_tensor(p_y, dtype=torch.float32) * img_size
    else:
        K[:, 0, 2] = K[:, 1, 2] = img_size // 2
    return K.to(device)
