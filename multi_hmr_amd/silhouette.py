"""Fit persons to instance-segmentation masks: exact distance maps and the silhouette term (``csrc/silhouette.hip``, include/mhmr.h
``mhmr_distance_transform_desc`` and ``mhmr_silhouette_desc``: the contracts).  There is no CPU path.

The rasteriser (``raster.py``) holds the keys fixed, so a body that is too wide, too narrow or shifted sideways gets no signal from
``depth_loss``.  ``silhouette_loss`` is the classical pair of one-sided distances of SMPLify-style fitting, without soft
rasterisation: ``outside`` (the model's vertices should project inside the mask: the distance map of the mask, sampled at every
projected vertex) and ``uncovered`` (the mask should be covered by the model: every mask pixel the mesh does not cover pulls the
nearest projected vertex).  The assignments and the cover are held fixed, as the correspondences of ICP, and the values are
differentiated in closed form:

    d = model.decode_readout(readout, offset, idx, K)
    s = silhouette_loss(d["v3d"], idx[0], K, faces, masks)
    (prior + s.loss.sum()).backward()

``distance_transform`` is the exact integer transform the term is built on, useful on its own (mask dilation, truncated distance
fields from ``render_maps(...).person``); ``assign_instance_masks`` turns a segmenter's unordered instances into per-person masks.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import maps as _maps
from . import render as _render


def distance_transform(mask, max_dist: int = 0):
    """(dist2, nearest) int32 of a ``[..., H, W]`` bool / uint8 cuda tensor (nonzero = on): the squared Euclidean distance of every
    pixel to the nearest on-pixel of its own map and that pixel's linear index ``y * W + x`` (the smallest among all nearest ones).
    ``max_dist`` = R > 0 caps the search: beyond R pixels ``dist2`` is R R + 1 and ``nearest`` -1; with R = 0 a map without on-pixel
    has ``dist2`` 0x7fffffff and ``nearest`` -1.  Exact integers, the same on every call (include/mhmr.h).  Each pixel scans its row
    outward until the distance found or ``max_dist`` stops it, so with the default R = 0 a map with very few on-pixels costs up to W reads
    per pixel: give a cap where one is known."""
    if not (torch.is_tensor(mask) and mask.is_cuda and mask.dim() >= 2 and mask.dtype in (torch.bool, torch.uint8)):
        raise ValueError("mask must be a bool or uint8 cuda tensor [..., H, W]")
    R = int(max_dist)
    H, W = int(mask.shape[-2]), int(mask.shape[-1])
    if not (1 <= H <= _lib.DISTANCE_MAX_SIDE and 1 <= W <= _lib.DISTANCE_MAX_SIDE):
        raise ValueError(f"H and W must lie in [1, {_lib.DISTANCE_MAX_SIDE}], got {H} x {W}")
    if not 0 <= R <= _lib.DISTANCE_MAX_R:
        raise ValueError(f"max_dist must lie in [0, {_lib.DISTANCE_MAX_R}], got {max_dist}")
    dev = mask.device
    src = mask.contiguous().view(torch.uint8)
    dist2 = torch.empty(mask.shape, dtype=torch.int32, device=dev)
    nearest = torch.empty(mask.shape, dtype=torch.int32, device=dev)
    d = _lib.DistanceTransformDesc()
    d.N, d.H, d.W, d.max_dist = src.numel() // (H * W), H, W, R
    if d.N:
        with torch.cuda.device(dev):
            nbytes = _lib.workspace_bytes("mhmr_distance_transform_workspace_bytes", C.byref(d))
            ws = _render._workspace(nbytes, dev)
            d.src, d.dist2, d.nearest, d.workspace, d.workspace_bytes = src.data_ptr(), dist2.data_ptr(), nearest.data_ptr(), ws.data_ptr(), nbytes
            _lib.check(_lib.lib().mhmr_distance_transform(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "mhmr_distance_transform")
    return dist2, nearest


class Silhouette(NamedTuple):
    """The result of ``silhouette_loss``, one entry per person."""
    loss: torch.Tensor               # float32 [P], autograd: weights[0] * outside + weights[1] * uncovered
    outside: torch.Tensor            # float32 [P], autograd
    uncovered: torch.Tensor          # float32 [P], autograd
    outside_vertices: torch.Tensor   # int32 [P]: projected vertices off the allowed region
    uncovered_px: torch.Tensor       # int32 [P]: mask pixels the mesh does not cover (within max_dist of a projected vertex)


def _desc(B, H, W, P, V, F):
    d = _lib.SilhouetteDesc()
    d.B, d.H, d.W, d.P, d.V, d.F, d.vstride = B, H, W, P, V, F, 3 * V
    return d


def pass_bytes(size, V, F) -> int:
    """The workspace ``silhouette_loss`` needs to take ONE person per pass: the smallest ``max_workspace_bytes`` it accepts."""
    return _lib.workspace_bytes("mhmr_silhouette_workspace_bytes", C.byref(_desc(1, int(size[0]), int(size[1]), 1, int(V), int(F))), 1)


class _Silhouette(torch.autograd.Function):
    """outside, uncovered = f(verts): the forward calls mhmr_silhouette once and keeps the gradient of each term; the backward scales
    the two by the per-person cotangents."""

    @staticmethod
    def forward(ctx, verts, call):
        v = _maps._strided(verts, call["dev"], "verts")
        dev, P, V = call["dev"], call["P"], int(v.shape[1])
        terms = torch.zeros((P, 2), dtype=torch.float64, device=dev)
        counts = torch.zeros((P, 2), dtype=torch.int32, device=dev)
        g = torch.zeros((2, P, V, 3), dtype=torch.float32, device=dev)
        if P:
            d = _desc(call["B"], call["H"], call["W"], P, V, call["F"])
            d.verts, d.vstride = v.data_ptr(), (int(v.stride(0)) if P > 1 else 3 * V)
            d.faces, d.image_index, d.K, d.Rt = call["faces"].data_ptr(), call["idx"].data_ptr(), call["K"].data_ptr(), _lib.ptr(call["Rt"])
            d.znear, d.zfar, d.cull_back = _render.ZNEAR, _render.ZFAR, int(call["cull_back"])
            d.mask, d.allowed = call["mask"].data_ptr(), _lib.ptr(call["allowed"])
            d.sigma, d.robust, d.max_dist = call["sigma"], call["robust"], call["max_dist"]
            d.terms, d.counts, d.g_verts = terms.data_ptr(), counts.data_ptr(), g.data_ptr()
            need = lambda n: _lib.workspace_bytes("mhmr_silhouette_workspace_bytes", C.byref(d), n)
            one = need(1)
            n = max(1, min(P, (call["max_workspace_bytes"] - 256) // (one - 256)))
            with torch.cuda.device(dev):
                ws = _render._workspace(need(n), dev)
                d.workspace, d.workspace_bytes = ws.data_ptr(), need(n)
                _lib.check(_lib.lib().mhmr_silhouette(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "mhmr_silhouette")
        ctx.save_for_backward(g)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(counts)
        return terms[:, 0].float(), terms[:, 1].float(), counts

    @staticmethod
    def backward(ctx, g_outside, g_uncovered, _):
        g, = ctx.saved_tensors
        out = None
        for k, cot in enumerate((g_outside, g_uncovered)):
            if cot is not None:
                part = g[k] * cot.to(torch.float32).reshape(-1, 1, 1)
                out = part if out is None else out + part
        return out, None


def silhouette_loss(verts, image_index, K, faces, masks, size=None, Rt=None, ignore="others", sigma=8.0, robust="gmof", max_dist=64,
                    weights=(1.0, 1.0), cull_back=True, max_workspace_bytes=256 << 20) -> Silhouette:
    """The silhouette term of P meshes sharing one face array against one segmentation mask per person; the scene is given as to
    ``raster.rasterize`` with one view: verts [P, V, 3] cuda float32 (a strided ``v3d`` block is read in place), image_index [P],
    K [B, 3, 3], faces [F, 3], Rt None / [B, 3, 4].  masks: [P, H, W] bool / uint8 on the same device; ``size`` defaults to its (H, W).

    ``outside`` = sum over the projected vertices of rho(phi^2 / sigma^2), phi = the distance (pixels, bilinear, capped at
    ``max_dist``) from the vertex to the region the person may project into; ``uncovered`` = sum over the mask pixels the mesh does
    not cover of |nearest projected vertex - pixel centre|^2 / sigma^2 (pixels farther than ``max_dist`` from every vertex are left
    out).  include/mhmr.h ``mhmr_silhouette_desc`` has every rule.  ignore: what a person may project into besides its own mask:
    "others" = the other persons' masks of the same image (the person may be occluded by them), None = nothing, or a [B, H, W] tensor =
    a region of each image every person may project into (an occluder, a "don't know" region).  robust: "gmof" or "l2" for ``outside``.
    ``sigma``, ``max_dist`` and ``weights`` are CONVENTIONS in pixels, not measurements.

    The result is differentiable with respect to ``verts`` with the assignments and the cover held fixed; one kernel call in the
    forward, none in the backward.  The workspace stays within ``max_workspace_bytes`` whatever P is (``pass_bytes`` is the floor)."""
    if not (torch.is_tensor(verts) and verts.is_cuda and verts.dim() == 3 and verts.shape[-1] == 3):
        raise ValueError("verts must be a cuda tensor [P, V, 3]")
    if robust not in _lib.FIT_ROBUST:
        raise ValueError(f"robust must be one of {sorted(_lib.FIT_ROBUST)}, not {robust!r}")
    dev = verts.device
    P, V = int(verts.shape[0]), int(verts.shape[1])
    if not (torch.is_tensor(masks) and masks.dim() == 3 and masks.shape[0] == P and masks.dtype in (torch.bool, torch.uint8)):
        raise ValueError(f"masks must be a bool or uint8 tensor [{P}, H, W]")
    H, W = (int(masks.shape[1]), int(masks.shape[2])) if size is None else (int(size[0]), int(size[1]))
    if tuple(masks.shape[1:]) != (H, W):
        raise ValueError(f"masks are {tuple(masks.shape[1:])}, size is {(H, W)}")
    if not (float(sigma) > 0 and np.isfinite(float(sigma))) or not 1 <= int(max_dist) <= _lib.DISTANCE_MAX_R or len(weights) != 2:
        raise ValueError("sigma must be positive, max_dist an integer >= 1, weights a pair")
    idx = torch.as_tensor(image_index).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if idx.numel() != P:
        raise ValueError(f"image_index has {idx.numel()} entries for {P} meshes")
    Kt = torch.as_tensor(K, dtype=torch.float32).to(dev).reshape(-1, 3, 3).contiguous()
    B = int(Kt.shape[0])
    Rtt = None
    if Rt is not None:
        Rtt = torch.as_tensor(Rt, dtype=torch.float32).to(dev).contiguous()
        if tuple(Rtt.shape) != (B, 3, 4):
            raise ValueError(f"Rt must be [{B}, 3, 4], got {tuple(Rtt.shape)}")
    mask = masks.to(dev).contiguous().view(torch.uint8)
    allowed = None
    if isinstance(ignore, str):
        if ignore != "others":
            raise ValueError(f'ignore must be "others", None or a [B, H, W] tensor, not {ignore!r}')
        on = (mask != 0)
        ok = (idx >= 0) & (idx < B)
        union = torch.zeros((B, H, W), dtype=torch.int32, device=dev)
        union.index_add_(0, idx[ok].long(), on[ok].to(torch.int32))                 # per image: how many masks hold the pixel
        others = union[idx.clamp(0, B - 1).long()] - on.to(torch.int32)             # minus one's own
        allowed = (on | ((others > 0) & ok.reshape(-1, 1, 1))).to(torch.uint8)
    elif ignore is not None:
        region = torch.as_tensor(ignore).to(dev)
        if tuple(region.shape) != (B, H, W):
            raise ValueError(f"ignore must be [{B}, {H}, {W}], got {tuple(region.shape)}")
        ok = (idx >= 0) & (idx < B)
        allowed = ((mask != 0) | ((region != 0)[idx.clamp(0, B - 1).long()] & ok.reshape(-1, 1, 1))).to(torch.uint8)
    f_host = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
    F = int(f_host.shape[0])
    one = pass_bytes((H, W), V, F)
    if int(max_workspace_bytes) < one:
        raise ValueError(f"max_workspace_bytes = {max_workspace_bytes} is below the {one} bytes of one person per pass")
    call = dict(dev=dev, B=B, H=H, W=W, P=P, F=F, idx=idx, K=Kt, Rt=Rtt, faces=_render._faces_on(f_host, V, dev)[0], mask=mask, allowed=allowed,
                sigma=float(sigma), robust=_lib.FIT_ROBUST[robust], max_dist=int(max_dist), cull_back=bool(cull_back),
                max_workspace_bytes=int(max_workspace_bytes))
    outside, uncovered, counts = _Silhouette.apply(verts, call)
    return Silhouette(float(weights[0]) * outside + float(weights[1]) * uncovered, outside, uncovered, counts[:, 0], counts[:, 1])


def assign_instance_masks(person_map, image_index, instances):
    """Give each person the segmenter's instance that fits its rendered region best.  person_map [B, H, W] int (``render_maps(...)
    .person``: -1 = background), image_index [P], instances [B, M, H, W] bool.  Pairs (person, instance of the person's image) are
    matched greedily by IoU in descending order, ties to the lower (person, instance) pair, each person and each instance at most
    once; an IoU of 0 never matches.  Returns (masks [P, H, W] bool, matched [P] int64: the instance, -1 = none; an unmatched
    person's mask is empty).  Plain torch."""
    person_map, instances = torch.as_tensor(person_map), torch.as_tensor(instances)
    dev = instances.device
    if instances.dim() != 4 or person_map.dim() != 3 or tuple(person_map.shape) != (instances.shape[0],) + tuple(instances.shape[2:]):
        raise ValueError("person_map must be [B, H, W] and instances [B, M, H, W]")
    B, M, H, W = (int(s) for s in instances.shape)
    idx = torch.as_tensor(image_index).to(dev).long().reshape(-1)
    P = int(idx.numel())
    masks = torch.zeros((P, H, W), dtype=torch.bool, device=dev)
    if P == 0 or M == 0:
        return masks, torch.full((P,), -1, dtype=torch.long, device=dev)
    ok = (idx >= 0) & (idx < B)
    b = idx.clamp(0, B - 1)
    own = (person_map.to(dev)[b] == torch.arange(P, device=dev).reshape(-1, 1, 1)) & ok.reshape(-1, 1, 1)        # [P, H, W]
    inst = instances.bool()
    own_px = own.flatten(1).sum(-1).double()
    iou = np.zeros((P, M))
    for m in range(M):                                                       # one instance slot at a time: nothing [P, M, H, W] is formed
        im = inst[b, m]                                                      # [P, H, W]: slot m of each person's image
        inter = (own & im).flatten(1).sum(-1).double()
        union = own_px + im.flatten(1).sum(-1).double() - inter
        iou[:, m] = torch.where(union > 0, inter / union.clamp(min=1), torch.zeros_like(inter)).cpu().numpy()
    b_host = b.cpu().numpy()
    order = np.argsort(-iou.reshape(-1), kind="stable")                      # descending IoU, ties to the lower (person, instance)
    matched, taken = [-1] * P, set()
    for o in order:
        p, m = divmod(int(o), M)
        if iou[p, m] <= 0:
            break
        if matched[p] >= 0 or (int(b_host[p]), m) in taken:
            continue
        matched[p] = m
        taken.add((int(b_host[p]), m))
        masks[p] = inst[int(b_host[p]), m]
    return masks, torch.tensor(matched, dtype=torch.long, device=dev)
