"""Who owns which pixel: per-pixel person, face, depth and body-part maps, per-person visible and amodal area, occlusion, bounding
boxes and the visibility of 3D points, all read off the rasteriser's 64-bit keys on the GPU (``csrc/render_maps.hip``, include/mhmr.h
``mhmr_render_maps``, ``mhmr_render_point_visibility``, ``mhmr_render_amodal``).  There is no CPU path and nothing is copied to the host.

The rasteriser (``render.py``, contract items 1-5) decides every pixel's winner exactly: the smallest key ``(float_bits(Z) << 32) |
(person * F + face)``.  This module adds no approximation to that: every output is an integer, an fp32 copied out of a key, or a
comparison of fp64 values formed in the rasteriser's own operation order, and every reduction is an integer add / min / max, so two
calls give the same bits (the tests restate the three contracts in numpy).

* maps: ``person`` = low32 / F (-1 background), ``face`` = low32 % F (-1), ``depth`` = the key's fp32 depth (0 background, as pyrender's
  depth map), ``label`` = ``face_labels[face]`` (255 background).
* statistics per person and view: ``visible_px``, ``bbox`` (x0, y0, x1, y1 inclusive; W, H, -1, -1 when the person wins nothing),
  ``zmin`` (+inf), ``label_px`` [L].
* ``amodal_px``: the pixels the person would win alone in their image (the drawn keys of a one-person render: same face drop, cull,
  coverage and clip planes); ``occlusion = 1 - visible_px / amodal_px`` (0 where ``amodal_px == 0``): the share hidden behind others.
  Self-occlusion does not count: a person alone has occlusion 0.
* ``point_visibility`` of points [P, N, 3] (vertices, joints): 0 occluded, 1 visible, 2 projects outside the image, 3 behind znear or
  non-finite.  A point is visible when no drawn surface is nearer than it by more than ``tau`` metres: Z <= depth + tau at its pixel.
  ``tau`` is a CONVENTION, not a measurement: 0.03 m suits the mesh's own vertices (the depth map is sampled at pixel centres, the
  vertex is not, so tau absorbs the surface's slope across one pixel); for joints, which lie inside the body, pass about a limb's radius
  (0.05 - 0.10 m), otherwise every joint is "occluded" by the person's own skin.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from . import render as _render

CODE_OCCLUDED, CODE_VISIBLE, CODE_OUTSIDE, CODE_INVALID = 0, 1, 2, 3
LABEL_NONE = 255


class RenderMaps(NamedTuple):
    """The result of ``render_maps``.  With a 3-D ``Rt`` (or None) the per-pixel maps are [B, H, W] and the statistics [P, ...]; with a
    4-D ``Rt`` [B, NV, 3, 4] they are [B, NV, H, W] and [P, NV, ...].  Fields that were not asked for are None."""
    person: torch.Tensor                      # int32, -1 = background
    face: torch.Tensor                        # int32, -1 = background
    depth: torch.Tensor                       # float32, 0 = background
    label: Optional[torch.Tensor]             # uint8, 255 = background (face_labels given)
    visible_px: torch.Tensor                  # int32 [P(, NV)]
    amodal_px: Optional[torch.Tensor]         # int32 [P(, NV)] (amodal=True)
    occlusion: Optional[torch.Tensor]         # float32 [P(, NV)] (amodal=True)
    bbox: torch.Tensor                        # int32 [P(, NV), 4]: x0, y0, x1, y1 inclusive
    zmin: torch.Tensor                        # float32 [P(, NV)], +inf = wins nothing
    label_px: Optional[torch.Tensor]          # int32 [P(, NV), L] (face_labels given)
    point_visibility: Optional[torch.Tensor]  # uint8 [P(, NV), N] (points given)
    keys: torch.Tensor                        # int64 holding the uint64 keys, as render_batch / render_views return them


def part_labels(lbs_weights, faces, groups=None) -> np.ndarray:
    """Face labels uint8 [F] from skinning weights [V, J] (host, numpy): a vertex takes its dominant joint (the lowest index on a tie),
    mapped through ``groups`` (a joint -> part table of J entries) when given; a face takes the label two or three of its corners share,
    and the first corner's label when all three differ."""
    w = np.asarray(lbs_weights)
    f = np.asarray(faces, np.int64)
    if w.ndim != 2 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"lbs_weights must be [V, J] and faces [F, 3], got {w.shape} and {f.shape}")
    if f.size and (f.min() < 0 or f.max() >= w.shape[0]):
        raise ValueError(f"face indices must lie in [0, {w.shape[0]})")
    lab = np.argmax(w, axis=1)                                          # numpy's argmax returns the first maximum
    if groups is not None:
        g = np.asarray(groups, np.int64).reshape(-1)
        if g.shape[0] != w.shape[1]:
            raise ValueError(f"groups has {g.shape[0]} entries for {w.shape[1]} joints")
        lab = g[lab]
    if lab.size and (lab.min() < 0 or lab.max() >= LABEL_NONE):
        raise ValueError("labels must lie in [0, 255): 255 is the background")
    a, b, c = lab[f[:, 0]], lab[f[:, 1]], lab[f[:, 2]]
    return np.where(b == c, b, a).astype(np.uint8)                      # b == c: the majority (or all equal); otherwise a wins or all differ


def amodal_pass_bytes(size, F, nviews=1) -> int:
    """The workspace ``render_maps(amodal=True)`` needs to take ONE person per pass at this image size, face count and view count: the
    smallest ``max_workspace_bytes`` it accepts."""
    d = _lib.RenderDesc()
    d.B, d.H, d.W, d.P, d.V, d.F, d.vstride = 1, int(size[0]), int(size[1]), 1, 3, int(F), 9
    return _lib.workspace_bytes("mhmr_render_amodal_workspace_bytes", C.byref(d), int(nviews), 1)


def _strided(t, dev, what):
    """[P, N, 3] float32 on dev whose rows of one person are contiguous (any person stride: v3d / j3d blocks are read in place)."""
    if not (torch.is_tensor(t) and t.dim() == 3 and t.shape[-1] == 3):
        raise ValueError(f"{what} must be a tensor [P, N, 3]")
    t = t.detach().to(device=dev, dtype=torch.float32)
    P, N = int(t.shape[0]), int(t.shape[1])
    if P and N and (t.stride(2) != 1 or t.stride(1) != 3 or (P > 1 and t.stride(0) < 3 * N)):
        t = t.contiguous()
    return t


def render_maps(verts, image_index, K, faces, size, Rt=None, keys=None, face_labels=None, points=None, tau=0.03, amodal=True,
                max_workspace_bytes=256 << 20, cull_back=True) -> RenderMaps:
    """Maps and statistics of P meshes sharing one face array in B images of ``size`` = (H, W); the scene is given as to
    ``render.render_batch``: verts [P, V, 3] cuda float32, image_index [P], K [B, 3, 3], faces [F, 3], Rt [B, 3, 4] / None (one view
    per image) or [B, NV, 3, 4] (NV views, as ``render.render_views``).

    keys: those of an earlier ``render_batch`` / ``render_views(..., return_debug=True)`` call of the same scene ([B, H, W] or
    [B, NV, H, W] int64); None: the scene is rendered once here (over black images, which are discarded).
    face_labels: uint8 [F], every label < 255 (``part_labels``; ``Model.face_part_labels()``): adds ``label`` and ``label_px`` [.., L],
    L = largest label + 1.  points: [P, N, 3] cuda (e.g. the forward's v3d or j3d block, read in place): adds ``point_visibility`` with
    the margin ``tau`` metres (see the module text: a convention).  amodal: also ``amodal_px`` and ``occlusion``; its workspace is at most
    ``max_workspace_bytes`` whatever P is (persons are taken in passes; ``amodal_pass_bytes`` is the floor, ValueError below it).
    Everything returned is a device tensor; nothing is copied to the host."""
    if not (torch.is_tensor(verts) and verts.is_cuda and verts.dim() == 3 and verts.shape[-1] == 3):
        raise ValueError("verts must be a cuda tensor [P, V, 3]")
    dev = verts.device
    verts = _strided(verts, dev, "verts")
    P, V = int(verts.shape[0]), int(verts.shape[1])
    H, W = int(size[0]), int(size[1])
    idx = torch.as_tensor(image_index).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if idx.numel() != P:
        raise ValueError(f"image_index has {idx.numel()} entries for {P} meshes")
    Kt = torch.as_tensor(K, dtype=torch.float32).to(dev).reshape(-1, 3, 3).contiguous()
    B = int(Kt.shape[0])
    multi = Rt is not None and torch.as_tensor(Rt).dim() == 4
    Rtt = None
    if Rt is not None:
        Rtt = torch.as_tensor(Rt, dtype=torch.float32).to(dev)
        if Rtt.shape[0] != B or Rtt.shape[-2:] != (3, 4) or Rtt.dim() not in (3, 4) or (multi and Rtt.shape[1] < 1):
            raise ValueError(f"Rt must be [B, 3, 4] or [B, NV, 3, 4] with B = {B}, got {tuple(Rtt.shape)}")
        Rtt = Rtt.reshape(B, -1, 3, 4).contiguous()
    NV = int(Rtt.shape[1]) if multi else 1
    f_host = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
    F = int(f_host.shape[0])

    if keys is None:
        black = torch.zeros((B, H, W, 3), dtype=torch.uint8, device=dev)
        if multi:
            _, keys, _ = _render.render_views(black, verts, idx, Kt, f_host, Rtt, smooth=False, cull_back=cull_back, return_debug=True)
        else:
            _, keys, _ = _render.render_batch(black, verts, idx, Kt, f_host, Rt=None if Rtt is None else Rtt[:, 0], smooth=False,
                                              cull_back=cull_back, return_debug=True)
    want = (B, NV, H, W) if multi else (B, H, W)
    if not (torch.is_tensor(keys) and keys.is_cuda and keys.dtype == torch.int64 and tuple(keys.shape) == want):
        raise ValueError(f"keys must be a cuda int64 tensor {want}")
    keys = keys.contiguous()

    lab_dev, L = None, 0
    if face_labels is not None:
        lab = face_labels.detach().cpu().numpy() if torch.is_tensor(face_labels) else np.asarray(face_labels)
        if lab.shape != (F,) or lab.dtype != np.uint8 or (F and int(lab.max()) >= LABEL_NONE):
            raise ValueError(f"face_labels must be uint8 [{F}] with every label < 255")
        L = int(lab.max()) + 1 if F else 1
        lab_dev = torch.from_numpy(np.ascontiguousarray(lab)).to(dev)

    img, per = (B, NV, H, W), (P, NV)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    person, face, depth = new(img, torch.int32), new(img, torch.int32), new(img, torch.float32)
    label = new(img, torch.uint8) if L else None
    visible, bbox, zmin = new(per, torch.int32), new(per + (4,), torch.int32), new(per, torch.float32)
    label_px = new(per + (L,), torch.int32) if L else None
    amodal_px = new(per, torch.int32) if amodal else None
    vis = None
    lib = _lib.lib()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        m = _lib.RenderMapsDesc()
        m.B, m.NV, m.H, m.W, m.P, m.F, m.L = B, NV, H, W, P, F, L
        m.keys, m.image_index, m.face_label = keys.data_ptr(), _lib.ptr(idx) if P else None, _lib.ptr(lab_dev)
        m.person, m.face, m.depth, m.label = person.data_ptr(), face.data_ptr(), depth.data_ptr(), _lib.ptr(label)
        if P:
            m.visible_px, m.bbox, m.zmin, m.label_px = visible.data_ptr(), bbox.data_ptr(), zmin.data_ptr(), _lib.ptr(label_px)
        _lib.check(lib.mhmr_render_maps(C.byref(m), stream), "mhmr_render_maps")

        if points is not None:
            pts = _strided(points, dev, "points")
            if pts.shape[0] != P:
                raise ValueError(f"points has {pts.shape[0]} persons for {P} meshes")
            N = int(pts.shape[1])
            vis = new((P, NV, N), torch.uint8)
            if P and N:
                v = _lib.PointVisibilityDesc()
                v.B, v.NV, v.H, v.W, v.P, v.N = B, NV, H, W, P, N
                v.points, v.pstride = pts.data_ptr(), int(pts.stride(0)) if P > 1 else 3 * N
                v.image_index, v.K, v.view_Rt, v.keys = idx.data_ptr(), Kt.data_ptr(), _lib.ptr(Rtt), keys.data_ptr()
                v.znear, v.tau, v.out = _render.ZNEAR, float(tau), vis.data_ptr()
                _lib.check(lib.mhmr_render_point_visibility(C.byref(v), stream), "mhmr_render_point_visibility")

        if amodal and P:
            f_dev = _render._faces_on(f_host, V, dev)[0]
            d = _lib.RenderDesc()
            d.B, d.H, d.W, d.P, d.V, d.F = B, H, W, P, V, F
            d.verts, d.vstride = verts.data_ptr(), int(verts.stride(0)) if P > 1 else 3 * V
            d.faces, d.image_index, d.K = f_dev.data_ptr(), idx.data_ptr(), Kt.data_ptr()
            d.znear, d.zfar, d.cull_back = _render.ZNEAR, _render.ZFAR, int(bool(cull_back))
            need = lambda n: _lib.workspace_bytes("mhmr_render_amodal_workspace_bytes", C.byref(d), NV, n)
            one = need(1)
            if int(max_workspace_bytes) < one:
                raise ValueError(f"max_workspace_bytes = {max_workspace_bytes} is below the {one} bytes of one person per pass")
            n = max(1, min(P, (int(max_workspace_bytes) - 256) // (one - 256)))
            ws = _render._workspace(need(n), dev)
            d.workspace, d.workspace_bytes = ws.data_ptr(), need(n)
            _lib.check(lib.mhmr_render_amodal(C.byref(d), NV, _lib.ptr(Rtt), amodal_px.data_ptr(), stream), "mhmr_render_amodal")

    occlusion = None
    if amodal:
        a = amodal_px.to(torch.float32)
        occlusion = torch.where(amodal_px > 0, 1.0 - visible.to(torch.float32) / a.clamp_min(1.0), torch.zeros_like(a))
    sq = (lambda t: t) if multi else (lambda t: None if t is None else t.squeeze(1))
    return RenderMaps(sq(person), sq(face), sq(depth), sq(label), sq(visible), sq(amodal_px), sq(occlusion), sq(bbox), sq(zmin),
                      sq(label_px), sq(vis), keys)
