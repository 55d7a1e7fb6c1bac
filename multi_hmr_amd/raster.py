"""Differentiable rasteriser: per-pixel depth, perspective-correct barycentrics and interpolated vertex attributes of the visible
surface, attached to autograd with respect to the vertices and the attributes (``csrc/raster_grad.hip``, include/mhmr.h
``mhmr_raster_desc``: the contract; ``mhmr_raster_interpolate``, ``mhmr_raster_backward``).  There is no CPU path.

The rasteriser (``render.py``) decides who owns which pixel; that decision (the 64-bit keys) is held fixed and the values inside
each owned pixel are differentiated: nothing flows through coverage (silhouette edges), K or Rt.  ``depth`` is the key's own depth
bit for bit, so a per-pixel depth term compares the visible surface with a sensor's or a depth network's map:

    d = model.decode_readout(readout, offset, idx, K)
    ras = rasterize(d["v3d"], idx[0], K, faces, (S, S))
    (prior + depth_loss(ras, depth_map)).backward()

``attributes=template_vertices`` ([V, 3], shared by all persons) gives a dense-correspondence map: each pixel holds the template
position of the surface point it shows.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from . import maps as _maps
from . import render as _render

WANT = ("depth", "bary", "attributes")


class Raster(NamedTuple):
    """The result of ``rasterize``.  [B, H, W, ...] with a 3-D ``Rt`` (or None), [B, NV, H, W, ...] with a 4-D one.  Outputs that were
    not asked for are None.  Background (and stale, see include/mhmr.h) pixels hold 0, -1 and False."""
    depth: Optional[torch.Tensor]        # float32 [...], autograd
    bary: Optional[torch.Tensor]         # float32 [..., 3], autograd
    attributes: Optional[torch.Tensor]   # float32 [..., C], autograd
    person: torch.Tensor                 # int32, -1 = background
    face: torch.Tensor                   # int32, -1 = background
    mask: torch.Tensor                   # bool: the pixel shows a surface
    keys: torch.Tensor                   # int64 holding the uint64 keys


class _Scene(NamedTuple):
    """What one call fixes: shapes, device tensors that are not differentiated, options."""
    B: int
    NV: int
    H: int
    W: int
    P: int
    V: int
    F: int
    idx: torch.Tensor
    K: torch.Tensor
    Rt: Optional[torch.Tensor]
    faces: Optional[tuple]
    keys: torch.Tensor
    cull_back: bool
    max_workspace_bytes: int


def _desc(sc: _Scene, verts, attr):
    d = _lib.RasterDesc()
    d.B, d.NV, d.H, d.W, d.P, d.V, d.F = sc.B, sc.NV, sc.H, sc.W, sc.P, sc.V, sc.F
    d.verts, d.vstride = (verts.data_ptr() if sc.P else None), (int(verts.stride(0)) if sc.P > 1 else 3 * sc.V)
    if sc.faces is not None:
        d.faces, d.adj_off, d.adj = (t.data_ptr() for t in sc.faces)
    d.image_index, d.K, d.view_Rt, d.keys = (sc.idx.data_ptr() if sc.P else None), sc.K.data_ptr(), _lib.ptr(sc.Rt), sc.keys.data_ptr()
    d.znear, d.cull_back = _render.ZNEAR, int(sc.cull_back)
    if attr is not None:
        d.C = int(attr.shape[-1])
        d.attr, d.astride = (attr.data_ptr() if sc.P else sc.K.data_ptr()), (0 if attr.dim() == 2 else sc.V * d.C)   # nobody: never read
    return d


def pass_bytes(size, F, nviews=1, channels=0) -> int:
    """The workspace the backward needs to take ONE person per pass: the smallest ``max_workspace_bytes`` ``rasterize`` accepts."""
    d = _lib.RasterDesc()
    d.B, d.NV, d.H, d.W, d.P, d.V, d.F, d.C, d.vstride = 1, int(nviews), int(size[0]), int(size[1]), 1, 3, int(F), int(channels), 9
    return _lib.workspace_bytes("mhmr_raster_workspace_bytes", C.byref(d), 1)


def _interpolate(sc: _Scene, verts, attr, want_depth, want_bary, want_attr):
    dev = sc.keys.device
    img = (sc.B, sc.NV, sc.H, sc.W)
    new = lambda *tail: torch.empty(img + tail, dtype=torch.float32, device=dev)
    depth = new() if want_depth else None
    bary = new(3) if want_bary else None
    out = new(int(attr.shape[-1])) if want_attr else None
    d = _desc(sc, verts, attr if want_attr else None)
    d.depth, d.bary, d.out_attr = _lib.ptr(depth), _lib.ptr(bary), _lib.ptr(out)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mhmr_raster_interpolate(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "mhmr_raster_interpolate")
    return depth, bary, out


class _Rasterize(torch.autograd.Function):
    """depth, bary, attributes = f(verts, attributes) with the keys fixed; backward recomputes the geometry from the saved verts and keys.
    ``attr`` carries the graph ([P, V, C]; a shared table arrives expanded, so autograd sums its gradient over the persons) and
    ``table`` the values the kernels read ([P, V, C], or the shared [V, C] itself, passed with astride = 0)."""

    @staticmethod
    def forward(ctx, verts, attr, table, sc, want_bary, want_attr):
        v = _maps._strided(verts, sc.keys.device, "verts")
        depth, bary, out = _interpolate(sc, v, table, True, want_bary, want_attr)
        ctx.sc, ctx.wants = sc, (want_bary, want_attr)
        ctx.save_for_backward(v, table)
        ctx.set_materialize_grads(False)
        outs = [t if t is not None else torch.empty(0, device=sc.keys.device) for t in (depth, bary, out)]
        ctx.mark_non_differentiable(*[o for o, t in zip(outs, (depth, bary, out)) if t is None])
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_depth, g_bary, g_out):
        sc = ctx.sc
        v, a = ctx.saved_tensors
        dev = sc.keys.device
        want_bary, want_attr = ctx.wants
        cot = lambda g, w: g.to(torch.float32).contiguous() if (w and g is not None) else None
        g_depth, g_bary, g_out = cot(g_depth, True), cot(g_bary, want_bary), cot(g_out, want_attr)
        need_v, need_a = ctx.needs_input_grad[0], bool(ctx.needs_input_grad[1] and want_attr)
        use_attr = want_attr and (g_out is not None or need_a)
        g_verts = torch.empty((sc.P, sc.V, 3), dtype=torch.float32, device=dev)
        g_attr = torch.empty((sc.P, sc.V, int(a.shape[-1])), dtype=torch.float32, device=dev) if need_a else None
        if sc.P:
            d = _desc(sc, v, a if use_attr else None)
            d.g_depth, d.g_bary, d.g_out_attr = _lib.ptr(g_depth), _lib.ptr(g_bary), (_lib.ptr(g_out) if use_attr else None)
            d.g_verts, d.g_attr = g_verts.data_ptr(), _lib.ptr(g_attr)
            need = lambda n: _lib.workspace_bytes("mhmr_raster_workspace_bytes", C.byref(d), n)
            one = need(1)
            n = max(1, min(sc.P, (int(sc.max_workspace_bytes) - 256) // (one - 256)))
            with torch.cuda.device(dev):
                ws = _render._workspace(need(n), dev)
                d.workspace, d.workspace_bytes = ws.data_ptr(), need(n)
                _lib.check(_lib.lib().mhmr_raster_backward(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "mhmr_raster_backward")
        return (g_verts if need_v else None), g_attr, None, None, None, None


def rasterize(verts, image_index, K, faces, size, Rt=None, attributes=None, keys=None, cull_back=True, want=WANT,
              max_workspace_bytes=256 << 20) -> Raster:
    """Depth, barycentrics and interpolated attributes of the visible surface of P meshes sharing one face array, in B images of
    ``size`` = (H, W); the scene is given as to ``maps.render_maps``: verts [P, V, 3] cuda float32 (a strided ``v3d`` block is read in
    place), image_index [P], K [B, 3, 3], faces [F, 3], Rt None / [B, 3, 4] (outputs [B, H, W, ...]) or [B, NV, 3, 4] ([B, NV, H, W, ...]).

    attributes: [P, V, C] or [V, C] (one table for every person), C <= 16.  keys: those of an earlier render of the scene; None: the
    scene is rendered once here.  Given keys are used as they are: a pixel whose key does not fit these vertices (its face is dropped or
    does not cover the pixel's centre) is background.  want: which of "depth", "bary", "attributes" to compute ("attributes" needs
    ``attributes``).  The outputs are differentiable with respect to ``verts`` and ``attributes`` with the keys held fixed; the backward
    keeps its workspace within ``max_workspace_bytes`` whatever P is (persons are taken in passes; ``pass_bytes`` is the floor)."""
    if not (torch.is_tensor(verts) and verts.is_cuda and verts.dim() == 3 and verts.shape[-1] == 3):
        raise ValueError("verts must be a cuda tensor [P, V, 3]")
    want = tuple(want)
    if any(w not in WANT for w in want):
        raise ValueError(f"want must be a subset of {WANT}, got {want}")
    dev = verts.device
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
    if attributes is not None:
        if not (torch.is_tensor(attributes) and tuple(attributes.shape[:-1]) in ((P, V), (V,)) and 1 <= attributes.shape[-1] <= _lib.RASTER_MAX_CHANNELS):
            raise ValueError(f"attributes must be a tensor [{P}, {V}, C] or [{V}, C] with 1 <= C <= {_lib.RASTER_MAX_CHANNELS}")
    want_attr = "attributes" in want and attributes is not None
    if "attributes" in want and attributes is None and want != WANT:
        raise ValueError('want names "attributes" but no attributes were given')

    m = _maps.render_maps(verts, idx, Kt, f_host, (H, W), Rt=(Rtt if multi else (None if Rtt is None else Rtt[:, 0])), keys=keys,
                          amodal=False, cull_back=cull_back)
    keys4 = m.keys.reshape(B, NV, H, W)
    sc = _Scene(B, NV, H, W, P, V, F, idx, Kt, Rtt, _render._faces_on(f_host, V, dev) if P else None, keys4, bool(cull_back),
                int(max_workspace_bytes))
    one = pass_bytes((H, W), F, NV, int(attributes.shape[-1]) if want_attr else 0)
    if int(max_workspace_bytes) < one:
        raise ValueError(f"max_workspace_bytes = {max_workspace_bytes} is below the {one} bytes of one person per pass")

    table = graph = None
    if want_attr:
        table = attributes.detach().to(device=dev, dtype=torch.float32).contiguous()
        graph = attributes if attributes.dim() == 3 else attributes.expand(P, V, attributes.shape[-1])
    depth, bary, out = _Rasterize.apply(verts, graph, table, sc, "bary" in want, want_attr)
    sq = (lambda t: t) if multi else (lambda t: t.squeeze(1))
    mask = depth.detach() > 0                                           # Z >= znear > 0 wherever a surface is shown
    person = torch.where(mask, m.person.reshape(B, NV, H, W), torch.full_like(keys4, -1, dtype=torch.int32))
    face = torch.where(mask, m.face.reshape(B, NV, H, W), torch.full_like(keys4, -1, dtype=torch.int32))
    return Raster(sq(depth) if "depth" in want else None, sq(bary) if "bary" in want else None, sq(out) if want_attr else None,
                  sq(person), sq(face), sq(mask), m.keys)


def depth_loss(r: Raster, target, valid=None, sigma: float = 0.1, robust: str = "gmof") -> torch.Tensor:
    """sum over ``r.mask & valid`` of rho((r.depth - target)^2 / sigma^2), rho(s) = s / (1 + s) ("gmof", Geman-McClure, as
    ``KeypointFitter``) or s ("l2").  Plain torch on ``r.depth``: the gradient reaches the vertices through ``rasterize``.  ``target``
    has r.depth's shape (metres along the optical axis; where it is not finite the pixel is left out); ``sigma`` is a convention in
    metres, not a measurement."""
    if robust not in _lib.FIT_ROBUST:
        raise ValueError(f"robust must be one of {sorted(_lib.FIT_ROBUST)}, not {robust!r}")
    if r.depth is None:
        raise ValueError('depth_loss needs rasterize(..., want=) to include "depth"')
    target = torch.as_tensor(target, dtype=r.depth.dtype, device=r.depth.device)
    if target.shape != r.depth.shape:
        raise ValueError(f"target must have the depth map's shape {tuple(r.depth.shape)}, got {tuple(target.shape)}")
    keep = r.mask & torch.isfinite(target)
    if valid is not None:
        keep = keep & torch.as_tensor(valid, device=r.depth.device).bool()
    diff = torch.where(keep, r.depth - torch.where(keep, target, torch.zeros_like(target)), torch.zeros_like(r.depth))
    s = diff * diff / float(sigma) ** 2
    return (s / (1.0 + s) if robust == "gmof" else s).sum()
