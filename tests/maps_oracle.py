"""CPU restatement, in numpy, of the three contracts of multi_hmr_amd/maps.py (include/mhmr.h mhmr_render_maps_desc,
mhmr_point_visibility_desc, mhmr_render_amodal) on top of tests/render_oracle.py's `raster` and `camera_vertices`: the keys are the
rasteriser oracle's, the maps and statistics are read off them as the header words it, the amodal area is the count of drawn keys of a
one-person raster, and a point's code is the header's fp64 rule, one rounding per operation.  Everything here is an integer, an fp32
copied out of a key or a comparison of fp64 values, so the device is expected to agree bit for bit."""
from __future__ import annotations

import numpy as np

import render_oracle as ro

KEY_NONE = ro.KEY_NONE
OCCLUDED, VISIBLE, OUTSIDE, INVALID = 0, 1, 2, 3


def views_of(Rt, B):
    """Rt None / [B, 3, 4] / [B, NV, 3, 4] -> ([B, NV, 3, 4] float32 or None, NV)."""
    if Rt is None:
        return None, 1
    Rt = np.asarray(Rt, np.float32).reshape(B, -1, 3, 4)
    return Rt, Rt.shape[1]


def _view(Rt, b, v):
    return (None, None) if Rt is None else (Rt[b, v, :, :3], Rt[b, v, :, 3])


def scene_keys(verts, image_index, K, faces, H, W, Rt=None, cull=True, only=None):
    """keys uint64 [B, NV, H, W] of the scene (render contract items 1-5); only = p: that person alone, keeping their id."""
    K = np.asarray(K, np.float32).reshape(-1, 3, 3)
    B, F = len(K), len(faces)
    Rt, NV = views_of(Rt, B)
    keys = np.full((B, NV, H, W), KEY_NONE, np.uint64)
    for p in range(len(verts)):
        b = int(image_index[p])
        if not 0 <= b < B or (only is not None and p != only):
            continue
        for v in range(NV):
            ro.raster(ro.camera_vertices(verts[p], *_view(Rt, b, v)), faces, K[b], H, W, id_base=p * F, keys=keys[b, v], cull=cull)
    return keys


def maps(keys, P, F, image_index, face_label=None):
    """The per-pixel maps and per-(person, view) statistics of keys [B, NV, H, W]."""
    keys = np.asarray(keys).view(np.uint64)
    B, NV, H, W = keys.shape
    idx = np.asarray(image_index, np.int64).reshape(-1)
    low = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    person, face = low // max(F, 1), low % max(F, 1)
    drawn = (keys != KEY_NONE) & (person < P)
    if P:
        drawn &= idx[np.minimum(person, P - 1)] == np.arange(B)[:, None, None, None]
    person = np.where(drawn, person, -1).astype(np.int32)
    face = np.where(drawn, face, -1).astype(np.int32)
    depth = np.where(drawn, (keys >> np.uint64(32)).astype(np.uint32), 0).astype(np.uint32).view(np.float32)
    out = dict(person=person, face=face, depth=depth)
    L = 0
    if face_label is not None:
        face_label = np.asarray(face_label, np.uint8)
        L = int(face_label.max()) + 1
        out["label"] = np.where(drawn, face_label[np.maximum(face, 0)], 255).astype(np.uint8)
        out["label_px"] = np.zeros((P, NV, L), np.int32)
    vis = np.zeros((P, NV), np.int32)
    bbox = np.tile(np.array([W, H, -1, -1], np.int32), (P, NV, 1))
    zmin = np.full((P, NV), np.inf, np.float32)
    for p in range(P):
        b = int(idx[p])
        if not 0 <= b < B:
            continue
        for v in range(NV):
            ys, xs = np.nonzero(person[b, v] == p)
            vis[p, v] = len(ys)
            if len(ys):
                bbox[p, v] = [xs.min(), ys.min(), xs.max(), ys.max()]
                zmin[p, v] = depth[b, v, ys, xs].min()
                if L:
                    out["label_px"][p, v] = np.bincount(out["label"][b, v, ys, xs], minlength=L)[:L]
    out.update(visible_px=vis, bbox=bbox, zmin=zmin)
    return out


def amodal(verts, image_index, K, faces, H, W, Rt=None, cull=True):
    """amodal_px int32 [P, NV]: the drawn keys of the raster that holds only person p."""
    K = np.asarray(K, np.float32).reshape(-1, 3, 3)
    _, NV = views_of(Rt, len(K))
    out = np.zeros((len(verts), NV), np.int32)
    for p in range(len(verts)):
        out[p] = (scene_keys(verts, image_index, K, faces, H, W, Rt, cull, only=p) != KEY_NONE).sum(axis=(0, 2, 3))
    return out


def occlusion(visible, amodal_px):
    a = amodal_px.astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(amodal_px > 0, np.float32(1) - visible.astype(np.float32) / np.maximum(a, np.float32(1)), np.float32(0)).astype(np.float32)


def point_visibility(points, image_index, K, keys, Rt=None, tau=0.03, znear=ro.ZNEAR):
    """codes uint8 [P, NV, N] of points [P, N, 3] against keys [B, NV, H, W]: the rule of mhmr_point_visibility_desc in fp64."""
    keys = np.asarray(keys).view(np.uint64)
    B, NV, H, W = keys.shape
    K = np.asarray(K, np.float32).reshape(B, 3, 3)
    Rt, _ = views_of(Rt, B)
    points = np.asarray(points, np.float32)
    P, N = points.shape[:2]
    tau = float(np.float32(tau))
    out = np.full((P, NV, N), OUTSIDE, np.uint8)
    depth = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(np.float64)
    for p in range(P):
        b = int(image_index[p])
        if not 0 <= b < B:
            continue
        fx, fy, cx, cy = (float(K[b, 0, 0]), float(K[b, 1, 1]), float(K[b, 0, 2]), float(K[b, 1, 2]))
        for v in range(NV):
            with np.errstate(all="ignore"):
                X = ro.camera_vertices(points[p], *_view(Rt, b, v))
                ok = np.isfinite(points[p]).all(1) & np.isfinite(X).all(1)
                ok &= X[:, 2] >= znear
                Z = np.where(ok, X[:, 2], 1.0)
                c = np.floor((fx * np.where(ok, X[:, 0], 0.0)) / Z + cx)
                r = np.floor((fy * np.where(ok, X[:, 1], 0.0)) / Z + cy)
            inside = ok & (c >= 0) & (c <= W - 1) & (r >= 0) & (r <= H - 1)
            ci, ri = np.where(inside, c, 0).astype(np.int64), np.where(inside, r, 0).astype(np.int64)
            none = keys[b, v, ri, ci] == KEY_NONE
            seen = none | (Z <= depth[b, v, ri, ci] + tau)
            out[p, v] = np.where(~ok, INVALID, np.where(~inside, OUTSIDE, np.where(seen, VISIBLE, OCCLUDED)))
    return out
