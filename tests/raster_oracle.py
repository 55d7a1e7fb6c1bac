"""CPU restatement of the differentiable key read-out (include/mhmr.h mhmr_raster_desc, csrc/raster_grad.hip, multi_hmr_amd/raster.py).

Three forms of one map, on top of tests/render_oracle.py's ``setup`` / ``edge_values`` / ``depth``:

* ``forward_np``: numpy fp64 in the device's operation order; depth, barycentrics and attributes are expected bit for bit.
* ``forward_torch``: the same edge-function route in torch fp64 on the owned pixels ``forward_np`` found, for autograd: the gradient's
  reference (``backward_autograd``).
* ``backward_closed``: the header's closed form per pixel (w = M^-1 d, M^T h = g_w, g_X_i = -w_i h), in numpy.

The contract, restated.  A pixel is background when its key is ~0, names a person >= P, or a person of another image.  Otherwise
(p, f) = low32 / F, % F; the pixel is stale (treated as background, no gradient) when a face index is outside [0, V), the face fails
the rasteriser's setup, the pixel lies outside the face's pixel box, or its centre is not covered.  Else w_i = (e_i / area) / Z_i,
Z = 1 / ((w0 + w1) + w2), b_i = w_i Z, attribute c = (b0 a0c + b1 a1c) + b2 a2c; each output is rounded to fp32 once."""
from __future__ import annotations

import numpy as np
import torch

import maps_oracle as mo
import render_oracle as ro

KEY_NONE = ro.KEY_NONE


def _attr_of(attr, p):
    return attr if attr.ndim == 2 else attr[p]


def forward_np(verts, image_index, K, faces, H, W, keys, Rt=None, attr=None, cull=True, znear=ro.ZNEAR):
    """keys uint64 [B, NV, H, W] -> dict of depth [B, NV, H, W], bary [.., 3], attr [.., C] (float32; fp64 copies under "depth64" ...),
    owned (bool: neither background nor stale), person / face (int64, the key's, -1 where not owned)."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64)
    keys = np.asarray(keys).view(np.uint64)
    K = np.asarray(K, np.float32).reshape(-1, 3, 3)
    B, NV = keys.shape[:2]
    P, V, F = len(verts), verts.shape[1], len(faces)
    idx = np.asarray(image_index, np.int64).reshape(-1)
    Rt, _ = mo.views_of(Rt, B)
    if attr is not None:
        attr = np.asarray(attr, np.float32).astype(np.float64)
    C = 0 if attr is None else attr.shape[-1]
    low = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    person, face = low // max(F, 1), low % max(F, 1)
    fg = (keys != KEY_NONE) & (person < P)
    if P:
        fg &= idx[np.minimum(person, P - 1)] == np.arange(B)[:, None, None, None]
    depth, bary, out = np.zeros(keys.shape), np.zeros(keys.shape + (3,)), np.zeros(keys.shape + (C,))
    owned = np.zeros(keys.shape, bool)
    for b in range(B):
        for v in range(NV):
            for p in np.unique(person[b, v][fg[b, v]]):
                ys, xs = np.nonzero(fg[b, v] & (person[b, v] == p))
                f = face[b, v, ys, xs]
                ok = ((faces[f] >= 0) & (faces[f] < V)).all(1)
                ys, xs, f = ys[ok], xs[ok], f[ok]
                with np.errstate(all="ignore"):
                    X = ro.camera_vertices(verts[p], *mo._view(Rt, b, v))
                    t = ro.setup(X, faces[f], K[b], H, W, znear, cull)
                sel = np.arange(len(t["idx"]))
                ys, xs, f = ys[t["idx"]], xs[t["idx"]], f[t["idx"]]
                box = (xs >= t["x0"]) & (xs <= t["x1"]) & (ys >= t["y0"]) & (ys <= t["y1"])
                e = ro.edge_values(t, sel, xs + 0.5, ys + 0.5)
                cov = box & np.all((e > 0) | ((e == 0) & t["tl"]), axis=1)
                ys, xs, f, sel, e = ys[cov], xs[cov], f[cov], sel[cov], e[cov]
                Z, w = ro.depth(t, sel, e)
                bc = w * Z[:, None]
                owned[b, v, ys, xs] = True
                depth[b, v, ys, xs], bary[b, v, ys, xs] = Z, bc
                if C:
                    a = _attr_of(attr, p)[faces[f]]                    # [n, 3, C]
                    out[b, v, ys, xs] = (bc[:, 0:1] * a[:, 0] + bc[:, 1:2] * a[:, 1]) + bc[:, 2:3] * a[:, 2]
    return dict(depth=depth.astype(np.float32), bary=bary.astype(np.float32), attr=out.astype(np.float32), depth64=depth, bary64=bary,
                attr64=out, owned=owned, person=np.where(owned, person, -1), face=np.where(owned, face, -1))


def _pixels(fwd, K, Rt):
    """The owned pixels as index arrays, and their camera (fx, fy, cx, cy) and rotation / translation, fp64."""
    b, v, r, c = np.nonzero(fwd["owned"])
    K = np.asarray(K, np.float32).reshape(-1, 3, 3).astype(np.float64)
    cam = np.stack([K[b, 0, 0], K[b, 1, 1], K[b, 0, 2], K[b, 1, 2]], 1)
    if Rt is None:
        R, T = np.tile(np.eye(3), (len(b), 1, 1)), np.zeros((len(b), 3))
    else:
        Rt = np.asarray(Rt, np.float32).reshape(K.shape[0], -1, 3, 4).astype(np.float64)
        R, T = Rt[b, v, :, :3], Rt[b, v, :, 3]
    return (b, v, r, c), fwd["person"][b, v, r, c], fwd["face"][b, v, r, c], cam, R, T


def forward_torch(verts, attr, fwd, K, faces, Rt=None):
    """The edge-function route in torch fp64 on the owned pixels of ``fwd`` (their (p, f) fixed): verts [P, V, 3] and attr ([P, V, C],
    [V, C] or None) are fp64 tensors, possibly requiring grad.  Returns depth, bary, attr in ``fwd``'s shapes (0 where not owned)."""
    F64 = torch.float64
    (b, v, r, c), p, f, cam, R, T = _pixels(fwd, K, Rt)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    faces_t = tt(np.asarray(faces, np.int64))
    pt, corners = tt(p), faces_t[tt(f)]                                 # [n], [n, 3]
    x = verts[pt[:, None], corners]                                     # [n, 3, 3]
    X = torch.einsum("nij,nkj->nki", tt(R), x) + tt(T)[:, None]
    cam = tt(cam)
    sx = cam[:, 0:1] * X[..., 0] / X[..., 2] + cam[:, 2:3]
    sy = cam[:, 1:2] * X[..., 1] / X[..., 2] + cam[:, 3:4]
    A = (sx[:, 1] - sx[:, 0]) * (sy[:, 2] - sy[:, 0]) - (sy[:, 1] - sy[:, 0]) * (sx[:, 2] - sx[:, 0])
    px, py = tt(c + 0.5), tt(r + 0.5)
    w = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        e = (sx[:, k] - sx[:, j]) * (py - sy[:, j]) - (sy[:, k] - sy[:, j]) * (px - sx[:, j])
        w.append((e / A) / X[:, i, 2])                                  # sigma e / |A| = e / A
    w = torch.stack(w, 1)
    Z = 1.0 / ((w[:, 0] + w[:, 1]) + w[:, 2])
    bc = w * Z[:, None]
    shape = fwd["owned"].shape
    where = (tt(b), tt(v), tt(r), tt(c))
    depth = torch.zeros(shape, dtype=F64).index_put(where, Z)
    bary = torch.zeros(shape + (3,), dtype=F64).index_put(where, bc)
    out = None
    if attr is not None:
        a = attr[corners] if attr.dim() == 2 else attr[pt[:, None], corners]            # [n, 3, C]
        out = torch.zeros(shape + (a.shape[-1],), dtype=F64).index_put(where, (bc[:, 0:1] * a[:, 0] + bc[:, 1:2] * a[:, 1]) + bc[:, 2:3] * a[:, 2])
    return depth, bary, out


def _masked(g, owned):
    """A cotangent as fp64 with zeros where the pixel is not owned (the contract does not read it there)."""
    g = np.asarray(g, np.float64)
    return np.where(owned.reshape(owned.shape + (1,) * (g.ndim - owned.ndim)), g, 0.0)


def backward_autograd(verts, attr, fwd, K, faces, Rt=None, g_depth=None, g_bary=None, g_attr=None):
    """fp64 autograd of ``forward_torch``: (g_verts [P, V, 3], g_attr in attr's shape or None), numpy."""
    vt = torch.from_numpy(np.asarray(verts, np.float32).astype(np.float64)).requires_grad_(True)
    at = None if attr is None else torch.from_numpy(np.asarray(attr, np.float32).astype(np.float64)).requires_grad_(True)
    depth, bary, out = forward_torch(vt, at, fwd, K, faces, Rt)
    loss = (vt * 0).sum()
    for y, g in ((depth, g_depth), (bary, g_bary), (out, g_attr)):
        if g is not None and y is not None:
            loss = loss + (y * torch.from_numpy(_masked(g, fwd["owned"]))).sum()
    loss.backward()
    return vt.grad.numpy(), None if at is None else (np.zeros(at.shape) if at.grad is None else at.grad.numpy())


def backward_closed(verts, attr, fwd, K, faces, Rt=None, g_depth=None, g_bary=None, g_attr=None):
    """The header's closed form, per owned pixel, summed with np.add.at: (g_verts, g_attr) fp64."""
    verts = np.asarray(verts, np.float32).astype(np.float64)
    faces = np.asarray(faces, np.int64)
    (b, v, r, c), p, f, cam, R, T = _pixels(fwd, K, Rt)
    n = len(p)
    corners = faces[f]
    X = np.einsum("nij,nkj->nki", R, verts[p[:, None], corners]) + T[:, None]
    M = np.transpose(X, (0, 2, 1))                                       # columns X0 X1 X2
    d = np.stack([(c + 0.5 - cam[:, 2]) / cam[:, 0], (r + 0.5 - cam[:, 3]) / cam[:, 1], np.ones(n)], 1)
    w = np.linalg.solve(M, d[..., None])[..., 0] if n else np.zeros((0, 3))
    Z = 1.0 / w.sum(1)
    bc = w * Z[:, None]
    owned = fwd["owned"]
    gh = np.zeros((n, 3))
    if g_bary is not None:
        gh += _masked(g_bary, owned)[b, v, r, c]
    go = None
    if attr is not None:
        attr = np.asarray(attr, np.float32).astype(np.float64)
        a = attr[corners] if attr.ndim == 2 else attr[p[:, None], corners]                # [n, 3, C]
        if g_attr is not None:
            go = _masked(g_attr, owned)[b, v, r, c]                                       # [n, C]
            gh += np.einsum("nc,nic->ni", go, a)
    gz = _masked(g_depth, owned)[b, v, r, c] if g_depth is not None else np.zeros(n)
    gw = Z[:, None] * (gh - (gh * bc).sum(1, keepdims=True)) - (gz * Z * Z)[:, None]
    h = np.linalg.solve(np.transpose(M, (0, 2, 1)), gw[..., None])[..., 0] if n else np.zeros((0, 3))
    gX = -w[:, :, None] * h[:, None, :]                                                   # [n, corner, 3]
    gx = np.einsum("nji,nkj->nki", R, gX)                                                 # R^T g_X
    g_verts = np.zeros_like(verts)
    np.add.at(g_verts, (p[:, None], corners), gx)
    ga = None
    if attr is not None:
        ga = np.zeros_like(attr)
        if go is not None:
            contrib = bc[:, :, None] * go[:, None, :]
            np.add.at(ga, corners if attr.ndim == 2 else (p[:, None], corners), contrib)
    return g_verts, ga
