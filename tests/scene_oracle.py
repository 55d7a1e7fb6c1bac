"""CPU restatement of the scene-packing contract (include/mhmr.h mhmr_scene_desc, csrc/scene.hip), in numpy, on top of
tests/render_oracle.py: positions ``camera_vertices`` rounded once to fp32, normals the render contract's angle-weighted vertex
normals rotated and rounded once to fp32 ((0, 0, 1) where a vertex has none), bounds the min / max of the fp32 positions."""
from __future__ import annotations

import numpy as np

import render_oracle as ro

DEFAULT_TRANSFORM = np.array([[-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 1, 0]], np.float32)


def normal_sums(x, faces):
    """The unnormalised sum of ``render_oracle.vertex_normals`` (same operations, same order: per vertex the incident non-degenerate
    faces in ascending face order) and the sum of the corner angles that weigh it: (n [V, 3], angles [V]).  |n| / angles says how
    much of the sum survives cancellation (1 on a flat neighbourhood)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    faces = np.asarray(faces, np.int64)
    P = x[faces]
    fn = ro._cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    ln = ro._norm(fn)
    ok = ln > 0
    fu = fn / np.where(ok, ln, 1.0)[:, None]
    n, angles = np.zeros_like(x), np.zeros(len(x))
    ang, verts = [], []
    for c in range(3):
        u, w = P[:, (c + 1) % 3] - P[:, c], P[:, (c + 2) % 3] - P[:, c]
        cs = ((u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]) / np.where(ok, ro._norm(u) * ro._norm(w), 1.0)
        ang.append(np.arccos(np.clip(cs, -1.0, 1.0)))
        verts.append(faces[:, c])
    fidx = np.concatenate([np.arange(len(faces))] * 3)
    ang, verts, okk, fu3 = np.concatenate(ang), np.concatenate(verts), np.concatenate([ok] * 3), np.concatenate([fu] * 3)
    order = np.lexsort((fidx, verts))
    order = order[okk[order]]
    np.add.at(n, verts[order], ang[order, None] * fu3[order])
    np.add.at(angles, verts[order], ang[order])
    return n, angles


def pack(verts, faces, transform=None):
    """verts [P, V, 3] -> (packed float32 [P, 2, V, 3], bounds float32 [P, 2, 3], none bool [P, V]: the vertices without a normal,
    survive float64 [P, V]: |weighted sum| / sum of angles, inf where there is no normal)."""
    M = np.asarray(DEFAULT_TRANSFORM if transform is None else transform, np.float32).reshape(3, 4)
    R, t = M[:, :3], M[:, 3]
    verts = np.asarray(verts, np.float32)
    P, V = verts.shape[:2]
    packed = np.zeros((P, 2, V, 3), np.float32)
    bounds = np.zeros((P, 2, 3), np.float32)
    none = np.zeros((P, V), bool)
    survive = np.full((P, V), np.inf)
    for p in range(P):
        packed[p, 0] = ro.camera_vertices(verts[p], R, t).astype(np.float32)
        n = ro.vertex_normals(verts[p], faces)
        none[p] = np.all(n == 0, axis=1)
        packed[p, 1] = np.where(none[p][:, None], np.array([0.0, 0.0, 1.0]), ro._rotate(R, n)).astype(np.float32)
        bounds[p, 0], bounds[p, 1] = packed[p, 0].min(0), packed[p, 0].max(0)
        s, a = normal_sums(verts[p], faces)
        assert np.array_equal(ro._unit(s), n)                              # the restated sum is vertex_normals' own
        survive[p, ~none[p]] = ro._norm(s)[~none[p]] / a[~none[p]]
    return packed, bounds, none, survive
