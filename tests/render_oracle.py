"""CPU restatement of the mesh-overlay render contract (multi_hmr_amd/render.py, include/mhmr.h mhmr_render_desc), in numpy.

Geometry (camera transform, projection, edge functions, depth) is fp64 with every operation in the order csrc/render.hip
evaluates it, so the winning keys are expected to agree exactly; shading is fp64 here and fp32 on the device (1 LSB of rgb);
the mask and the blend are fp32, one rounding per operation, as the device computes them (bit-exact)."""
from __future__ import annotations

import numpy as np

KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
ZNEAR, ZFAR = float(np.float32(0.05)), 100.0                       # the clip planes are the descriptor's fp32 fields


def camera_vertices(x, R=None, t=None):
    """X = R x + t in fp64, summed as ((R0 x0 + R1 x1) + R2 x2) + t."""
    x = np.asarray(x, np.float32).astype(np.float64)
    R = np.eye(3) if R is None else np.asarray(R, np.float32).astype(np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, np.float32).astype(np.float64)
    return np.stack([((R[i, 0] * x[:, 0] + R[i, 1] * x[:, 1]) + R[i, 2] * x[:, 2]) + t[i] for i in range(3)], axis=1)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _norm(a):
    return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])


def _unit(a):
    n = _norm(a)[..., None]
    return np.where(n > 0, a / np.where(n > 0, n, 1.0), a)


def vertex_normals(x, faces):
    """Angle-weighted vertex normals (trimesh's vertex_normals form) of model-space vertices x [V, 3] (fp32 values, fp64
    arithmetic): sum over the incident non-degenerate faces, in face order, of corner angle x unit face normal, normalised;
    zero rows where the sum is zero."""
    x = np.asarray(x, np.float32).astype(np.float64)
    faces = np.asarray(faces, np.int64)
    P = x[faces]                                                   # [F, 3 corners, 3]
    fn = _cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    ln = _norm(fn)
    ok = ln > 0
    fu = fn / np.where(ok, ln, 1.0)[:, None]
    n = np.zeros_like(x)
    contrib, verts = [], []
    for c in range(3):
        u, w = P[:, (c + 1) % 3] - P[:, c], P[:, (c + 2) % 3] - P[:, c]
        cs = ((u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]) / np.where(ok, _norm(u) * _norm(w), 1.0)
        contrib.append(np.arccos(np.clip(cs, -1.0, 1.0))[:, None] * fu)
        verts.append(faces[:, c])
    fidx = np.concatenate([np.arange(len(faces))] * 3)
    contrib, verts, okk = np.concatenate(contrib), np.concatenate(verts), np.concatenate([ok] * 3)
    order = np.lexsort((fidx, verts))                             # per vertex, ascending face (the device's CSR order)
    order = order[okk[order]]
    np.add.at(n, verts[order], contrib[order])
    return _unit(n)


def _rotate(R, n):
    R = np.eye(3) if R is None else np.asarray(R, np.float32).astype(np.float64)
    return np.stack([(R[i, 0] * n[:, 0] + R[i, 1] * n[:, 1]) + R[i, 2] * n[:, 2] for i in range(3)], axis=1)


def _edge(ax, ay, bx, by, x, y):
    """Edge function of a -> b at (x, y) with the endpoints in lexicographic order, negated if swapped (exactly antisymmetric)."""
    keep = (ax < bx) | ((ax == bx) & (ay <= by))
    v1 = (bx - ax) * (y - ay) - (by - ay) * (x - ax)
    v2 = -((ax - bx) * (y - by) - (ay - by) * (x - bx))
    return np.where(keep, v1, v2)


def setup(X, faces, K, H, W, znear=ZNEAR, cull=True):
    """Face setup of camera-space vertices X [V, 3]: returns the indices of the faces that can draw and their screen data."""
    fx, fy, cx, cy = (float(np.float32(K[0][0])), float(np.float32(K[1][1])), float(np.float32(K[0][2])), float(np.float32(K[1][2])))
    faces = np.asarray(faces, np.int64)
    P = X[faces]                                                   # [F, 3, 3]
    keep = np.all(P[:, :, 2] >= znear, axis=1)
    if cull:
        e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        n = _cross(e1, e2)
        keep &= ((n[:, 0] * P[:, 0, 0] + n[:, 1] * P[:, 0, 1]) + n[:, 2] * P[:, 0, 2]) < 0
    with np.errstate(divide="ignore", invalid="ignore"):
        sx = (fx * P[:, :, 0]) / P[:, :, 2] + cx
        sy = (fy * P[:, :, 1]) / P[:, :, 2] + cy
    A = (sx[:, 1] - sx[:, 0]) * (sy[:, 2] - sy[:, 0]) - (sy[:, 1] - sy[:, 0]) * (sx[:, 2] - sx[:, 0])
    keep &= A != 0
    c0 = np.maximum(np.ceil(sx.min(1) - 0.5), 0)
    c1 = np.minimum(np.floor(sx.max(1) - 0.5), W - 1)
    r0 = np.maximum(np.ceil(sy.min(1) - 0.5), 0)
    r1 = np.minimum(np.floor(sy.max(1) - 0.5), H - 1)
    keep &= (c0 <= c1) & (r0 <= r1)
    idx = np.nonzero(keep)[0]
    sig = np.where(A[idx] > 0, 1.0, -1.0)
    t = dict(idx=idx, sx=sx[idx], sy=sy[idx], Z=P[idx, :, 2], sigma=sig, area=np.abs(A[idx]),
             x0=c0[idx].astype(np.int64), x1=c1[idx].astype(np.int64), y0=r0[idx].astype(np.int64), y1=r1[idx].astype(np.int64))
    tl = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        dx, dy = sig * (t["sx"][:, k] - t["sx"][:, j]), sig * (t["sy"][:, k] - t["sy"][:, j])
        tl.append(((dy == 0) & (dx > 0)) | (dy < 0))
    t["tl"] = np.stack(tl, 1)
    return t


def edge_values(t, sel, px, py):
    """e [n, 3] of faces t[sel] at pixel centres (px, py)."""
    e = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        e.append(t["sigma"][sel] * _edge(t["sx"][sel, j], t["sy"][sel, j], t["sx"][sel, k], t["sy"][sel, k], px, py))
    return np.stack(e, 1)


def depth(t, sel, e):
    w = (e / t["area"][sel, None]) / t["Z"][sel]
    return 1.0 / ((w[:, 0] + w[:, 1]) + w[:, 2]), w


def raster(X, faces, K, H, W, id_base=0, keys=None, znear=ZNEAR, zfar=ZFAR, cull=True, chunk=1 << 22):
    """Min-key visibility of one mesh into keys [H, W] uint64 (created if None).  Returns keys."""
    if keys is None:
        keys = np.full((H, W), KEY_NONE, np.uint64)
    t = setup(X, faces, K, H, W, znear, cull)
    n = (t["x1"] - t["x0"] + 1) * (t["y1"] - t["y0"] + 1)
    flat = keys.reshape(-1)
    start = 0
    while start < len(n):                                          # chunks of about `chunk` fragments
        cs = np.cumsum(n[start:])
        stop = start + max(1, int(np.searchsorted(cs, chunk)))
        sel = np.arange(start, stop)
        cnt = n[sel]
        fi = np.repeat(sel, cnt)
        q = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        bw = t["x1"][fi] - t["x0"][fi] + 1
        x, y = t["x0"][fi] + q % bw, t["y0"][fi] + q // bw
        e = edge_values(t, fi, x + 0.5, y + 0.5)
        cov = np.all((e > 0) | ((e == 0) & t["tl"][fi]), axis=1)
        fi, x, y, e = fi[cov], x[cov], y[cov], e[cov]
        Z, _ = depth(t, fi, e)
        with np.errstate(over="ignore", invalid="ignore"):
            Z = Z.astype(np.float32)                               # the depth the key holds is the depth that is clipped
        ok = (Z >= znear) & (Z <= zfar)
        fi, x, y, Z = fi[ok], x[ok], y[ok], Z[ok]
        key = (Z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (t["idx"][fi] + id_base).astype(np.uint64)
        np.minimum.at(flat, y * W + x, key)
        start = stop
    return keys


def shade_colour(n, v, base, intensity=3.0, ambient=0.3, metallic=0.0, roughness=0.5):
    """glTF metallic-roughness shading (as pyrender's mesh.frag is recalled to implement it; not checked against pyrender) of unit
    normals n [N, 3] and unit view vectors v [N, 3] (towards the camera) for base colours base [N, 3], light direction l = (0, 0, -1)
    (towards the light): returns c before the gamma, [N, 3] fp64."""
    l = np.array([0.0, 0.0, -1.0])
    h = _unit(l + v)
    dot = lambda a, b: (a[:, 0] * b[..., 0] + a[:, 1] * b[..., 1]) + a[:, 2] * b[..., 2]
    nl = np.clip(dot(n, l[None]), 0.001, 1.0)[:, None]
    nv = np.clip(np.abs(dot(n, v)), 0.001, 1.0)[:, None]
    nh = np.clip(dot(n, h), 0.0, 1.0)[:, None]
    vh = np.clip(dot(v, h), 0.0, 1.0)[:, None]
    al = roughness * roughness
    a2 = al * al
    g1 = lambda x: 2 * x / (x + np.sqrt(a2 + (1 - a2) * x * x))
    G = g1(nl) * g1(nv)
    D = a2 / (np.pi * ((nh * a2 - nh) * nh + 1) ** 2)
    f0 = 0.04 * (1 - metallic) + base * metallic
    cdiff = base * (1 - 0.04) * (1 - metallic)
    F = f0 + (1 - f0) * (1 - vh) ** 5
    return nl * intensity * ((1 - F) * cdiff / np.pi + F * G * D / (4 * nl * nv)) + ambient * base


def to_rgb(c):
    return np.floor(255 * np.clip(c ** (1 / 2.2), 0, 1) + 0.5)


def shade_keys(keys, Xs, Ns, faces, K, colors, smooth=True, cull=True, znear=ZNEAR, shading=None):
    """rgb [H, W, 3] float (0 where nothing is drawn) of the winners in keys [H, W]: Xs / Ns = per-person camera-space vertices /
    rotated vertex normals (person p of the key's id p F + f)."""
    shading = shading or {}
    H, W = keys.shape
    F = len(faces)
    rgb = np.zeros((H, W, 3))
    ys, xs = np.nonzero(keys != KEY_NONE)
    if len(ys) == 0:
        return rgb
    ids = (keys[ys, xs] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    faces = np.asarray(faces, np.int64)
    for p in np.unique(ids // F):
        s = ids // F == p
        f = ids[s] % F
        X = Xs[p]
        t = setup(X, faces[f], K, H, W, znear, cull)
        assert len(t["idx"]) == len(f), "a winning face fails its own setup"
        sel = np.arange(len(f))
        e = edge_values(t, sel, xs[s] + 0.5, ys[s] + 0.5)
        Z, w = depth(t, sel, e)
        mu = w * Z[:, None]
        C = X[faces[f]]                                            # [n, 3, 3]
        Pt = (mu[:, 0:1] * C[:, 0] + mu[:, 1:2] * C[:, 1]) + mu[:, 2:3] * C[:, 2]
        fn = _unit(_cross(C[:, 1] - C[:, 0], C[:, 2] - C[:, 0]))
        if smooth:
            Nv = Ns[p][faces[f]].astype(np.float32).astype(np.float64)  # the device stores vertex normals as fp32
            none = np.all(Nv == 0, axis=2)
            Nv = np.where(none[..., None], fn[:, None], Nv)
            n = _unit((mu[:, 0:1] * Nv[:, 0] + mu[:, 1:2] * Nv[:, 1]) + mu[:, 2:3] * Nv[:, 2])
            n = np.where(np.all(n == 0, axis=1)[:, None], fn, n)
        else:
            n = fn
        v = _unit(-Pt)
        base = np.repeat(np.asarray(colors, np.float32)[p][None].astype(np.float64), len(f), 0)
        rgb[ys[s], xs[s]] = to_rgb(shade_colour(n, v, base, **shading))
    return rgb


def mask(covered):
    """m = fg ? max(0, fl32(fl32(k fl32(2/9)) - 1)) : 0, k = covered pixels of the 3x3 neighbourhood (outside = not covered)."""
    H, W = covered.shape
    c = np.pad(covered.astype(np.int32), 1)
    k = sum(c[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
    m = np.maximum(np.float32(0), k.astype(np.float32) * (np.float32(2) / np.float32(9)) - np.float32(1))
    return np.where(covered, m, np.float32(0)).astype(np.float32)


def blend(img, rgb, m, alpha):
    """out = trunc(m (a rgb + (1 - a) img) + (1 - m) img), fp32, one rounding per operation."""
    a = np.float32(alpha)
    img = np.asarray(img).astype(np.float32)
    rgb = np.asarray(rgb).astype(np.float32)
    m = m[..., None].astype(np.float32)
    out = m * (a * rgb + (np.float32(1) - a) * img) + (np.float32(1) - m) * img
    return np.trunc(out).astype(np.uint8)


def render(images, verts, image_index, K, faces, colors, alpha=0.8, Rt=None, smooth=True, cull=True, shading=None):
    """The whole contract: images [B, H, W, 3] uint8, verts [P, V, 3], image_index [P], K [B, 3, 3], Rt [B, 3, 4] or None.
    Returns (out uint8 [B, H, W, 3], keys uint64 [B, H, W], rgb float [B, H, W, 3])."""
    images = np.asarray(images)
    B, H, W, _ = images.shape
    verts = np.asarray(verts, np.float32)
    P, F = len(verts), len(faces)
    keys = np.full((B, H, W), KEY_NONE, np.uint64)
    Xs, Ns = [], []
    for p in range(P):
        b = int(image_index[p])
        R, t = (None, None) if Rt is None else (np.asarray(Rt[b])[:, :3], np.asarray(Rt[b])[:, 3])
        Xs.append(camera_vertices(verts[p], R, t))
        Ns.append(_rotate(R, vertex_normals(verts[p], faces)) if smooth else None)
        raster(Xs[p], faces, K[b], H, W, id_base=p * F, keys=keys[b], cull=cull)
    out = np.empty_like(images)
    rgb = np.zeros((B, H, W, 3))
    for b in range(B):
        rgb[b] = shade_keys(keys[b], Xs, Ns, faces, K[b], colors, smooth=smooth, cull=cull, shading=shading)
        out[b] = blend(images[b], rgb[b], mask(keys[b] != KEY_NONE), alpha)
    return out, keys, rgb


def icosphere(subdiv):
    """Unit icosphere (outward faces, counter-clockwise seen from outside): subdiv 5 -> 10242 vertices, 20480 faces."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                cache[k] = len(v)
                v.append(m / np.linalg.norm(m))
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, np.float32), np.array(f, np.int32)
