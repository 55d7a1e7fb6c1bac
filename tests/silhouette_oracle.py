"""CPU restatement, in numpy and torch fp64, of the two contracts of multi_hmr_amd/silhouette.py (include/mhmr.h
mhmr_distance_transform_desc, mhmr_silhouette_desc).  The distance maps are brute force over all pairs in integers with the header's
tie rule; the projection is tests/render_oracle.py's ``camera_vertices`` and the point-visibility operation order, so ``floor`` gives
the device's pixels; the cover is tests/maps_oracle.py's one-person raster; the two terms are summed pixel by pixel and vertex by
vertex in fp64; the gradient exists twice, in closed form and as torch fp64 autograd with the assignments fixed.  No scipy."""
from __future__ import annotations

import numpy as np
import torch

import maps_oracle as mo
import render_oracle as ro

DIST_NONE = 0x7FFFFFFF
L2, GMOF = 0, 1


# ------------------------------------------------------------------------------------------------------------------ distance maps
def _cap(d2, near, R):
    if R > 0:
        far = d2 > R * R
        return np.where(far, R * R + 1, d2).astype(np.int32), np.where(far, -1, near).astype(np.int32)
    return d2.astype(np.int32), near.astype(np.int32)


def maps_of_every_kind(h, w, seed=0):
    """Eleven [h, w] bool maps: empty, full, one pixel in each corner, a checkerboard, point-symmetric pairs (dense ties), three random
    densities."""
    g = np.random.default_rng(seed)
    out = {"empty": np.zeros((h, w), bool), "full": np.ones((h, w), bool)}
    for name, (y, x) in dict(tl=(0, 0), tr=(0, w - 1), bl=(h - 1, 0), br=(h - 1, w - 1)).items():
        out[name] = np.zeros((h, w), bool)
        out[name][y, x] = True
    out["checker"] = (np.add.outer(np.arange(h), np.arange(w)) % 2) == 0
    pair = np.zeros((h, w), bool)
    pair[0, 0] = pair[h - 1, w - 1] = pair[h // 2, w // 3] = pair[h - 1 - h // 2, w - 1 - w // 3] = True        # point-symmetric pairs
    out["pairs"] = pair
    for dens in (0.001, 0.05, 0.5):
        out[f"random{dens}"] = g.random((h, w)) < dens
    return out


def transform_brute(src, R=0):
    """(dist2, nearest) int32 [H, W] of one map: every pixel against every on-pixel, the smallest linear index among the minimisers."""
    src = np.asarray(src) != 0
    H, W = src.shape
    ys, xs = np.nonzero(src)                                           # ascending linear index
    if len(ys) == 0:
        return np.full((H, W), R * R + 1 if R > 0 else DIST_NONE, np.int32), np.full((H, W), -1, np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = (xx.reshape(-1, 1).astype(np.int64) - xs[None]) ** 2 + (yy.reshape(-1, 1).astype(np.int64) - ys[None]) ** 2
    first = d2.argmin(1)                                               # the first minimum: the smallest linear index
    return _cap(d2[np.arange(H * W), first].reshape(H, W), (ys[first] * W + xs[first]).reshape(H, W), R)


def transform_separable(src, R=0):
    """The same maps by the two passes the kernel takes: per column each pixel's nearest on-row (the smaller row on a tie), then per row
    the lexicographic minimum of (d2, y', x') over the columns."""
    src = np.asarray(src) != 0
    H, W = src.shape
    col = np.full((H, W), -1, np.int64)
    for x in range(W):
        rows = np.nonzero(src[:, x])[0]
        if len(rows):
            d = np.abs(np.arange(H)[:, None] - rows[None])
            col[:, x] = rows[d.argmin(1)]                              # rows ascend: the first minimum is the smaller row
    if not src.any():
        return transform_brute(src, R)
    big = np.int64(1) << 40
    dy2 = np.where(col >= 0, (col - np.arange(H)[:, None]) ** 2, big)                       # [H, W'] per (row, column)
    d2 = dy2[:, None, :] + (np.arange(W)[None, :, None] - np.arange(W)[None, None, :]) ** 2  # [H, W, W']
    key = (d2 * (H * W)) + np.where(col >= 0, col * W + np.arange(W)[None], 0)[:, None, :]   # (d2, y' W + x') in one integer
    best = key.argmin(2)
    y = np.arange(H)[:, None]
    return _cap(np.take_along_axis(d2, best[..., None], 2)[..., 0], col[y, best] * W + best, R)


# ----------------------------------------------------------------------------------------------------------------------- the scene
def _cam(K, b):
    K = np.asarray(K, np.float32).reshape(-1, 3, 3)
    return float(K[b, 0, 0]), float(K[b, 1, 1]), float(K[b, 0, 2]), float(K[b, 1, 2])


def _rt(Rt, b):
    return (None, None) if Rt is None else (np.asarray(Rt, np.float32)[b, :, :3], np.asarray(Rt, np.float32)[b, :, 3])


def project(x, K, b, Rt, H, W, znear=ro.ZNEAR):
    """The point-visibility rule for vertices x [V, 3] of a person of image b: ok (projectable and inside), u, v, r, c."""
    x = np.asarray(x, np.float32)
    fx, fy, cx, cy = _cam(K, b)
    with np.errstate(all="ignore"):
        X = ro.camera_vertices(x, *_rt(Rt, b))
        ok = np.isfinite(x).all(1) & np.isfinite(X).all(1)
        ok &= X[:, 2] >= znear
        Z = np.where(ok, X[:, 2], 1.0)
        u = (fx * np.where(ok, X[:, 0], 0.0)) / Z + cx
        v = (fy * np.where(ok, X[:, 1], 0.0)) / Z + cy
        c, r = np.floor(u), np.floor(v)
    ok &= (c >= 0) & (c <= W - 1) & (r >= 0) & (r <= H - 1)
    return ok, u, v, np.where(ok, r, 0).astype(np.int64), np.where(ok, c, 0).astype(np.int64)


def cover(verts, image_index, K, faces, H, W, Rt=None, cull=True):
    """[P, H, W] bool: the pixels mhmr_render_amodal counts for each person (the drawn keys of the raster that holds only that person)."""
    K = np.asarray(K, np.float32).reshape(-1, 3, 3)
    out = np.zeros((len(verts), H, W), bool)
    Rt4 = None if Rt is None else np.asarray(Rt, np.float32).reshape(len(K), 1, 3, 4)
    for p in range(len(verts)):
        b = int(image_index[p])
        if 0 <= b < len(K):
            out[p] = mo.scene_keys(verts, image_index, K, faces, H, W, Rt4, cull, only=p)[b, 0] != mo.KEY_NONE
    return out


def others_allowed(mask, image_index, B):
    """ignore="others": a person's own mask or another person's mask of the same image."""
    mask = np.asarray(mask) != 0
    out = mask.copy()
    for p in range(len(mask)):
        for q in range(len(mask)):
            if q != p and 0 <= image_index[p] < B and image_index[q] == image_index[p]:
                out[p] |= mask[q]
    return out


def forward(verts, image_index, K, faces, mask, allowed=None, sigma=8.0, robust=GMOF, R=64, Rt=None, cull=True):
    """Everything mhmr_silhouette decides and computes, per person: splat [P, H, W] int32, moments [P, V, 4] int64, counts [P, 2] int32,
    terms [P, 2] fp64 (term 1 summed pixel by pixel), the assignment ``assign`` (per person: pixel rows, columns, owners) and what the
    torch restatement holds fixed."""
    verts = np.asarray(verts, np.float32)
    mask = np.asarray(mask) != 0
    allowed = mask if allowed is None else (np.asarray(allowed) != 0)
    P, V = verts.shape[:2]
    H, W = mask.shape[1:]
    B = len(np.asarray(K).reshape(-1, 3, 3))
    sig2 = float(np.float32(sigma)) ** 2
    cov = cover(verts, image_index, K, faces, H, W, Rt, cull)
    out = dict(splat=np.full((P, H, W), -1, np.int32), moments=np.zeros((P, V, 4), np.int64), counts=np.zeros((P, 2), np.int32),
               terms=np.zeros((P, 2)), cover=cov, ok=np.zeros((P, V), bool), assign=[], cell=[], phi=np.zeros((P, V)), sig2=sig2,
               robust=robust, dist2=np.zeros((P, H, W), np.int32))
    for p in range(P):
        b = int(image_index[p])
        out["dist2"][p] = transform_brute(allowed[p], R)[0]
        empty = (np.zeros(0, np.int64),) * 3
        if not 0 <= b < B:
            out["assign"].append(empty)
            out["cell"].append(None)
            continue
        ok, u, v, r, c = project(verts[p], K, b, Rt, H, W)
        out["ok"][p] = ok
        # ---- term 0
        phi_map = np.sqrt(out["dist2"][p].astype(np.float64))
        ru, rv = u - 0.5, v - 0.5
        su, sv = np.clip(ru, 0.0, W - 1), np.clip(rv, 0.0, H - 1)
        x0, y0 = np.floor(np.where(ok, su, 0)).astype(np.int64), np.floor(np.where(ok, sv, 0)).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        free_u, free_v = (ru > 0) & (ru < W - 1), (rv > 0) & (rv < H - 1)
        out["cell"].append(dict(x0=x0, y0=y0, x1=x1, y1=y1, free_u=free_u, free_v=free_v, su=su, sv=sv,
                                f=[phi_map[y0, x0], phi_map[y0, x1], phi_map[y1, x0], phi_map[y1, x1]]))
        tx, ty = su - x0, sv - y0
        f00, f10, f01, f11 = out["cell"][p]["f"]
        phi = (1 - ty) * ((1 - tx) * f00 + tx * f10) + ty * ((1 - tx) * f01 + tx * f11)
        phi = np.where(ok, phi, 0.0)
        s = phi * phi / sig2
        out["phi"][p] = phi
        out["terms"][p, 0] = np.where(ok, s / (1 + s) if robust == GMOF else s, 0.0).sum()
        out["counts"][p, 0] = int((ok & (phi > 0)).sum())
        # ---- term 1
        for n in np.nonzero(ok)[0][::-1]:                              # descending: the smallest index is written last
            out["splat"][p, r[n], c[n]] = n
        _, near = transform_brute(out["splat"][p] >= 0, R)
        ys, xs = np.nonzero(mask[p] & ~cov[p] & (near >= 0))
        owner = out["splat"][p].reshape(-1)[near[ys, xs]].astype(np.int64)
        out["assign"].append((ys, xs, owner))
        ax, ay = 2 * xs + 1, 2 * ys + 1
        for k, val in enumerate((np.ones_like(ax), ax, ay, ax * ax + ay * ay)):
            np.add.at(out["moments"][p, :, k], owner, val)
        out["counts"][p, 1] = len(ys)
        out["terms"][p, 1] = (((u[owner] - (xs + 0.5)) ** 2 + (v[owner] - (ys + 0.5)) ** 2) / sig2).sum()
    return out


def term1_from_moments(verts, image_index, K, fwd, Rt=None):
    """[P] fp64: the uncovered term through the per-vertex moments, n |pi|^2 - pi . (Sx, Sy) + Sq / 4 (the unshifted form)."""
    P = len(verts)
    H, W = fwd["splat"].shape[1:]
    out = np.zeros(P)
    for p in range(P):
        if fwd["cell"][p] is None:
            continue
        ok, u, v, _, _ = project(verts[p], K, int(image_index[p]), Rt, H, W)
        n, Sx, Sy, Sq = (fwd["moments"][p, :, k].astype(np.float64) for k in range(4))
        val = (n * (u * u + v * v) - (u * Sx + v * Sy) + Sq / 4) / fwd["sig2"]
        out[p] = np.where(ok & (n > 0), val, 0.0).sum()
    return out


def terms_torch(verts, image_index, K, fwd, Rt=None):
    """terms [P, 2] as a torch fp64 function of verts [P, V, 3] with everything discrete (which vertices count, the bilinear cells and
    their clamping, the assignment) taken from ``fwd``."""
    P, V = verts.shape[:2]
    rows = []
    for p in range(P):
        cell = fwd["cell"][p]
        if cell is None:
            rows.append(torch.zeros(2, dtype=torch.float64) + 0 * verts[p].sum() * 0)
            continue
        b = int(image_index[p])
        fx, fy, cx, cy = _cam(K, b)
        R_, t_ = _rt(Rt, b)
        R_ = torch.eye(3, dtype=torch.float64) if R_ is None else torch.from_numpy(R_.astype(np.float64))
        t_ = torch.zeros(3, dtype=torch.float64) if t_ is None else torch.from_numpy(t_.astype(np.float64))
        ok = torch.from_numpy(fwd["ok"][p])
        x = torch.where(ok[:, None], verts[p], torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(V, 3))
        X = x @ R_.T + t_
        u, v = fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy
        tn = lambda a: torch.from_numpy(np.asarray(a))
        su = torch.where(tn(cell["free_u"]), u - 0.5, tn(cell["su"]))
        sv = torch.where(tn(cell["free_v"]), v - 0.5, tn(cell["sv"]))
        tx, ty = su - tn(cell["x0"]), sv - tn(cell["y0"])
        f00, f10, f01, f11 = (tn(f) for f in cell["f"])
        phi = (1 - ty) * ((1 - tx) * f00 + tx * f10) + ty * ((1 - tx) * f01 + tx * f11)
        s = phi * phi / fwd["sig2"]
        t0 = torch.where(ok, s / (1 + s) if fwd["robust"] == GMOF else s, torch.zeros_like(s)).sum()
        ys, xs, owner = fwd["assign"][p]
        o = tn(owner)
        t1 = (((u[o] - tn(xs + 0.5)) ** 2 + (v[o] - tn(ys + 0.5)) ** 2) / fwd["sig2"]).sum()
        rows.append(torch.stack([t0, t1]))
    return torch.stack(rows) if rows else torch.zeros((0, 2), dtype=torch.float64)


def backward_autograd(verts, image_index, K, fwd, Rt=None):
    """g [2, P, V, 3] fp64: the gradient of each term on its own, by autograd of ``terms_torch``."""
    v = torch.from_numpy(np.asarray(verts, np.float32).astype(np.float64)).requires_grad_(True)
    t = terms_torch(v, image_index, K, fwd, Rt)
    out = np.zeros((2,) + tuple(v.shape))
    if t.numel():
        for k in range(2):
            g, = torch.autograd.grad(t[:, k].sum(), v, retain_graph=True, allow_unused=True)
            out[k] = 0 if g is None else np.nan_to_num(g.numpy(), nan=0.0) * fwd["ok"][..., None]
    return out


def backward_closed(verts, image_index, K, fwd, Rt=None):
    """The same gradient by the header's formulas, numpy fp64."""
    verts = np.asarray(verts, np.float32)
    P, V = verts.shape[:2]
    H, W = fwd["splat"].shape[1:]
    out = np.zeros((2, P, V, 3))
    for p in range(P):
        cell = fwd["cell"][p]
        if cell is None:
            continue
        b = int(image_index[p])
        fx, fy, cx, cy = _cam(K, b)
        R_, _ = _rt(Rt, b)
        R_ = np.eye(3) if R_ is None else R_.astype(np.float64)
        ok = fwd["ok"][p]
        with np.errstate(all="ignore"):
            X = np.where(ok[:, None], ro.camera_vertices(verts[p], *_rt(Rt, b)), [0.0, 0.0, 1.0])
        u, v = fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy
        tx, ty = cell["su"] - cell["x0"], cell["sv"] - cell["y0"]
        f00, f10, f01, f11 = cell["f"]
        phi = fwd["phi"][p]
        dpu = np.where(cell["free_u"], (1 - ty) * (f10 - f00) + ty * (f11 - f01), 0.0)
        dpv = np.where(cell["free_v"], ((1 - tx) * f01 + tx * f11) - ((1 - tx) * f00 + tx * f10), 0.0)
        s = phi * phi / fwd["sig2"]
        gphi = (1 / (1 + s) ** 2 if fwd["robust"] == GMOF else 1.0) * 2 * phi / fwd["sig2"]
        n, Sx, Sy, _ = (fwd["moments"][p, :, k].astype(np.float64) for k in range(4))
        for k, (gu, gv) in enumerate(((gphi * dpu, gphi * dpv), ((2 * n * u - Sx) / fwd["sig2"], (2 * n * v - Sy) / fwd["sig2"]))):
            gX = np.stack([gu * fx / X[:, 2], gv * fy / X[:, 2], -(gu * fx * X[:, 0] + gv * fy * X[:, 1]) / X[:, 2] ** 2], 1)
            out[k, p] = np.where(ok[:, None], gX @ R_, 0.0)
    return out
