"""Exact scenes for the mesh-overlay rasteriser: no pixel of them is decided by rounding (but for `rounded_seam_scene` at the end,
which rounds on purpose and claims only what holds under any rounding).

Every scene has fx = fy = 64, an integer principal point, and vertices x = (u - cx) Z / 64, y = (v - cy) Z / 64 whose screen position
(u, v) lies on a pixel centre or a quarter pixel.  With Z a power of two (1, 2 or 4; the clip-plane scene uses the fp32 neighbours of
znear and zfar with u - cx = +-8) every vertex is an fp32 number and projects back to (u, v) bit for bit, so every edge function is an
exact fp64 number: any correct implementation of the contract of include/mhmr.h gives the same coverage and the same winner on every
pixel, and a mismatch is a bug, not rounding.  `check_exact` asserts those two properties for every scene it is given.

`exact_cover` is the third party to the numpy oracle (tests/render_oracle.py) and the kernel (csrc/render.hip): coverage in integer
arithmetic on coordinates x 4, written from the header's wording and sharing no code with either.

To count how often a pixel centre is covered, a scene of n triangles is drawn one face per image (`one_face_per_image`): n persons of
three vertices, faces [[0, 1, 2]], person p into image p.  The per-pixel sum of `key != none` over the images is the count."""
from __future__ import annotations

import numpy as np

import render_oracle as ro

FOCAL = 64.0
ZS = (1.0, 2.0, 4.0)
SMALL_MAX = 128                     # csrc/render.hip: a larger pixel box goes to the workgroup pass
LARGE_GRID = 1024                   # csrc/render.hip: workgroups of that pass
ONE_FACE = np.array([[0, 1, 2]], np.int32)


def cam(cx, cy):
    assert cx == int(cx) and cy == int(cy)
    return np.array([[FOCAL, 0, cx], [0, FOCAL, cy], [0, 0, 1]], np.float32)


def vertex(u, v, Z, cx, cy):
    """The fp32 vertex at depth Z that projects to (u, v); asserts that it is exactly representable."""
    assert 4 * u == int(4 * u) and 4 * v == int(4 * v), (u, v)
    x = np.array([(u - cx) * Z / FOCAL, (v - cy) * Z / FOCAL, Z], np.float64)
    x32 = x.astype(np.float32)
    assert (x32.astype(np.float64) == x).all(), (u, v, Z)
    return x32


# ---------------------------------------------------------------------------------------------------------------------------------
# exact coverage, from the wording of include/mhmr.h
# ---------------------------------------------------------------------------------------------------------------------------------
def _quarter(c):
    q = 4 * float(c)
    assert q == int(q), c
    return int(q)


def _cover_convex(points, H, W):
    """Pixel centres inside a convex polygon (screen points on quarter pixels): for every edge the edge function is > 0, or == 0 on a
    top or left edge.  Integers throughout (coordinates x 4, the centre of pixel (r, c) at (4 c + 2, 4 r + 2)).  An edge is a left
    edge when one step to the right leads into the polygon, and a top edge when it is horizontal and one step down does."""
    P = [(_quarter(p[0]), _quarter(p[1])) for p in points]
    n = len(P)
    area2 = sum(P[i][0] * P[(i + 1) % n][1] - P[(i + 1) % n][0] * P[i][1] for i in range(n))
    cov = np.zeros((H, W), bool)
    if area2 == 0:
        return cov                                                # zero area covers nothing
    s = 1 if area2 > 0 else -1
    px = (4 * np.arange(W, dtype=np.int64) + 2)[None, :]
    py = (4 * np.arange(H, dtype=np.int64) + 2)[:, None]
    cov[:] = True
    for i in range(n):
        (ax, ay), (bx, by) = P[i], P[(i + 1) % n]
        E = lambda x, y: s * ((bx - ax) * (y - ay) - (by - ay) * (x - ax))
        right, down = E(1, 0) - E(0, 0), E(0, 1) - E(0, 0)
        top_left = right > 0 or (right == 0 and down > 0)
        e = E(px, py)
        cov &= (e > 0) | ((e == 0) & top_left)
    return cov


def signed_area4(tri):
    """16 x twice the signed screen area (x right, y down) of a triangle, an integer."""
    (ax, ay), (bx, by), (cx, cy) = [(_quarter(p[0]), _quarter(p[1])) for p in tri]
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def exact_cover(tri, H, W, cull):
    """Coverage [H, W] of one triangle ((u, v) or (u, v, Z) rows, Z > 0) under the contract.  Culling: face (a, b, c) is culled when
    dot((b - a) x (c - a), a) >= 0 in camera coordinates; that triple product is det[a b c] = Za Zb Zc / (fx fy) times the signed
    screen area above, so with every Z > 0 the face is kept exactly when that area is negative."""
    if cull and signed_area4(tri) >= 0:
        return np.zeros((H, W), bool)
    return _cover_convex([p[:2] for p in tri], H, W)


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes of separate triangles
# ---------------------------------------------------------------------------------------------------------------------------------
class Scene:
    """n triangles tris [n, 3, 3] of (u, v, Z) rows in an H x W image with principal point (cx, cy).  expect: where the coverage count
    of the n triangles must be 1 (0 elsewhere), or None where the scene makes no such claim."""

    def __init__(self, name, H, W, cx, cy, tris, cull, expect=None, dyadic=True):
        self.name, self.H, self.W, self.cx, self.cy, self.cull, self.expect = name, H, W, cx, cy, cull, expect
        self.tris = np.asarray(tris, np.float64).reshape(-1, 3, 3)
        self.K = cam(cx, cy)
        assert not dyadic or np.isin(self.tris[:, :, 2], ZS).all()
        self.verts = np.stack([np.stack([vertex(u, v, Z, cx, cy) for u, v, Z in t]) for t in self.tris])
        check_exact(self.verts.reshape(-1, 3), np.arange(3 * len(self.tris)).reshape(-1, 3), self.K, self.tris.reshape(-1, 3)[:, :2])

    def __repr__(self):
        return self.name

    def covers(self):
        return np.stack([exact_cover(t, self.H, self.W, self.cull) for t in self.tris])

    def boxes(self):
        """Pixels in every face's clipped bounding box, from the oracle's setup (all faces are kept: no znear, no cull)."""
        t = ro.setup(ro.camera_vertices(self.verts.reshape(-1, 3)), np.arange(3 * len(self.tris)).reshape(-1, 3), self.K, self.H, self.W,
                     znear=0.0, cull=False)
        n = np.zeros(len(self.tris), np.int64)
        n[t["idx"]] = (t["x1"] - t["x0"] + 1) * (t["y1"] - t["y0"] + 1)
        return n


def check_exact(verts, faces, K, uv):
    """ro.setup of the fp32 vertices returns the screen positions uv [V, 2] bit for bit (identity view, every face kept)."""
    X = ro.camera_vertices(verts)
    assert (X == np.asarray(verts, np.float64)).all()
    t = ro.setup(X, faces, K, 1 << 20, 1 << 20, znear=0.0, cull=False)
    uv = np.asarray(uv, np.float64)
    assert len(t["idx"]) == len(faces)
    f = np.asarray(faces)[t["idx"]]
    assert (t["sx"] == uv[f, 0]).all() and (t["sy"] == uv[f, 1]).all()
    return t


def one_face_per_image(scene, seed=0):
    """(images [n, H, W, 3], verts [n, 3, 3], image_index [n], K [n, 3, 3], faces [1, 3]) of a Scene: triangle p alone in image p."""
    n = len(scene.tris)
    images = np.random.default_rng(seed).integers(0, 256, (n, scene.H, scene.W, 3)).astype(np.uint8)
    return images, scene.verts, np.arange(n), np.repeat(scene.K[None], n, 0), ONE_FACE


def oracle_keys(scene):
    """The oracle's keys [n, H, W] of the one-face-per-image call (person p has id p, F = 1)."""
    return np.stack([ro.raster(ro.camera_vertices(scene.verts[p]), ONE_FACE, scene.K, scene.H, scene.W, id_base=p, cull=scene.cull)
                     for p in range(len(scene.tris))])


def _zof(u, v):
    """A depth in {1, 2, 4} that depends on the screen position alone, so that faces sharing a vertex agree on it."""
    return ZS[(_quarter(u) // 2 + 3 * (_quarter(v) // 2)) % 3]


def _wind(tri, front):
    """The triangle with its last two corners swapped if needed: front faces have a negative signed screen area."""
    tri = [tuple(p) for p in tri]
    return tri if (signed_area4(tri) < 0) == front else [tri[0], tri[2], tri[1]]


def _rect(H, W, u0, v0, u1, v1):
    """Centres with u0 <= c + 0.5 < u1 and v0 <= r + 0.5 < v1: top and left edges in, bottom and right edges out."""
    m = np.zeros((H, W), bool)
    rows = [r for r in range(H) if v0 <= r + 0.5 < v1]
    cols = [c for c in range(W) if u0 <= c + 0.5 < u1]
    m[np.ix_(rows, cols)] = True
    return m


FAN6 = [(8, 0), (4, 7), (-4, 7), (-8, 0), (-4, -7), (4, -7)]
FAN8 = [(8, 0), (6, 6), (0, 8), (-6, 6), (-8, 0), (-6, -6), (0, -8), (6, -6)]


def shared_edge_scenes():
    """Scene 1: quads split along diagonals of slope +-1, +-2, +-1/2, a 2 x 2 block of quads (horizontal and vertical shared edges),
    all with corners on pixel centres, and fans of 6 and 8 triangles around a pixel centre; both windings, cull on and off."""
    H, W = 96, 128
    out = []
    for front in (True, False):
        for cull in (True, False):
            tris, expect = [], np.zeros((H, W), bool)
            quads = [(4.5, 4.5, 16, 16, 0), (28.5, 4.5, 8, 16, 0), (44.5, 4.5, 16, 8, 0), (4.5, 28.5, 16, 16, 1), (28.5, 28.5, 8, 16, 1),
                     (44.5, 28.5, 16, 8, 1)]
            quads += [(68.5 + 8 * i, 4.5 + 6 * j, 8, 6, (i + j) % 2) for i in range(2) for j in range(2)]
            for u0, v0, w, h, anti in quads:
                tl, tr, br, bl = (u0, v0), (u0 + w, v0), (u0 + w, v0 + h), (u0, v0 + h)
                tris += [(tl, bl, tr), (tr, bl, br)] if anti else [(tl, br, tr), (tl, bl, br)]
                expect |= _rect(H, W, u0, v0, u0 + w, v0 + h)
            for (cu, cv), ring in (((20.5, 70.5), FAN6), ((60.5, 70.5), FAN8)):
                pts = [(cu + du, cv + dv) for du, dv in ring]
                tris += [((cu, cv), pts[i], pts[(i + 1) % len(pts)]) for i in range(len(pts))]
                expect |= _cover_convex(pts, H, W)
            tris = [[(u, v, _zof(u, v)) for u, v in _wind(t, front)] for t in tris]
            if cull and not front:
                expect = np.zeros((H, W), bool)
            out.append(Scene(f"shared-{'front' if front else 'back'}-{'cull' if cull else 'nocull'}", H, W, 64, 48, tris, cull, expect))
    return out


def lattice_scene(step, cells, Z, seed):
    """Scene 2: a lattice of pixel-centre vertices, the interior ones moved by whole pixels, alternating diagonals.  The jitter is
    redrawn with the next seed until every triangle keeps the sign of its area; then every centre of the lattice rectangle is
    covered exactly once, the bottom row and right column out."""
    (sx, sy), (nx, ny) = step, cells
    u0, v0 = 4.5, 4.5
    H, W = int(v0 + ny * sy + 4), int(u0 + nx * sx + 4)
    assert H <= 96 and W <= 128
    jx, jy = (sx - 1) // 2, (sy - 1) // 2
    while True:
        rng = np.random.default_rng(seed)
        du, dv = rng.integers(-jx, jx + 1, (ny + 1, nx + 1)), rng.integers(-jy, jy + 1, (ny + 1, nx + 1))
        for d in (du, dv):
            d[0], d[-1], d[:, 0], d[:, -1] = 0, 0, 0, 0
        pt = lambda i, j: (u0 + i * sx + int(du[j, i]), v0 + j * sy + int(dv[j, i]))
        tris = []
        for j in range(ny):
            for i in range(nx):
                tl, tr, br, bl = pt(i, j), pt(i + 1, j), pt(i + 1, j + 1), pt(i, j + 1)
                tris += [(tl, bl, tr), (tr, bl, br)] if (i + j) % 2 else [(tl, br, tr), (tl, bl, br)]
        if all(signed_area4(t) < 0 for t in tris):
            break
        seed += 1
    assert all(signed_area4(t) < 0 for t in tris)                  # the precondition: no folded triangle
    tris = [[(u, v, Z) for u, v in t] for t in tris]
    return Scene(f"lattice-{sx}x{sy}-Z{int(Z)}", H, W, W // 2, H // 2, tris, True, _rect(H, W, u0, v0, u0 + nx * sx, v0 + ny * sy))


def lattice_scenes():
    return [lattice_scene((4, 4), (10, 8), 1.0, 0), lattice_scene((8, 2), (6, 12), 2.0, 1), lattice_scene((2, 8), (12, 6), 4.0, 2)]


PATH_BOXES = [(1, 127), (127, 1), (8, 16), (16, 8), (2, 64), (64, 2), (4, 32), (1, 128), (128, 1), (3, 43), (43, 3), (1, 129), (129, 1),
              (10, 13), (13, 10), (2, 65), (5, 26), (1, 130), (130, 1)]
PATH_FULL, PATH_CLIP = 136, 12


def path_cut_scene(clipped):
    """Scene 3: right triangles with quarter-pixel corners whose pixel boxes hold 127, 128, 129 and 130 pixels (w x h of PATH_BOXES,
    the right angle in each of the four corners, so the first and the last pixel of a box are covered by some triangle), in a 136 x 136
    image (a 1 x 127 box needs one side that long).  clipped: the same triangles and camera in a 12 x 12 image, whose right and bottom
    borders cut every box to at most 8 x 8 pixels.  Returns (scene, box pixels it must have)."""
    tris, want = [], []
    for w, h in PATH_BOXES:
        cw, ch = max(1, min(8, w - 1)), max(1, min(8, h - 1))
        x0, y0 = PATH_CLIP - cw, PATH_CLIP - ch
        L, R, T, B = x0 + 0.25, x0 + w - 0.25, y0 + 0.25, y0 + h - 0.25
        for corner in range(4):
            a = (L if corner % 2 == 0 else R, T if corner < 2 else B)
            t = _wind([a, (R if corner % 2 == 0 else L, a[1]), (a[0], B if corner < 2 else T)], True)
            tris.append([(u, v, ZS[(corner + w + h) % 3]) for u, v in t])
            want.append(cw * ch if clipped else w * h)
    S = PATH_CLIP if clipped else PATH_FULL
    sc = Scene("path-cut-clipped" if clipped else "path-cut", S, S, 8, 8, tris, True)
    assert (sc.boxes() == np.array(want)).all()                    # the box sizes are what the scene was built for
    return sc, np.array(want)


Z_NEAR32, Z_FAR32 = np.float32(0.05), np.float32(100.0)
CLIP_ZS = [float(Z_NEAR32), float(np.nextafter(Z_NEAR32, np.float32(0))), float(Z_FAR32), float(np.nextafter(Z_FAR32, np.float32(1e9)))]


def clip_scene():
    """Scene 6: four right triangles with 16-px legs (twice the area = 256, so e / area is exact), one per image, at the depths
    float32(0.05), its fp32 predecessor, 100.0 and its fp32 successor.  The first and third lie on the clip planes and are drawn; the
    second is dropped by znear (a vertex nearer than znear) and the fourth by zfar (every fragment beyond zfar)."""
    tris = [[(u, v, Z) for u, v in _wind([(8, 8), (24, 8), (8, 24)], True)] for Z in CLIP_ZS]
    return Scene("clip-planes", 32, 32, 16, 16, tris, True, dyadic=False)


SMALL_H, SMALL_W = (1, 3, 4, 5, 9), (1, 63, 64, 65, 129)


def small_image_scenes():
    """Scene 7: every H x W of SMALL_H x SMALL_W twice: wholly covered by one large triangle, and with a small right triangle over one
    corner (the four corners in turn) whose hypotenuse passes through pixel centres."""
    out = []
    for i, H in enumerate(SMALL_H):
        for j, W in enumerate(SMALL_W):
            cx, cy = W // 2, H // 2
            full = [(u, v, _zof(u, v)) for u, v in _wind([(-200.5, -10.5), (400.5, -10.5), (100.5, 300.5)], True)]
            out.append(Scene(f"small-{H}x{W}-full", H, W, cx, cy, [full], True, np.ones((H, W), bool)))
            right, low = (i + j) % 2, ((i + j) // 2) % 2
            a = (W + 1.25 if right else -1.25, H + 1.25 if low else -1.25)
            b = (a[0] + (-4.5 if right else 4.5), a[1])
            c = (a[0], a[1] + (-4.5 if low else 4.5))
            out.append(Scene(f"small-{H}x{W}-corner{2 * low + right}", H, W, cx, cy, [[(u, v, 2.0) for u, v in _wind([a, b, c], True)]], True))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# meshes (one face array, several persons)
# ---------------------------------------------------------------------------------------------------------------------------------
def grid_mesh(nx, ny, step, u0, v0, Z, cx, cy):
    """A lattice of nx x ny quads of `step` pixels with pixel-centre vertices, alternating diagonals, wound towards the camera:
    (verts [V, 3] fp32, faces [2 nx ny, 3], uv [V, 2]).  Z: one depth, or a function of (i, j)."""
    zf = Z if callable(Z) else (lambda i, j: Z)
    uv = np.array([(u0 + i * step, v0 + j * step) for j in range(ny + 1) for i in range(nx + 1)], np.float64)
    verts = np.stack([vertex(uv[j * (nx + 1) + i, 0], uv[j * (nx + 1) + i, 1], zf(i, j), cx, cy) for j in range(ny + 1) for i in range(nx + 1)])
    faces = []
    for j in range(ny):
        for i in range(nx):
            tl, tr, bl, br = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i, (j + 1) * (nx + 1) + i + 1
            faces += [(tl, bl, tr), (tr, bl, br)] if (i + j) % 2 else [(tl, br, tr), (tl, bl, br)]
    faces = np.array(faces, np.int32)
    check_exact(verts, faces, cam(cx, cy), uv)
    return verts, faces, uv


LONG_H, LONG_W, LONG_SHIFT = 400, 512, 39


def long_list_scene():
    """Scene 4: one person, a 40 x 30 lattice of 12-px quads at Z = 2 in a 400 x 512 image: 2400 faces, each with a 13 x 13 = 169 pixel
    box, so the workgroup pass walks its list more than twice.  Returns (verts [1, V, 3], faces, K, Rt [1, 2, 3, 4]): view 1 is the
    translation t = (39 Z / 64, 0, 0), 39 whole pixels to the right: the last column of quads leaves the image and the one before it is cut
    to 9 x 13 pixel boxes, which the face's own thread draws."""
    cx, cy, Z = 256, 200, 2.0
    verts, faces, uv = grid_mesh(40, 30, 12, 8.5, 8.5, Z, cx, cy)
    K = cam(cx, cy)
    Rt = np.zeros((1, 2, 3, 4), np.float32)
    Rt[:, :, :, :3] = np.eye(3)
    Rt[0, 1, 0, 3] = LONG_SHIFT * Z / FOCAL
    assert float(Rt[0, 1, 0, 3]) == LONG_SHIFT * Z / FOCAL
    for v in range(2):
        X = ro.camera_vertices(verts, Rt[0, v, :, :3], Rt[0, v, :, 3])
        t = ro.setup(X, faces, K, LONG_H, LONG_W)
        if v == 0:
            assert len(t["idx"]) == len(faces) == 2400 and ((t["x1"] - t["x0"] + 1) * (t["y1"] - t["y0"] + 1) == 169).all()
        else:                                                      # the shifted view is as exact as the first
            f = faces[t["idx"]]
            assert (t["sx"] == uv[f, 0] + LONG_SHIFT).all() and (t["sy"] == uv[f, 1]).all()
        large = int(((t["x1"] - t["x0"] + 1) * (t["y1"] - t["y0"] + 1) > SMALL_MAX).sum())
        assert large >= 2 * LARGE_GRID + 1, large                  # the precondition: a third walk of the list in every view
    return verts[None], faces, K, Rt


def tie_scene_twins():
    """Scene 5 (a): two persons with bit-identical vertices (a 4 x 3 lattice of 8-px quads, depths 1, 2, 4 by vertex)."""
    verts, faces, _ = grid_mesh(4, 3, 8, 6.5, 5.5, lambda i, j: ZS[(i + 2 * j) % 3], 24, 16)
    return np.stack([verts, verts]), faces, cam(24, 16), 36, 48


def tie_scene_doubled():
    """Scene 5 (b): one mesh with every face listed twice (face f and face F / 2 + f are the same triangle)."""
    verts, faces, _ = grid_mesh(4, 3, 8, 6.5, 5.5, lambda i, j: ZS[(2 * i + j) % 3], 24, 16)
    return verts[None], np.concatenate([faces, faces]), cam(24, 16), 36, 48


TIE_COL = 48


def tie_scene_crossing():
    """Scene 5 (c): a fronto-parallel quad at Z = 2 (u 8.5 .. 72.5, v 8.5 .. 40.5) against a tilted quad with Z = 1 at u = 16.5 and
    Z = 4 at u = 64.5 (v 4.5 .. 44.5): 1 / Z falls by exactly 1 / 64 per pixel, so column 48 (u = 48.5) holds depth 2 from both.
    Returns (verts [2, 4, 3], faces, K, H, W): person 0 the flat quad, person 1 the tilted one."""
    cx, cy, H, W = 40, 24, 48, 80
    quad = lambda u0, v0, u1, v1, z0, z1: np.stack([vertex(u0, v0, z0, cx, cy), vertex(u1, v0, z1, cx, cy), vertex(u1, v1, z1, cx, cy),
                                                    vertex(u0, v1, z0, cx, cy)])
    flat, tilt = quad(8.5, 8.5, 72.5, 40.5, 2.0, 2.0), quad(16.5, 4.5, 64.5, 44.5, 1.0, 4.0)
    faces = np.array([[0, 2, 1], [0, 3, 2]], np.int32)
    K = cam(cx, cy)
    check_exact(flat, faces, K, [(8.5, 8.5), (72.5, 8.5), (72.5, 40.5), (8.5, 40.5)])
    check_exact(tilt, faces, K, [(16.5, 4.5), (64.5, 4.5), (64.5, 44.5), (16.5, 44.5)])
    return np.stack([flat, tilt]), faces, K, H, W


def tied_pixels(verts, faces, K, H, W):
    """Pixels at which the two persons of a tie scene, rastered alone, hold the same depth bits (both covered)."""
    k = [ro.raster(ro.camera_vertices(verts[p]), faces, K, H, W) for p in range(2)]
    both = (k[0] != ro.KEY_NONE) & (k[1] != ro.KEY_NONE)
    return both & ((k[0] >> np.uint64(32)) == (k[1] >> np.uint64(32)))


def nonfinite_scene():
    """Scene 8: three persons (a 3 x 3 lattice of 10-px quads each, overlapping on screen at depths 2, 1 and 4) in one image.  Returns
    (verts [3, 16, 3], broken [16, 3], behind [16, 3], faces, K, H, W): `broken` replaces the middle person by NaN in x, y or z of some
    vertices and +-Inf in x or y of others, so that every face touches at least one such vertex; `behind` puts it wholly behind the
    camera instead, which draws nothing either and leaves the other persons' ids as they are."""
    cx, cy, H, W = 32, 24, 48, 64
    m = [grid_mesh(3, 3, 10, u0, v0, Z, cx, cy)[0] for u0, v0, Z in ((6.5, 6.5, 2.0), (14.5, 10.5, 1.0), (24.5, 12.5, 4.0))]
    faces = grid_mesh(3, 3, 10, 6.5, 6.5, 2.0, cx, cy)[1]
    broken = m[1].copy()
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for v, (axis, val) in {0: (0, nan), 2: (1, inf), 5: (2, nan), 7: (0, -inf), 8: (1, nan), 10: (0, inf), 13: (1, -inf), 15: (0, nan),
                           3: (2, nan), 12: (0, nan)}.items():
        broken[v, axis] = val
    bad = ~np.isfinite(broken).all(1)
    assert bad[faces].any(1).all() and not bad.all()               # every face touches a non-finite vertex; finite vertices remain
    behind = m[1].copy()
    behind[:, 2] = -1.0
    return np.stack(m), broken, behind, faces, cam(cx, cy), H, W


# ---------------------------------------------------------------------------------------------------------------------------------
# the one scene that is NOT exact: shared edges whose edge function rounds
# ---------------------------------------------------------------------------------------------------------------------------------
class Seams:
    """Pairs of triangles (A, B, R1), (B, A, R2) over a shared edge A-B, one face per image like a Scene."""

    def __init__(self, verts, centres, H, W, cx, cy):
        self.name, self.verts, self.centres, self.H, self.W, self.K, self.cull = "rounded-seams", verts, centres, H, W, cam(cx, cy), False
        self.tris = verts                                          # len() = number of images

    def __repr__(self):
        return self.name


def _naive_cover(tri, x, y):
    """Coverage of (x, y) by a screen triangle when every edge is evaluated from the face's own winding, b - a first: the form that
    csrc/render.hip's edge_fn avoids.  fp64, one rounding per operation."""
    A = (tri[1][0] - tri[0][0]) * (tri[2][1] - tri[0][1]) - (tri[1][1] - tri[0][1]) * (tri[2][0] - tri[0][0])
    s = 1.0 if A > 0 else -1.0
    for i in range(3):
        (ax, ay), (bx, by) = tri[(i + 1) % 3], tri[(i + 2) % 3]
        e = s * ((bx - ax) * (y - ay) - (by - ay) * (x - ax))
        dx, dy = s * (bx - ax), s * (by - ay)
        if not (e > 0 or (e == 0 and ((dy == 0 and dx > 0) or dy < 0))):
            return False
    return True


def rounded_seam_scene(pairs=12, seed=0):
    """Shared edges at Z = 3, where the projection 64 x / 3 + cx rounds: the endpoints A = c - k1 d and B = c + k2 d lie about a pixel
    centre c, so c is on the edge up to the rounding of A and B, and the edge function at c is a difference of two nearly equal
    products.  Kept are the edges for which evaluating A -> B in the one face and B -> A in the other (each face's own winding) would
    draw c twice or not at all: only one fixed endpoint order for both faces, as the contract demands, draws it exactly once.  That
    property needs no exact arithmetic, and the scene asserts nothing else about these pixels."""
    Z, cx, cy, H, W = 3.0, 32, 24, 48, 64
    rng = np.random.default_rng(seed)
    verts, centres = [], []
    proj = lambda v: ((FOCAL * float(v[0])) / float(v[2]) + cx, (FOCAL * float(v[1])) / float(v[2]) + cy)
    while len(centres) < pairs:
        m, n = int(rng.integers(8, W - 8)), int(rng.integers(8, H - 8))
        p, q = int(rng.integers(-40, 41)) / 64, int(rng.integers(-40, 41)) / 64
        k1, k2 = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        if abs(p) + abs(q) < 0.25:
            continue
        c = np.array([(m + 0.5 - cx) * Z / FOCAL, (n + 0.5 - cy) * Z / FOCAL])
        d, nrm = np.array([p, q]), np.array([-q, p])
        A, B, R1, R2 = (np.float32(np.append(c + off, Z)) for off in (-k1 * d, k2 * d, nrm, -nrm))
        t1, t2 = [proj(A), proj(B), proj(R1)], [proj(B), proj(A), proj(R2)]
        if _naive_cover(t1, m + 0.5, n + 0.5) + _naive_cover(t2, m + 0.5, n + 0.5) == 1:
            continue                                               # this edge would not tell the two forms apart
        verts += [np.stack([A, B, R1]), np.stack([B, A, R2])]
        centres.append((n, m))
    return Seams(np.stack(verts), centres, H, W, cx, cy)
