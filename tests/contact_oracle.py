"""numpy restatement of the contact contract (include/mhmr.h, mhmr_contact_desc) at any dtype, the scene builders of the contact tests
and the comparison rules.  fp64 is the yardstick; the cull (validity, boxes, which pairs and vertices are evaluated, which faces are
skipped) is done in fp32 exactly as the contract says, whatever the dtype of the distance arithmetic.

The oracle follows Ericson's text (Real-Time Collision Detection 5.1.5) region by region, with the closest point formed per region
(a + v ab, b + u (c - b), ...); the kernel forms one pair of barycentric parameters instead.  The two agree to rounding."""
import numpy as np

F32 = np.float32

#: gate of the float outputs against the fp64 oracle on the same fp32 inputs, in metres: 4 x the worst error measured on the GPU over
#: the scenes of tests/test_gpu_contact.py (profiles/contact_tests.txt: 4.27e-7 m, the reported closest point, which is rounded to fp32
#: at the size of the coordinates; the signed distance itself is within 4.7e-8 m).  It must stay below
#: 16 * 2^-23 * M, M the largest coordinate magnitude of a scene (1.3e-5 m at M = 6.8): see ``gate_ceiling``.
GATE = 4 * 4.27e-7
GUARD_D, GUARD_W, GUARD_TAU, GUARD_CAP = 1e-4, 0.05, 1e-4, 0.02


def gate_ceiling(verts):
    v = np.asarray(verts, np.float64)
    return 16 * 2.0 ** -23 * float(np.abs(v[np.isfinite(v)]).max())


# ------------------------------------------------------------------------------------------------------------------- scenes
def icosphere(level):
    """Unit sphere, closed, outward-oriented: 12 / 20 at level 0, 162 / 320 at level 2, 642 / 1280 at level 3 (float64, int32)."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, float) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, np.int32)


def box():
    """The cube [-0.5, 0.5]^3, closed, outward-oriented: 8 vertices (index = 4 x + 2 y + z of the corner bits), 12 faces."""
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], float)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], np.int32)
    return v, f


def torus(nu, nv, R=0.5, r=0.15):
    """Torus around the z axis (centre-line radius R, tube radius r), closed, outward-oriented: nu nv vertices, 2 nu nv faces."""
    u = 2 * np.pi * np.arange(nu) / nu
    w = 2 * np.pi * np.arange(nv) / nv
    U, W = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    f = []
    for i in range(nu):
        for j in range(nv):
            f += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return v, np.array(f, np.int32)


def signed_volume(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6)


def open_sphere(level, zcut=0.8):
    """The icosphere without the faces that have a corner above z = zcut: a cap removed, the vertices kept."""
    v, f = icosphere(level)
    return v, f[(v[f][:, :, 2] <= zcut).all(1)]


def inverted(f):
    return np.ascontiguousarray(f[:, ::-1])


def with_degenerate(f, n=3):
    """n faces with a repeated corner appended: (0, 0, 1), (2, 3, 3), (5, 5, 5), then (k, k, k + 1)."""
    extra = [(0, 0, 1), (2, 3, 3), (5, 5, 5)] + [(k % 7, k % 7, k % 7 + 1) for k in range(max(0, n - 3))]
    return np.concatenate([f, np.array(extra[:n], np.int32).reshape(-1, 3)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------- oracle
def closest_on_triangles(p, a, b, c):
    """Closest points [n, F, 3] of the triangles (a, b, c) [F, 3] to the points p [n, 3], in p's dtype: Ericson's region tests in his
    order (vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, interior)."""
    P = p[:, None, :]
    ab, ac = (b - a)[None], (c - a)[None]
    ap, bp, cp = P - a[None], P - b[None], P - c[None]
    dot = lambda x, y: (x * y).sum(-1)
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    out = np.empty(ap.shape, p.dtype)
    done = np.zeros(ap.shape[:2], bool)

    def put(m, val):
        m = m & ~done
        out[m] = np.broadcast_to(val, out.shape)[m]
        done[m] = True
    with np.errstate(all="ignore"):
        put((d1 <= 0) & (d2 <= 0), a[None])
        put((d3 >= 0) & (d4 <= d3), b[None])
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a[None] + (d1 / (d1 - d3))[..., None] * ab)
        put((d6 >= 0) & (d5 <= d6), c[None])
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a[None] + (d2 / (d2 - d6))[..., None] * ac)
        put((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b[None] + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (c - b)[None])
        den = 1 / (va + vb + vc)
        put(np.ones_like(done), a[None] + ab * (vb * den)[..., None] + ac * (vc * den)[..., None])
    return out


def winding(p, a, b, c):
    """Winding numbers [n] of the points p [n, 3] about the triangles (a, b, c) [F, 3], summed in ascending face order."""
    A, B, C = a[None] - p[:, None], b[None] - p[:, None], c[None] - p[:, None]
    la, lb, lc = (np.sqrt((x * x).sum(-1)) for x in (A, B, C))
    num = (A * np.cross(B, C)).sum(-1)
    den = la * lb * lc + (A * B).sum(-1) * lc + (B * C).sum(-1) * la + (C * A).sum(-1) * lb
    th = 2 * np.arctan2(num, den)
    w = np.zeros(len(p), p.dtype)
    for k in range(th.shape[1]):                                        # ascending, one rounding per face
        w = w + th[:, k]
    return w / p.dtype.type(4 * np.pi)


def kept_faces(vb32, faces):
    """The faces of a person that are not skipped: the fp32 normal, every operation rounded on its own, is not the zero vector."""
    a, b, c = vb32[faces[:, 0]], vb32[faces[:, 1]], vb32[faces[:, 2]]
    u, v = (b - a).astype(F32), (c - a).astype(F32)
    n = np.stack([(u[:, 1] * v[:, 2]).astype(F32) - (u[:, 2] * v[:, 1]).astype(F32),
                  (u[:, 2] * v[:, 0]).astype(F32) - (u[:, 0] * v[:, 2]).astype(F32),
                  (u[:, 0] * v[:, 1]).astype(F32) - (u[:, 1] * v[:, 0]).astype(F32)], 1).astype(F32)
    return np.nonzero((n != 0).any(1))[0]


def contacts(verts, image_index, faces, max_dist=0.10, tau=0.01, dtype=np.float64, chunk=256):
    """The contract on verts [P, V, 3] (taken as fp32), image_index [P], faces [F, 3].  Returns the eleven outputs by name (the float
    ones in ``dtype``, aabb in fp32) and, under "detail", what the comparison rules need per ordered pair: ``pair`` [P, P] bool (the pair
    is evaluated), ``evaluated`` [P, P, V] bool, ``d`` and ``w`` [P, P, V] (distance and winding number; w = 0 where the vertex is
    outside b's un-inflated box and the sum is not taken), ``s`` [P, P, V] (signed distance, +inf where not evaluated)."""
    v32 = np.ascontiguousarray(verts, F32)
    P, V = v32.shape[:2]
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    idx = np.asarray(image_index).reshape(-1)
    m, dt = F32(max_dist), np.dtype(dtype).type
    valid = np.isfinite(v32.reshape(P, -1)).all(1) if V else np.ones(P, bool)
    aabb = np.empty((P, 6), F32)
    for p in range(P):
        ok = valid[p] and V
        aabb[p, :3] = v32[p].min(0) if ok else np.inf
        aabb[p, 3:] = v32[p].max(0) if ok else -np.inf
    lo, hi = (aabb[:, :3] - m).astype(F32), (aabb[:, 3:] + m).astype(F32)
    inf = dt(np.inf)
    det = dict(pair=np.zeros((P, P), bool), evaluated=np.zeros((P, P, V), bool), d=np.full((P, P, V), inf), w=np.zeros((P, P, V), dtype),
               s=np.full((P, P, V), inf))
    cl = np.zeros((P, P, V, 3), dtype)
    nf = np.full((P, P, V), -1, np.int64)
    for a in range(P):
        for b in range(P):
            if a == b or not (valid[a] and valid[b]) or idx[a] != idx[b]:
                continue
            if not ((lo[a] <= hi[b]).all() and (lo[b] <= hi[a]).all()):
                continue
            det["pair"][a, b] = True
            live = ((lo[b] <= v32[a]) & (v32[a] <= hi[b])).all(1)
            inbox = live & ((aabb[b, :3] <= v32[a]) & (v32[a] <= aabb[b, 3:])).all(1)
            det["evaluated"][a, b] = live
            keep = kept_faces(v32[b], faces)
            if not len(keep) or not live.any():
                continue
            vb = v32[b].astype(dtype)
            fa, fb, fc = vb[faces[keep, 0]], vb[faces[keep, 1]], vb[faces[keep, 2]]
            rows = np.nonzero(live)[0]
            for r0 in range(0, len(rows), chunk):
                r = rows[r0:r0 + chunk]
                p = v32[a, r].astype(dtype)
                c = closest_on_triangles(p, fa, fb, fc)
                diff = p[:, None] - c
                d2 = (diff * diff).sum(-1)
                k = d2.argmin(1)                                        # the first minimum: the lowest face index
                det["d"][a, b, r] = np.sqrt(d2[np.arange(len(r)), k])
                cl[a, b, r] = c[np.arange(len(r)), k]
                nf[a, b, r] = keep[k]
                wi = inbox[r]
                if wi.any():
                    det["w"][a, b, r[wi]] = winding(p[wi], fa, fb, fc)
            inside = inbox & (np.abs(det["w"][a, b]) > 0.5)
            det["s"][a, b, live] = np.where(inside[live], -det["d"][a, b, live], det["d"][a, b, live])
    det["inside"] = det["evaluated"] & (det["s"] < 0)
    out = dict(sdf=np.full((P, V), inf), nearest_person=np.full((P, V), -1, np.int32), nearest_face=np.full((P, V), -1, np.int32),
               closest=v32.astype(dtype), valid=valid.astype(np.uint8), aabb=aabb, detail=det)
    for a in range(P):
        for b in range(P):                                              # b ascending, strict <
            s = det["s"][a, b]
            better = (s <= dt(m)) & (s < out["sdf"][a])
            out["sdf"][a, better] = s[better]
            out["nearest_person"][a, better] = b
            out["nearest_face"][a, better] = nf[a, b, better]
            out["closest"][a, better] = cl[a, b, better]
    sdf = out["sdf"]
    out["penetration_depth"] = np.maximum(0, -sdf).max(1) if V else np.zeros(P, dtype)
    out["inside_count"] = (sdf < 0).sum(1).astype(np.int32)
    out["contact_count"] = (np.abs(sdf) <= dt(F32(tau))).sum(1).astype(np.int32)
    pd = det["s"].min(2) if V else np.full((P, P), inf)
    out["pair_distance"] = np.where(pd <= dt(m), pd, inf)
    out["pair_inside"] = det["inside"].sum(2).astype(np.int32)
    return out


def point_triangle_distance(p, tri):
    """fp64 distance from the point p [3] to the triangle tri [3, 3]."""
    p = np.asarray(p, np.float64)[None]
    t = np.asarray(tri, np.float64)
    c = closest_on_triangles(p, t[0:1], t[1:2], t[2:3])[0, 0]
    return float(np.sqrt(((p[0] - c) ** 2).sum()))


# --------------------------------------------------------------------------------------------------------------- comparison
def guard_set(ref, tau):
    """[P, P, V] bool: the evaluated (v, b) whose sign or count the fp32 kernel may decide differently: fp64 d < 1e-4 m, ||w| - 0.5| <
    0.05, or |d - tau| < 1e-4 m.  Asserts the cap: at most 2 % of the evaluated vertices, from the oracle alone."""
    det = ref["detail"]
    g = det["evaluated"] & ((det["d"] < GUARD_D) | (np.abs(np.abs(det["w"]) - 0.5) < GUARD_W) | (np.abs(det["d"] - float(F32(tau))) < GUARD_TAU))
    n = int(det["evaluated"].sum())
    assert g.sum() <= GUARD_CAP * n, (int(g.sum()), n)
    return g


def compare(got, ref, verts, faces, max_dist, tau, gate=None):
    """Asserts the rules of the contact tests on ``got`` (name -> numpy array, the kernel's outputs; all eleven) against ``ref`` (the
    fp64 ``contacts`` of the same fp32 inputs) and returns the worst absolute errors found, in metres."""
    gate = GATE if gate is None else gate
    v32 = np.ascontiguousarray(verts, F32)
    v64 = v32.astype(np.float64)
    P, V = v32.shape[:2]
    det = ref["detail"]
    assert gate < gate_ceiling(v32)
    g3 = guard_set(ref, tau)
    clear = ~g3.any(1)                                                  # [P, V]: no evaluated b of this vertex is in the guard set
    # exact: validity, boxes, the cull
    assert np.array_equal(got["valid"], ref["valid"]) and np.array_equal(got["aabb"].view(np.uint32), ref["aabb"].view(np.uint32))
    sdf, np_, nf, cl = got["sdf"], got["nearest_person"], got["nearest_face"], got["closest"]
    assert np.array_equal(np.isinf(sdf)[clear], np.isinf(ref["sdf"])[clear])
    assert not np.isnan(sdf).any() and (sdf[np.isinf(sdf)] > 0).all() and (sdf[np.isfinite(sdf)] <= F32(max_dist)).all()
    assert not (np.isfinite(sdf) & ~det["evaluated"].any(1)).any()      # nothing outside the cull is ever reported
    # the kernel's own outputs hang together, exactly
    empty = np.isinf(sdf)
    assert np.array_equal(np_ == -1, empty) and np.array_equal(nf == -1, empty)
    assert np.array_equal(cl[empty].view(np.uint32), v32[empty].view(np.uint32))
    assert np.array_equal(got["inside_count"], (sdf < 0).sum(1)) and np.array_equal(got["contact_count"], (np.abs(sdf) <= F32(tau)).sum(1))
    pen = np.maximum(F32(0), -sdf).max(1) if V else np.zeros(P, F32)
    assert np.array_equal(got["penetration_depth"].view(np.uint32), pen.astype(F32).view(np.uint32))
    # against fp64, on the vertices outside the guard set
    worst = dict(sdf=0.0, closest=0.0, nearest_face=0.0, pair_distance=0.0, penetration_depth=0.0)
    fin = clear & ~empty
    if fin.any():
        worst["sdf"] = float(np.abs(sdf[fin].astype(np.float64) - ref["sdf"][fin]).max())
        assert worst["sdf"] <= gate, worst
        assert np.array_equal(np.sign(sdf[fin]), np.sign(ref["sdf"][fin]))
    faces = np.asarray(faces, np.int64)
    for a, n in zip(*np.nonzero(fin)):
        b, f = int(np_[a, n]), int(nf[a, n])
        assert det["evaluated"][a, b, n] and abs(det["s"][a, b, n] - ref["sdf"][a, n]) <= gate           # the lowest b on a tie, or a near tie
        ties = np.nonzero(det["s"][a, :, n] == ref["sdf"][a, n])[0]
        if len(ties) > 1 and b in ties:                                 # identical meshes: the same bits in the kernel too
            assert b == ties[0], (a, n, b, ties)
        tri = v64[b][faces[f]]
        e = abs(point_triangle_distance(v64[a, n], tri) - det["d"][a, b, n])       # the reported face attains the minimum
        worst["nearest_face"] = max(worst["nearest_face"], e)
        c = cl[a, n].astype(np.float64)                                              # the reported point lies on it, at the distance
        e = max(point_triangle_distance(c, tri), abs(np.sqrt(((v64[a, n] - c) ** 2).sum()) - det["d"][a, b, n]))
        worst["closest"] = max(worst["closest"], e)
    assert worst["nearest_face"] <= gate and worst["closest"] <= gate, worst
    assert np.array_equal(got["inside_count"][clear.all(1)], ref["inside_count"][clear.all(1)])
    assert np.array_equal(got["contact_count"][clear.all(1)], ref["contact_count"][clear.all(1)])
    for a in range(P):
        if clear[a].all() and V:
            e = abs(float(got["penetration_depth"][a]) - float(ref["penetration_depth"][a]))
            worst["penetration_depth"] = max(worst["penetration_depth"], e)
        for b in range(P):
            gi, gd = int(got["pair_inside"][a, b]), float(got["pair_distance"][a, b])
            if not det["pair"][a, b]:
                assert gi == 0 and gd == np.inf
                continue
            ng = int(g3[a, b].sum())
            sure = int((det["inside"][a, b] & ~g3[a, b]).sum())
            assert sure <= gi <= sure + ng, (a, b, gi, sure, ng)
            if ng == 0:
                rd = float(ref["pair_distance"][a, b])
                assert (gd == np.inf) == (rd == np.inf), (a, b, gd, rd)
                if rd != np.inf:
                    worst["pair_distance"] = max(worst["pair_distance"], abs(gd - rd))
    assert worst["pair_distance"] <= gate and worst["penetration_depth"] <= gate, worst
    return worst
