"""-m "not gpu": the mesh-overlay entry points are declared and exported, and the CPU oracle of the render contract
(tests/render_oracle.py) agrees with the contract's closed forms and with the reference's own mask smoothing."""
import os
import re

import numpy as np
import pytest
import torch

import render_oracle as ro
from multi_hmr_amd import _lib, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_entries_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    for sym in ("mhmr_render_workspace_bytes", "mhmr_render_meshes"):
        assert sym in declared and sym in _lib.EXPORTS, sym
    assert "typedef struct" in header and "} mhmr_render_desc;" in header
    assert "render.hip" in _lib.SOURCES and "-ffp-contract=off" in _lib.EXTRA_FLAGS["render.hip"]


def _desc(**kw):
    d = _lib.RenderDesc()
    d.B, d.H, d.W, d.P, d.V, d.F, d.vstride = 2, 48, 64, 3, 100, 196, 300
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_library_builds_with_render_and_validates_shapes_before_launch():
    import ctypes as C
    _lib.build()
    L = _lib.lib()
    good = L.mhmr_render_workspace_bytes(C.byref(_desc()))
    # camera vertices (fp64) + normals (fp32) + keys + large-face list, each 256-byte aligned
    assert good >= 3 * 100 * 24 + 3 * 100 * 12 + 2 * 48 * 64 * 8 + 3 * 196 * 4
    for bad in (dict(B=0), dict(H=0), dict(P=-1), dict(vstride=299), dict(F=0), dict(P=70000, F=70000), dict(B=70000)):
        assert L.mhmr_render_workspace_bytes(C.byref(_desc(**bad))) == -2, bad
        assert L.mhmr_render_meshes(C.byref(_desc(**bad)), None) == -2, bad     # refused before anything is launched
    assert L.mhmr_render_meshes(None, None) == -1
    assert L.mhmr_render_meshes(C.byref(_desc()), None) == -1                      # null images / workspace


def test_csr_lists_incident_faces_in_face_order():
    faces = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 2], [0, 2, 4]], np.int32)
    off, adj = render.build_csr(faces, 6)
    assert off.tolist() == [0, 2, 4, 8, 10, 12, 12]
    for v in range(6):
        e = adj[off[v]:off[v + 1]]
        assert (faces.reshape(-1)[e] == v).all() and (np.diff(e // 3) > 0).all()
    with pytest.raises(ValueError):
        render.build_csr(faces, 4)


def _cam(f=100.0, W=64, H=48):
    return np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)


def test_axis_aligned_quad_covers_the_expected_pixels():
    """A quad with corners at screen (10.2, 7.7) - (30.6, 21.3) covers the centres c + 0.5 in that box: cols 10..30, rows 8..20."""
    K = _cam()
    Z = 2.0
    u0, v0, u1, v1 = 10.2, 7.7, 30.6, 21.3
    to3 = lambda u, v: [(u - 32) * Z / 100, (v - 24) * Z / 100, Z]
    x = np.array([to3(u0, v0), to3(u1, v0), to3(u1, v1), to3(u0, v1)], np.float32)
    faces = np.array([[0, 2, 1], [0, 3, 2]], np.int32)                       # facing the camera (kept by the cull)
    keys = ro.raster(ro.camera_vertices(x), faces, K, 48, 64)
    cov = keys != ro.KEY_NONE
    exp = np.zeros_like(cov)
    exp[8:21, 10:31] = True                                                   # rows with r + 0.5 in [7.7, 21.3], cols in [10.2, 30.6]
    assert (cov == exp).all()
    # the other winding faces away and is culled; without culling it draws the same pixels
    assert (ro.raster(ro.camera_vertices(x), faces[:, ::-1], K, 48, 64) == ro.KEY_NONE).all()
    assert ((ro.raster(ro.camera_vertices(x), faces[:, ::-1], K, 48, 64, cull=False) != ro.KEY_NONE) == exp).all()


def test_shared_edges_cover_each_pixel_exactly_once():
    """Two triangles of a quad whose shared edges pass exactly through pixel centres (a horizontal top edge, a vertical edge,
    a diagonal): every centre of the quad is covered by exactly one of them.  f = 64 and Z = 1 make the corners exact in fp32."""
    K = _cam(f=64.0)
    Z = 1.0
    to3 = lambda u, v: [(u - 32) * Z / 64, (v - 24) * Z / 64, Z]
    for quad, split in (([(4.5, 4.5), (20.5, 4.5), (20.5, 20.5), (4.5, 20.5)], "diag"),
                        ([(4.5, 4.5), (12.5, 4.5), (12.5, 12.5), (4.5, 12.5)], "diag"),
                        ([(2.5, 2.5), (30.5, 2.5), (30.5, 8.5), (2.5, 8.5)], "diag")):
        x = np.array([to3(*p) for p in quad], np.float32)
        faces = [np.array([[0, 2, 1]], np.int32), np.array([[0, 3, 2]], np.int32)]
        c = [ro.raster(ro.camera_vertices(x), f, K, 48, 64) != ro.KEY_NONE for f in faces]
        assert not (c[0] & c[1]).any()
        both = c[0] | c[1]
        (u0, v0), (u1, v1) = quad[0], quad[2]
        exp = np.zeros_like(both)
        rows = [r for r in range(48) if v0 <= r + 0.5 <= v1]
        cols = [cc for cc in range(64) if u0 <= cc + 0.5 <= u1]
        exp[np.ix_(rows, cols)] = True
        # the quad's own boundary follows the top-left rule: its top and left edges are in, its bottom and right edges out
        exp[rows[-1], :] = False
        exp[:, cols[-1]] = False
        assert (both == exp).all()
    # a fan of 6 triangles around a centre that is itself a pixel centre: covered exactly once
    ctr = (20.5, 20.5)
    ring = [(ctr[0] + 8 * np.cos(a), ctr[1] + 8 * np.sin(a)) for a in np.linspace(0, 2 * np.pi, 7)[:-1]]
    x = np.array([to3(*ctr)] + [to3(*p) for p in ring], np.float32)
    cnt = np.zeros((48, 64), int)
    for i in range(6):
        f = np.array([[0, 1 + i, 1 + (i + 1) % 6]], np.int32)
        cnt += ro.raster(ro.camera_vertices(x), f, K, 48, 64, cull=False) != ro.KEY_NONE
    assert cnt.max() == 1 and cnt[20, 20] == 1


def test_mask_matches_the_reference_conv2d_smoothing():
    """utils/render.py:302-311 restated with torch: clamp_min(conv2d(fg, 2/9 ones(3,3), bias -1, padding 1) * fg, 0).  conv2d sums
    nine rounded terms in its own order, so the two agree to 1 ulp of that sum (k 2/9, near 1 to 2); subtracting the bias
    then leaves the same absolute difference on a smaller m."""
    g = np.random.default_rng(0)
    for p in (0.2, 0.5, 0.9):
        fg = g.random((61, 77)) < p
        t = torch.from_numpy(fg.astype(np.float32))[None]
        kern = 2.0 * torch.ones((1, 1, 3, 3)) / 9
        ref = torch.clamp_min(torch.nn.functional.conv2d(t, weight=kern, bias=-torch.ones(1), padding=1) * t, 0.0)[0].numpy()
        m = ro.mask(fg)
        assert m.dtype == np.float32
        ulp = np.spacing((ref + np.float32(1)).astype(np.float32))
        assert (np.abs(m - ref) <= ulp).all()
        assert (m[ref == 0] == 0).all() and (m[ref == 1] == 1).all()
        assert ((m > 0) <= fg).all()


def test_shading_at_normal_incidence_equals_the_closed_form():
    """n = v = l: nl = nv = nh = vh = 1, F = f0, G = 1, D = 1 / (pi a^2):
    c = I ((1 - f0) c_diff / pi + f0 / (4 pi a^2)) + A b."""
    n = np.array([[0.0, 0.0, -1.0]] * 3)
    base = np.array([[0.2, 0.5, 0.9], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
    for m, rho, I in ((0.0, 0.5, 3.0), (0.3, 0.8, 2.0)):
        c = ro.shade_colour(n, n, base, intensity=I, ambient=0.3, metallic=m, roughness=rho)
        a2 = rho ** 4
        f0 = 0.04 * (1 - m) + base * m
        cdiff = base * 0.96 * (1 - m)
        exp = I * ((1 - f0) * cdiff / np.pi + f0 / (4 * np.pi * a2)) + 0.3 * base
        assert np.allclose(c, exp, rtol=1e-12, atol=0)
    assert ro.to_rgb(np.array([0.0, 1.0, 5.0])).tolist() == [0, 255, 255]


def test_blend_is_the_fp32_expression_and_leaves_uncovered_pixels():
    g = np.random.default_rng(1)
    img = g.integers(0, 256, (9, 11, 3)).astype(np.uint8)
    rgb = g.integers(0, 256, (9, 11, 3)).astype(np.float64)
    cov = g.random((9, 11)) < 0.6
    m = ro.mask(cov)
    for a in (0.0, 0.8, 1.0):
        out = ro.blend(img, rgb, m, a)
        assert (out[~cov] == img[~cov]).all()
        if a == 0.0:
            assert (out == img).all()
        if a == 1.0:
            full = m == 1
            assert (out[full] == rgb[full]).all()


def test_oracle_icosphere_and_normals():
    v, f = ro.icosphere(2)
    assert v.shape == (162, 3) and f.shape == (320, 3)
    n = ro.vertex_normals(v, f)
    assert np.allclose(np.einsum("vk,vk->v", n, v), 1.0, atol=2e-3)     # outward, close to the radius on a sphere
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.einsum("fk,fk->f", fn, v[f].mean(1)) > 0).all()           # faces wound outward


def test_render_meshes_rejects_before_touching_the_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("reached the library")
    monkeypatch.setattr(render, "render_batch", boom)
    img = np.zeros((8, 8, 3), np.uint8)
    v, f = ro.icosphere(0)
    cam = {"focal": np.array([10.0, 10.0]), "princpt": np.array([4.0, 4.0])}
    with pytest.raises(NotImplementedError):
        render.render_meshes(img, [v], [f], cam, show_camera=True)
    with pytest.raises(ValueError):
        render.render_meshes(img, [v, v], [f, f[::-1].copy()], cam)
    assert (render.render_meshes(img, [], [], cam) == img).all()


def test_palette_starts_with_the_reference_demo_colours():
    assert render.PALETTE[0] == (0x00 / 255, 0x47 / 255, 0xAB / 255) and render.PALETTE[9] == (0x99 / 255, 0x33 / 255, 0xFF / 255)
    assert len(render.PALETTE) == 210 and all(0 <= c <= 1 for col in render.PALETTE for c in col)
