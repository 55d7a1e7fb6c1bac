"""-m "not gpu": the exact scenes of tests/render_exact.py on the CPU.  The numpy oracle's coverage equals `exact_cover` (integer
arithmetic from the header's wording) on every pixel of every scene, the one-face-per-image coverage count is 1 on every centre of a
scene's region and 0 elsewhere (top and left edges in, bottom and right edges out), and every precondition the GPU file relies on
holds.  Building a scene already asserts that its vertices are fp32 numbers that project back to their screen positions bit for bit
(render_exact.check_exact): a scene that is ever edited into a rounding scene fails here, without a GPU."""
import numpy as np
import pytest

import render_exact as rx
import render_oracle as ro

SCENES = rx.shared_edge_scenes() + rx.lattice_scenes() + [rx.path_cut_scene(False)[0], rx.path_cut_scene(True)[0], rx.clip_scene()] + \
    rx.small_image_scenes()


def test_exact_cover_follows_the_top_left_rule():
    """Hand-checked cases of the third party itself: a pixel-centre square keeps its top and left edges, and a triangle keeps the
    centres on its left-leaning hypotenuse only when the interior lies to their right."""
    sq = [(2.5, 1.5), (6.5, 1.5), (6.5, 4.5), (2.5, 4.5)]
    exp = np.zeros((8, 8), bool)
    exp[1:4, 2:6] = True                                           # rows 1..3 (v 1.5 in, 4.5 out), cols 2..5 (u 2.5 in, 6.5 out)
    assert np.array_equal(rx._cover_convex(sq, 8, 8), exp) and np.array_equal(rx._cover_convex(sq[::-1], 8, 8), exp)
    lower = rx.exact_cover([(0.5, 0.5), (0.5, 4.5), (4.5, 4.5)], 6, 6, False)        # interior below the diagonal u = v: a right edge
    assert [tuple(p) for p in np.argwhere(lower)] == [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]
    upper = rx.exact_cover([(0.5, 0.5), (4.5, 4.5), (4.5, 0.5)], 6, 6, False)        # interior above it: the diagonal is a left edge
    assert [tuple(p) for p in np.argwhere(upper)] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]
    assert not (lower & upper).any()
    # culling keeps the negative signed screen area (the winding test_render_host's quad faces the camera with)
    assert rx.exact_cover([(0.5, 0.5), (4.5, 4.5), (4.5, 0.5)], 6, 6, True).sum() == 10
    assert rx.exact_cover([(0.5, 0.5), (4.5, 0.5), (4.5, 4.5)], 6, 6, True).sum() == 0
    assert rx.exact_cover([(0.5, 0.5), (2.5, 2.5), (4.5, 4.5)], 6, 6, False).sum() == 0      # zero area


@pytest.mark.parametrize("scene", SCENES, ids=repr)
def test_oracle_coverage_equals_exact_cover(scene):
    cov = scene.covers()
    if scene.name == "clip-planes":
        # only the faces on the planes draw: the second has its vertices nearer than znear, the fourth every fragment beyond zfar.
        # znear is the descriptor's fp32 field, fl32(0.05); render_oracle.ZNEAR is that number.  The double 0.05 would decide the same
        # here, since under the identity view depths are fp32 numbers and none lies between 0.05 and fl32(0.05).
        assert ro.ZNEAR == float(np.float32(0.05)) and float(np.nextafter(np.float32(0.05), np.float32(0))) < 0.05 < ro.ZNEAR
        cov[1] = cov[3] = False
        assert cov[0].sum() == cov[2].sum() == 120
    assert np.array_equal(rx.oracle_keys(scene) != ro.KEY_NONE, cov)
    if scene.expect is not None:
        assert np.array_equal(cov.sum(0), scene.expect.astype(np.int64))
    if scene.name.endswith("-full"):
        assert cov.all()
    if "corner" in scene.name:                                     # the corner pixel is drawn, and the image is not filled
        corner = int(scene.name[-1])
        assert cov[0, -1 if corner >= 2 else 0, -1 if corner % 2 else 0] and ((scene.H, scene.W) == (1, 1) or not cov.all())


def test_shared_edge_and_lattice_regions_are_not_trivial():
    front = rx.shared_edge_scenes()[0]
    assert front.expect.sum() == 2 * 256 + 4 * 128 + 4 * 48 + rx._cover_convex([(20.5 + a, 70.5 + b) for a, b in rx.FAN6], 96, 128).sum() + \
        rx._cover_convex([(60.5 + a, 70.5 + b) for a, b in rx.FAN8], 96, 128).sum()
    assert front.expect[70, 20] and front.expect[70, 60]          # the fans' hubs are pixel centres, drawn once
    for sc in rx.lattice_scenes():
        moved = sum(1 for t in sc.tris for u, v, _ in t if (u - 4.5) % 2 or (v - 4.5) % 2)
        assert moved > 0                                           # the jitter moves vertices off the regular lattice
        assert sc.expect.sum() == {"lattice-4x4-Z1": 40 * 32, "lattice-8x2-Z2": 48 * 24, "lattice-2x8-Z4": 24 * 48}[sc.name]


def test_path_cut_boxes_straddle_the_small_face_limit():
    full, want = rx.path_cut_scene(False)
    assert sorted(set(want.tolist())) == [127, 128, 129, 130]
    assert {(w, h) for w, h in rx.PATH_BOXES if 1 in (w, h)} >= {(1, 127), (127, 1), (1, 128), (128, 1), (1, 129), (129, 1)}
    clipped, kept = rx.path_cut_scene(True)
    assert kept.max() <= rx.SMALL_MAX and kept.min() >= 1 and (want > rx.SMALL_MAX).sum() > 0
    # the two calls see the same triangles: coverage of the clipped image is the window of the full one
    assert np.array_equal(clipped.covers(), full.covers()[:, :rx.PATH_CLIP, :rx.PATH_CLIP])
    cov = full.covers()
    t = ro.setup(ro.camera_vertices(full.verts.reshape(-1, 3)), np.arange(3 * len(full.tris)).reshape(-1, 3), full.K, full.H, full.W)
    assert len(t["idx"]) == len(full.tris)
    first, last = cov[np.arange(len(cov)), t["y0"], t["x0"]], cov[np.arange(len(cov)), t["y1"], t["x1"]]
    for n in (128, 129):                                            # some box of each size has its first, some its last pixel drawn
        assert first[want == n].any() and last[want == n].any()


def test_long_list_scene_walks_the_list_more_than_twice():
    verts, faces, K, Rt = rx.long_list_scene()                     # asserts >= 2 * 1024 + 1 large boxes in both views
    assert verts.shape == (1, 41 * 31, 3) and faces.shape == (2400, 3)
    t = ro.setup(ro.camera_vertices(verts[0], Rt[0, 1, :, :3], Rt[0, 1, :, 3]), faces, K, rx.LONG_H, rx.LONG_W)
    n = (t["x1"] - t["x0"] + 1) * (t["y1"] - t["y0"] + 1)
    assert (n <= rx.SMALL_MAX).sum() == 60 and len(n) == 2340      # the shifted view also has faces for the one-thread path


def test_tie_scenes_hold_ties():
    v, f, K, H, W = rx.tie_scene_twins()
    tied = rx.tied_pixels(v, f, K, H, W)
    assert tied.sum() == 32 * 24 and np.array_equal(tied, ro.raster(ro.camera_vertices(v[0]), f, K, H, W) != ro.KEY_NONE)
    v, f, K, H, W = rx.tie_scene_doubled()
    keys = ro.raster(ro.camera_vertices(v[0]), f, K, H, W)
    assert (keys != ro.KEY_NONE).sum() == 32 * 24 and ((keys[keys != ro.KEY_NONE] & np.uint64(0xFFFFFFFF)) < len(f) // 2).all()
    v, f, K, H, W = rx.tie_scene_crossing()
    tied = rx.tied_pixels(v, f, K, H, W)
    exp = np.zeros((H, W), bool)
    exp[8:40, rx.TIE_COL] = True                                   # a full column of equal depth bits, and no other pixel
    assert np.array_equal(tied, exp)
    for order in ((0, 1), (1, 0)):                                 # the lower person index takes the column, whichever quad that is
        keys = np.full((H, W), ro.KEY_NONE, np.uint64)
        for p, q in enumerate(order):
            ro.raster(ro.camera_vertices(v[q]), f, K, H, W, id_base=p * len(f), keys=keys)
        col = keys[8:40, rx.TIE_COL]
        assert ((col >> np.uint64(32)) == np.float32(2.0).view(np.uint32)).all() and ((col & np.uint64(0xFFFFFFFF)) < len(f)).all()


def test_nonfinite_person_draws_nothing_in_the_oracle():
    verts, broken, behind, faces, K, H, W = rx.nonfinite_scene()
    with np.errstate(all="ignore"):
        assert (ro.raster(ro.camera_vertices(broken), faces, K, H, W, cull=False) == ro.KEY_NONE).all()
    assert (ro.raster(ro.camera_vertices(behind), faces, K, H, W, cull=False) == ro.KEY_NONE).all()
    alone = [ro.raster(ro.camera_vertices(verts[p]), faces, K, H, W) != ro.KEY_NONE for p in range(3)]
    assert all(a.sum() == 900 for a in alone) and (alone[0] & alone[1] & alone[2]).any()


def test_rounded_shared_edges_are_drawn_once_by_the_oracle():
    """The one rounding scene: at these centres a face-by-face evaluation of the shared edge would draw twice or not at all
    (asserted where the scene is built); the oracle's fixed endpoint order draws every one of them once."""
    seams = rx.rounded_seam_scene()
    cov = rx.oracle_keys(seams) != ro.KEY_NONE
    count = cov[0::2].astype(np.int64) + cov[1::2]
    assert len(seams.centres) == 12 and count.max() == 1
    assert [int(count[i][c]) for i, c in enumerate(seams.centres)] == [1] * 12
