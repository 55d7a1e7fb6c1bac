"""-m gpu: the rasteriser (csrc/render.hip) on the exact scenes of tests/render_exact.py.  Every screen coordinate of these scenes
is dyadic, so every edge function is an exact fp64 number and no pixel is forgiven: the device keys (coverage, id and depth bits)
equal the numpy oracle's on every pixel, and the device coverage equals `exact_cover`, which is integer arithmetic written from the
header's wording.  The scenes aim at what the kernel has dedicated code for: the endpoint order of `edge_fn` and the top-left flags
(shared edges through pixel centres, lattices, fans), the 128-pixel cut between the one-thread and the workgroup path, a large-face
list longer than twice the workgroup grid, the key's tie order, the clip planes, images smaller than a resolve tile, a person with
non-finite vertices, and the raw-descriptor rules of include/mhmr.h.  One scene rounds on purpose (rounded-seams, Z = 3): with dyadic
coordinates either endpoint order of an edge gives the same exact value, so only there does `edge_fn`'s ordering show.  Every comparison prints its count of differing pixels first
(pytest -s, lines starting with EXACT)."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_exact as rx
import render_oracle as ro
from multi_hmr_amd import _lib, render

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
LOW32 = np.uint64(0xFFFFFFFF)
ALPHA = 0.8


def _same(tag, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = got != want
    print(f"EXACT {tag}: {int(bad.sum())} of {bad.size} differ")
    assert not bad.any(), (tag, np.argwhere(bad)[:8].tolist())


def _cols(P):
    return np.array([render.PALETTE[i % len(render.PALETTE)] for i in range(P)], np.float32)


def _images(B, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3)).astype(np.uint8)


def _device(images, verts, idx, K, faces, cols, smooth=True, cull=True, Rt=None):
    out, key, rgb = render.render_batch(torch.from_numpy(images).to(DEV), torch.from_numpy(np.asarray(verts, np.float32)).to(DEV),
                                        torch.as_tensor(np.asarray(idx)), torch.from_numpy(np.asarray(K, np.float32)), faces, colors=cols,
                                        alpha=ALPHA, Rt=None if Rt is None else torch.from_numpy(Rt), smooth=smooth, cull_back=cull,
                                        return_debug=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), key.cpu().numpy().view(np.uint64), rgb.cpu().numpy()


def _ids(key):
    """The id field of the keys, -1 where nothing is drawn."""
    return np.where(key == KEY_NONE, -1, (key & LOW32).astype(np.int64))


def _draw_scene(scene):
    imgs, verts, idx, K, faces = rx.one_face_per_image(scene)
    return _device(imgs, verts, idx, K, faces, _cols(len(verts)), cull=scene.cull)


COUNT_SCENES = rx.shared_edge_scenes() + rx.lattice_scenes()


@pytest.mark.parametrize("scene", COUNT_SCENES, ids=repr)
def test_shared_edges_and_lattices_cover_every_centre_once(scene):
    """Scenes 1 and 2, one face per image: keys equal the oracle's, coverage equals exact_cover, and the count over the images is 1 on
    every centre of the region (top and left edges in, bottom and right edges out) and 0 elsewhere."""
    _, key, _ = _draw_scene(scene)
    _same(f"{scene} keys", key, rx.oracle_keys(scene))
    _same(f"{scene} coverage", key != KEY_NONE, scene.covers())
    _same(f"{scene} count", (key != KEY_NONE).sum(0), scene.expect.astype(np.int64))


def test_path_cut_small_and_workgroup_paths_give_the_same_fragments():
    """Scene 3: boxes of 127, 128, 129 and 130 pixels.  The 12 x 12 call cuts every box to at most 8 x 8 pixels with the same camera,
    so faces the workgroup pass draws in the 136 x 136 call are drawn by their own thread there: the keys of the common window are
    equal bit for bit."""
    full, want = rx.path_cut_scene(False)
    clipped, kept = rx.path_cut_scene(True)
    assert (want > rx.SMALL_MAX).sum() >= 32 and (want <= rx.SMALL_MAX).sum() >= 32 and kept.max() <= rx.SMALL_MAX
    _, kf, _ = _draw_scene(full)
    _, kc, _ = _draw_scene(clipped)
    _same("path-cut keys", kf, rx.oracle_keys(full))
    _same("path-cut coverage", kf != KEY_NONE, full.covers())
    _same("path-cut-clipped keys", kc, rx.oracle_keys(clipped))
    _same("path-cut-clipped coverage", kc != KEY_NONE, clipped.covers())
    _same("path-cut window", kc, kf[:, :rx.PATH_CLIP, :rx.PATH_CLIP])
    assert (kc != KEY_NONE).any(axis=(1, 2)).sum() >= len(kc) // 2    # the window is not an empty corner of the boxes


def test_long_large_face_list_in_two_views():
    """Scene 4: 2400 faces with 169-pixel boxes, so every workgroup of the 1024 walks the list a third time; through render_views with a
    second view shifted by 39 whole pixels, which also sends 60 border-cut faces down the one-thread path."""
    verts, faces, K, Rt = rx.long_list_scene()
    H, W = rx.LONG_H, rx.LONG_W
    imgs, cols = _images(1, H, W, 4), _cols(1)
    args = (torch.from_numpy(imgs).to(DEV), torch.from_numpy(verts).to(DEV), torch.zeros(1, dtype=torch.int32), torch.from_numpy(K[None]), faces)
    first = render.render_views(*args, torch.from_numpy(Rt), colors=cols, alpha=ALPHA, return_debug=True)
    second = render.render_views(*args, torch.from_numpy(Rt), colors=cols, alpha=ALPHA, return_debug=True)
    torch.cuda.synchronize()
    out, key, rgb = (t.cpu().numpy() for t in first)
    key = key.view(np.uint64)
    for v in range(2):
        okeys = ro.raster(ro.camera_vertices(verts[0], Rt[0, v, :, :3], Rt[0, v, :, 3]), faces, K, H, W)
        _same(f"long-list view {v} keys", key[0, v], okeys)
        region = rx._rect(H, W, 8.5 + rx.LONG_SHIFT * v, 8.5, 488.5 + rx.LONG_SHIFT * v, 368.5)
        _same(f"long-list view {v} coverage", key[0, v] != KEY_NONE, region)
    assert len(np.unique(_ids(key[0, 0]))) == 2400 + 1             # every face of the list won pixels
    o1, k1, r1 = _device(imgs, verts, [0], K[None], faces, cols, Rt=np.ascontiguousarray(Rt[:, 1]))
    _same("long-list view 1 = one-view keys", key[0, 1], k1[0])
    _same("long-list view 1 = one-view rgb", rgb[0, 1], r1[0])
    _same("long-list view 1 = one-view out", out[0, 1], o1[0])
    for a, b, name in zip(first, second, ("out", "key", "rgb")):
        _same(f"long-list two calls {name}", a.cpu().numpy(), b.cpu().numpy())


def test_depth_ties_go_to_the_lower_id():
    """Scene 5: the id field of the key is p F + f, and equal depth bits leave the pixel to the lower one."""
    # (a) two persons with bit-identical vertices and different colours: person 0 owns every pixel, with its own colour
    verts, faces, K, H, W = rx.tie_scene_twins()
    F, imgs, cols = len(faces), _images(1, H, W, 5), np.array([[0.9, 0.2, 0.1], [0.1, 0.3, 0.9]], np.float32)
    assert rx.tied_pixels(verts, faces, K, H, W).sum() == 32 * 24
    _, okeys, orgb = ro.render(imgs, verts, [0, 0], K[None], faces, cols, alpha=ALPHA)
    for order in ((0, 1), (1, 0)):
        out, key, rgb = _device(imgs, verts, [0, 0], K[None], faces, cols[list(order)])
        alone = _device(imgs, verts[:1], [0], K[None], faces, cols[[order[0]]])
        _same(f"twins {order} keys", key, okeys)
        assert (_ids(key)[key != KEY_NONE] < F).all()
        _same(f"twins {order} rgb = person 0 alone", rgb, alone[2])
        _same(f"twins {order} out = person 0 alone", out, alone[0])
        again = _device(imgs, verts, [0, 0], K[None], faces, cols[list(order)])
        assert all(np.array_equal(x, y) for x, y in zip((out, key, rgb), again))
    assert np.abs(_device(imgs, verts, [0, 0], K[None], faces, cols)[2].astype(np.int64) - orgb.astype(np.int64)).max() <= 1
    # (b) one mesh with every face listed twice: the first copy owns every pixel
    verts, faces, K, H, W = rx.tie_scene_doubled()
    out, key, rgb = _device(_images(1, H, W, 6), verts, [0], K[None], faces, _cols(1))
    _same("doubled keys", key[0], ro.raster(ro.camera_vertices(verts[0]), faces, K, H, W))
    assert (key != KEY_NONE).sum() == 32 * 24 and (_ids(key)[key != KEY_NONE] < len(faces) // 2).all()
    # (c) a flat quad at Z = 2 against a tilted one that passes through Z = 2 along column 48
    verts, faces, K, H, W = rx.tie_scene_crossing()
    F, imgs = len(faces), _images(1, H, W, 7)
    tied = rx.tied_pixels(verts, faces, K, H, W)
    assert tied[8:40, rx.TIE_COL].all() and tied.sum() == 32            # the precondition: a full column of equal depth bits
    quad, res = {}, {}
    for order in ((0, 1), (1, 0)):
        o = list(order)
        _, okeys, orgb = ro.render(imgs, verts[o], [0, 0], K[None], faces, cols[o], alpha=ALPHA)
        out, key, rgb = res[order] = _device(imgs, verts[o], [0, 0], K[None], faces, cols[o])
        _same(f"crossing {order} keys", key, okeys)
        ids = _ids(key[0])
        assert (ids[tied] >= 0).all() and (ids[tied] < F).all()         # the lower p F + f, whichever quad person 0 is
        quad[order] = np.where(ids < 0, -1, np.asarray(order)[np.clip(ids, 0, None) // F])
        assert np.abs(rgb.astype(np.int64) - orgb.astype(np.int64)).max() <= 1
        alone = _device(imgs, verts[o[:1]], [0], K[None], faces, cols[o[:1]])
        _same(f"crossing {order} rgb on the tie = person 0 alone", rgb[0][tied], alone[2][0][tied])
        again = _device(imgs, verts[o], [0, 0], K[None], faces, cols[o])
        assert all(np.array_equal(x, y) for x, y in zip(res[order], again))
    _same("crossing: the swap changes the winner on the tied pixels only", quad[(0, 1)] != quad[(1, 0)], tied)
    _same("crossing: depth bits", res[(0, 1)][1] >> np.uint64(32), res[(1, 0)][1] >> np.uint64(32))
    _same("crossing: rgb off the tie", res[(0, 1)][2][0][~tied], res[(1, 0)][2][0][~tied])
    assert (res[(0, 1)][2][0][tied] != res[(1, 0)][2][0][tied]).any(axis=1).all()


def test_faces_on_the_clip_planes_keep_every_pixel():
    """Scene 6: znear and zfar are the descriptor's fp32 fields.  A face at exactly fl32(0.05) or 100.0 draws exactly exact_cover (its
    interpolated fp64 depth strays an ulp to either side of the plane; the fp32 depth of the key does not), the fp32 neighbours beyond
    draw nothing.  The oracle's ZNEAR is fl32(0.05) as well; the double 0.05 would decide the same for these fp32 depths."""
    scene = rx.clip_scene()
    _, key, _ = _draw_scene(scene)
    _same("clip keys", key, rx.oracle_keys(scene))
    cov = scene.covers()
    assert cov[0].sum() == 120
    _same("clip on znear", key[0] != KEY_NONE, cov[0])
    _same("clip on zfar", key[2] != KEY_NONE, cov[2])
    assert (key[1] == KEY_NONE).all() and (key[3] == KEY_NONE).all()
    assert (key[0][cov[0]] >> np.uint64(32) == rx.Z_NEAR32.view(np.uint32)).all() and (key[2][cov[2]] >> np.uint64(32) == rx.Z_FAR32.view(np.uint32)).all()


@pytest.mark.parametrize("H", rx.SMALL_H)
def test_small_images(H):
    """Scene 7: images of 1 .. 9 rows and 1 .. 129 columns, below, at and one past the resolve tile (64 x 4 with a one-pixel apron): wholly
    covered (the 3 x 3 mask on all four borders) and with a small triangle over one corner."""
    for scene in [s for s in rx.small_image_scenes() if s.H == H]:
        imgs, verts, idx, K, faces = rx.one_face_per_image(scene, seed=H + scene.W)
        cols = _cols(1)
        out, key, rgb = _device(imgs, verts, idx, K, faces, cols)
        _, okeys, orgb = ro.render(imgs, verts, idx, K, faces, cols, alpha=ALPHA)
        _same(f"{scene} keys", key, okeys)
        _same(f"{scene} coverage", key != KEY_NONE, scene.covers())
        _same(f"{scene} out", out[0], ro.blend(imgs[0], rgb[0], ro.mask(key[0] != KEY_NONE), ALPHA))
        assert np.abs(rgb.astype(np.int64) - orgb.astype(np.int64)).max() <= 1, scene
        assert (rgb[key == KEY_NONE] == 0).all()
        if scene.name.endswith("-full"):
            assert (key != KEY_NONE).all()


@pytest.mark.parametrize("smooth", [True, False])
def test_nonfinite_person_draws_nothing_and_harms_nobody(smooth):
    """Scene 8: the middle of three persons has NaN and +-Inf coordinates in every face.  The call returns, that person owns no pixel, and
    keys, rgb and out equal the call in which it stands wholly behind the camera instead."""
    verts, broken, behind, faces, K, H, W = rx.nonfinite_scene()
    F, imgs, cols = len(faces), _images(1, H, W, 8), _cols(3)
    bad = np.stack([verts[0], broken, verts[2]])
    ref = np.stack([verts[0], behind, verts[2]])
    out, key, rgb = _device(imgs, bad, [0, 0, 0], K[None], faces, cols, smooth=smooth)
    o2, k2, r2 = _device(imgs, ref, [0, 0, 0], K[None], faces, cols, smooth=smooth)
    _, okeys, orgb = ro.render(imgs, ref, [0, 0, 0], K[None], faces, cols, alpha=ALPHA, smooth=smooth)
    ids = _ids(key)
    assert not ((ids >= F) & (ids < 2 * F)).any()
    assert (ids >= 2 * F).any() and ((ids >= 0) & (ids < F)).any()
    _same(f"non-finite smooth={smooth} keys", key, okeys)
    _same(f"non-finite smooth={smooth} keys = behind the camera", key, k2)
    _same(f"non-finite smooth={smooth} rgb = behind the camera", rgb, r2)
    _same(f"non-finite smooth={smooth} out = behind the camera", out, o2)
    assert np.abs(rgb.astype(np.int64) - orgb.astype(np.int64)).max() <= 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the raw descriptor (include/mhmr.h mhmr_render_desc), filled the way render._render fills it
# ---------------------------------------------------------------------------------------------------------------------------------
GUARD = 4096


def _raw(imgs, vbuf, vstride, V, faces, idx, K, cols, smooth=0, csr=None, cull=1, want_key=True, want_rgb=True):
    """One mhmr_render_meshes call on a hand-filled descriptor.  vbuf: the flat fp32 vertex block, person p at p * vstride.  img_out,
    key_out and rgb_out lie between guard bytes.  Returns (out, key or None, rgb or None); asserts that the guards and the inputs are
    untouched."""
    B, H, W, _ = imgs.shape
    P, F = len(idx), len(faces)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)
    d_img, d_v, d_f, d_idx, d_K, d_c = t(imgs, np.uint8), t(vbuf, np.float32), t(faces, np.int32), t(idx, np.int32), t(K, np.float32), t(cols, np.float32)
    d_csr = [None, None] if csr is None else [t(a, np.int32) for a in csr]
    npx = B * H * W
    bufs = {n: torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV) for n, nbytes in (("out", 3 * npx), ("key", 8 * npx), ("rgb", 3 * npx))}
    d = _lib.RenderDesc()
    d.B, d.H, d.W, d.P, d.V, d.F = B, H, W, P, V, F
    d.verts, d.vstride = d_v.data_ptr(), vstride
    d.faces, d.adj_off, d.adj = d_f.data_ptr(), _lib.ptr(d_csr[0]), _lib.ptr(d_csr[1])
    d.image_index, d.K, d.colors, d.Rt = d_idx.data_ptr(), d_K.data_ptr(), d_c.data_ptr(), None
    d.alpha, d.intensity, d.ambient, d.metallic, d.roughness = ALPHA, 3.0, render.AMBIENT, 0.0, 0.5
    d.znear, d.zfar, d.smooth, d.cull_back = render.ZNEAR, render.ZFAR, smooth, cull
    d.img_in, d.img_out = d_img.data_ptr(), bufs["out"].data_ptr() + GUARD
    d.key_out = bufs["key"].data_ptr() + GUARD if want_key else None
    d.rgb_out = bufs["rgb"].data_ptr() + GUARD if want_rgb else None
    nbytes = _lib.workspace_bytes("mhmr_render_workspace_bytes", C.byref(d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    _lib.check(_lib.lib().mhmr_render_meshes(C.byref(d), torch.cuda.current_stream().cuda_stream), "mhmr_render_meshes")
    torch.cuda.synchronize()
    host = {n: b.cpu().numpy() for n, b in bufs.items()}
    for n, h in host.items():
        assert (h[:GUARD] == 0xA5).all() and (h[-GUARD:] == 0xA5).all(), f"bytes around {n} were written"
    if not want_key:
        assert (host["key"] == 0xA5).all()
    if not want_rgb:
        assert (host["rgb"] == 0xA5).all()
    assert np.array_equal(d_v.cpu().numpy(), np.ascontiguousarray(vbuf, np.float32), equal_nan=True) and np.array_equal(d_img.cpu().numpy(), imgs)
    out = host["out"][GUARD:-GUARD].reshape(B, H, W, 3)
    key = host["key"][GUARD:-GUARD].view(np.uint64).reshape(B, H, W) if want_key else None
    rgb = host["rgb"][GUARD:-GUARD].reshape(B, H, W, 3) if want_rgb else None
    return out, key, rgb


def _raw_scene():
    """Three persons of nonfinite_scene (all finite) and their faces."""
    verts, _, _, faces, K, H, W = rx.nonfinite_scene()
    return verts, faces, K, H, W


def test_raw_descriptor_skips_faces_with_an_index_outside_the_mesh():
    verts, faces, K, H, W = _raw_scene()
    P, V, F = verts.shape[0], verts.shape[1], len(faces)
    wild = faces.copy()
    wild[2, 0], wild[5, 1], wild[9, 2], wild[12, 0], wild[17, 2] = -1, V, -7, V + 100, V
    skipped = np.array([2, 5, 9, 12, 17])
    tame = wild.copy()
    tame[skipped] = 0                                               # a zero-area face for the oracle: the ids keep their meaning
    imgs, cols = _images(1, H, W, 9), _cols(P)
    out, key, rgb = _raw(imgs, verts.reshape(P, -1), 3 * V, V, wild, [0, 0, 0], K[None], cols, smooth=0, csr=None)
    eo, ek, er = ro.render(imgs, verts, [0, 0, 0], K[None], tame, cols, alpha=ALPHA, smooth=False)
    whole = _ids(ro.render(imgs, verts, [0, 0, 0], K[None], faces, cols, alpha=ALPHA, smooth=False)[1])
    assert all((whole[whole >= 0] % F == f).any() for f in skipped)    # with their real indices the five faces win pixels
    ids = _ids(key)
    assert not np.isin(ids[ids >= 0] % F, skipped).any() and (ids >= 0).any()
    _same("raw bad faces keys", key, ek)
    _same("raw bad faces out", out, ro.blend(imgs, rgb, np.stack([ro.mask(k != KEY_NONE) for k in key]), ALPHA))
    assert np.abs(rgb.astype(np.int64) - er.astype(np.int64)).max() <= 1


def _oracle_keys_of_valid_persons(verts, idx, K, faces, B, H, W):
    keys = np.full((B, H, W), KEY_NONE, np.uint64)
    for p, b in enumerate(idx):
        if 0 <= b < B:
            ro.raster(ro.camera_vertices(verts[p]), faces, K[b], H, W, id_base=p * len(faces), keys=keys[b])
    return keys


def test_persons_with_an_image_index_outside_the_batch_are_skipped():
    verts3, faces, K, H, W = _raw_scene()
    verts = np.concatenate([verts3, verts3[:1]])                    # four persons, two images
    idx, B, F, V = [0, -1, 2, 1], 2, len(faces), verts3.shape[1]
    imgs, cols, Ks = _images(B, H, W, 10), _cols(4), np.stack([K, K])
    ek = _oracle_keys_of_valid_persons(verts, idx, Ks, faces, B, H, W)
    assert (ek[0] != KEY_NONE).any() and (ek[1] != KEY_NONE).any()
    csr = render.build_csr(faces, V)
    for smooth in (0, 1):
        out, key, rgb = _raw(imgs, verts.reshape(4, -1), 3 * V, V, faces, idx, Ks, cols, smooth=smooth, csr=csr if smooth else None)
        _same(f"raw image_index smooth={smooth} keys", key, ek)
        assert set(np.unique(_ids(key)[key != KEY_NONE] // F)) == {0, 3}
        wo, wk, wr = _device(imgs, verts, idx, Ks, faces, cols, smooth=bool(smooth))      # the wrapper passes the indices through
        _same(f"wrapper image_index smooth={smooth} keys", wk, key)
        _same(f"wrapper image_index smooth={smooth} rgb", wr, rgb)
        _same(f"wrapper image_index smooth={smooth} out", wo, out)
        _same(f"image_index smooth={smooth} out", out, ro.blend(imgs, rgb, np.stack([ro.mask(k != KEY_NONE) for k in key]), ALPHA))


def test_raw_descriptor_wide_vertex_stride_and_optional_outputs():
    verts, faces, K, H, W = _raw_scene()
    P, V, F = verts.shape[0], verts.shape[1], len(faces)
    imgs, cols = _images(1, H, W, 11), _cols(P)
    csr = render.build_csr(faces, V)
    tight = _raw(imgs, verts.reshape(P, -1), 3 * V, V, faces, [0, 0, 0], K[None], cols, smooth=1, csr=csr)
    wide = np.full((P, 3 * V + 12), 1234.5, np.float32)             # four sentinel rows behind every person's vertices
    wide[:, :3 * V] = verts.reshape(P, -1)
    loose = _raw(imgs, wide, 3 * V + 12, V, faces, [0, 0, 0], K[None], cols, smooth=1, csr=csr)
    _, ek, er = ro.render(imgs, verts, [0, 0, 0], K[None], faces, cols, alpha=ALPHA)
    _same("raw vstride keys", loose[1], ek)
    for a, b, name in zip(loose, tight, ("out", "key", "rgb")):
        _same(f"raw vstride {name} = tight stride", a, b)
    assert np.abs(loose[2].astype(np.int64) - er.astype(np.int64)).max() <= 1
    no_key = _raw(imgs, wide, 3 * V + 12, V, faces, [0, 0, 0], K[None], cols, smooth=1, csr=csr, want_key=False)
    no_rgb = _raw(imgs, wide, 3 * V + 12, V, faces, [0, 0, 0], K[None], cols, smooth=1, csr=csr, want_rgb=False)
    assert no_key[1] is None and no_rgb[2] is None
    _same("raw key_out NULL out", no_key[0], loose[0])
    _same("raw key_out NULL rgb", no_key[2], loose[2])
    _same("raw rgb_out NULL out", no_rgb[0], loose[0])
    _same("raw rgb_out NULL key", no_rgb[1], loose[1])


def test_rounded_shared_edges_are_drawn_once():
    """The one scene here whose edge functions round (Z = 3): twelve shared edges through a pixel centre at which evaluating the edge from
    each face's own winding would draw the centre twice or not at all.  With edge_fn's fixed endpoint order the two faces get exactly
    opposite values, so every centre is drawn once; the keys still equal the oracle's, which rounds the same operations."""
    seams = rx.rounded_seam_scene()
    _, key, _ = _draw_scene(seams)
    cov = key != KEY_NONE
    count = cov[0::2].astype(np.int64) + cov[1::2]
    at = [int(count[i][c]) for i, c in enumerate(seams.centres)]
    print(f"EXACT rounded-seams: count at the twelve centres {at}, largest count {int(count.max())}")
    assert at == [1] * 12 and count.max() == 1
    _same("rounded-seams keys", key, rx.oracle_keys(seams))
