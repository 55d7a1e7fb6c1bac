"""-m gpu: the mesh-overlay rasteriser (csrc/render.hip through multi_hmr_amd.render) against the numpy restatement of the render
contract (tests/render_oracle.py), its invariants, the batched scale scene and the end-to-end overlay of a forward's output."""
import os

import numpy as np
import pytest
import torch

import render_oracle as ro
from multi_hmr_amd import render

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _K(f, W, H, cx=None, cy=None):
    return np.array([[f, 0, W / 2 if cx is None else cx], [0, f, H / 2 if cy is None else cy], [0, 0, 1]], np.float32)


def _images(B, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3)).astype(np.uint8)


def _device(images, verts, image_index, K, faces, colors, alpha=0.8, Rt=None, smooth=True, cull=True):
    out, key, rgb = render.render_batch(torch.from_numpy(images).to(DEV), torch.from_numpy(np.asarray(verts, np.float32)).to(DEV),
                                        torch.as_tensor(np.asarray(image_index)), torch.from_numpy(np.asarray(K, np.float32)),
                                        faces, colors=colors, alpha=alpha, Rt=None if Rt is None else torch.from_numpy(Rt),
                                        smooth=smooth, cull_back=cull, return_debug=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), key.cpu().numpy().view(np.uint64), rgb.cpu().numpy()


def _edge_dist(X, face, K, x, y):
    """Smallest distance (pixels) from the pixel centre to the edges of the face's screen triangle."""
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    P = X[face]
    s = np.stack([(fx * P[:, 0]) / P[:, 2] + cx, (fy * P[:, 1]) / P[:, 2] + cy], 1)
    p = np.array([x + 0.5, y + 0.5])
    best = np.inf
    for i in range(3):
        a, b = s[i], s[(i + 1) % 3]
        d = b - a
        t = np.clip(np.dot(p - a, d) / max(np.dot(d, d), 1e-300), 0, 1)
        best = min(best, float(np.linalg.norm(a + t * d - p)))
    return best


def check_against_oracle(images, verts, image_index, K, faces, colors, alpha=0.8, Rt=None, smooth=True, cull=True, only=None):
    """Section 1 of the acceptance: winning keys equal except on <= 0.1 % of covered pixels, each within 1e-3 px of an edge of one of
    the two faces involved (or a depth tie to 1e-6 relative, where two surfaces cross); rgb within 1 LSB where the keys agree; the
    blend bit-exact against the oracle's fp32 blend fed the device's own keys and rgb.  only: images to compare (default all)."""
    out, key, rgb = _device(images, verts, image_index, K, faces, colors, alpha, Rt, smooth, cull)
    F = len(faces)
    sel = range(len(images)) if only is None else only
    for b in sel:
        ps = [p for p in range(len(verts)) if int(image_index[p]) == b]
        R, t = (None, None) if Rt is None else (Rt[b][:, :3], Rt[b][:, 3])
        Xs, Ns = {}, {}
        okeys = np.full(images.shape[1:3], KEY_NONE, np.uint64)
        for p in ps:
            Xs[p] = ro.camera_vertices(verts[p], R, t)
            Ns[p] = ro._rotate(R, ro.vertex_normals(verts[p], faces)) if smooth else None
            ro.raster(Xs[p], faces, K[b], *images.shape[1:3], id_base=p * F, keys=okeys, cull=cull)
        dk = key[b]
        bad = np.argwhere(dk != okeys)
        covered = int((okeys != KEY_NONE).sum())
        print(f"FORGIVEN image {b}: {len(bad)} of {covered} covered pixels differ from the oracle "
              f"({images.shape[1]}x{images.shape[2]}, P={len(ps)}, F={F})")
        assert len(bad) <= max(0.001 * covered, 0), (b, len(bad), covered)
        for y, x in bad:
            ok = False
            ids = [int(k & np.uint64(0xFFFFFFFF)) for k in (dk[y, x], okeys[y, x]) if k != KEY_NONE]
            for i in ids:
                ok |= _edge_dist(Xs[i // F], np.asarray(faces)[i % F], K[b], x, y) <= 1e-3
            if len(ids) == 2:
                z = [float(np.uint32(k >> np.uint64(32)).view(np.float32)) for k in (dk[y, x], okeys[y, x])]
                ok |= abs(z[0] - z[1]) <= 1e-6 * z[1]
            assert ok, (b, y, x, dk[y, x], okeys[y, x])
        same = (dk == okeys) & (dk != KEY_NONE)
        orgb = ro.shade_keys(dk, {**{p: Xs[p] for p in ps}}, Ns, faces, K[b], colors, smooth=smooth, cull=cull)
        diff = np.abs(rgb[b].astype(np.int64) - orgb.astype(np.int64))
        assert diff[same].max(initial=0) <= 1, (b, diff[same].max())
        assert (rgb[b][dk == KEY_NONE] == 0).all()
        exp = ro.blend(images[b], rgb[b], ro.mask(dk != KEY_NONE), alpha)
        assert np.array_equal(out[b], exp), (b, int((out[b] != exp).sum()))
        assert covered > 0 or only is not None
    return out, key, rgb


def _sphere(subdiv, centre, radius):
    v, f = ro.icosphere(subdiv)
    return (v * radius + np.asarray(centre, np.float32)).astype(np.float32), f


def test_scenes_match_the_oracle():
    H, W = 96, 128
    K = _K(110.0, W, H)[None]
    img = _images(1, H, W)
    cols = np.array([[0.8, 0.3, 0.2], [0.2, 0.6, 0.9]], np.float32)
    # two icospheres overlapping in depth
    a, f = _sphere(3, (0.0, 0.0, 3.0), 0.6)
    b, _ = _sphere(3, (0.3, 0.1, 3.4), 0.6)
    check_against_oracle(img, np.stack([a, b]), [0, 0], K, f, cols)
    check_against_oracle(img, np.stack([a, b]), [0, 0], K, f, cols, smooth=False, cull=False)
    # a cube across the image border (and larger than the image)
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32) * 0.5 + np.array([0.9, -0.3, 2.5], np.float32)
    cf = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                   [1, 5, 7], [1, 7, 3]], np.int32)
    check_against_oracle(img, c[None], [0], K, cf, cols[:1])
    check_against_oracle(img, c[None], [0], K, cf, cols[:1], cull=False)
    # a strip partly nearer than znear, partly beyond zfar (faces dropped by znear, fragments rejected by zfar)
    zs = np.geomspace(0.02, 300.0, 40)
    strip = np.array([[s, 0.3, zz] for zz in zs for s in (-6.0, 6.0)], np.float32)        # a floor receding from the lens
    sf = np.array([[2 * i, 2 * i + 2, 2 * i + 1] for i in range(39)] + [[2 * i + 1, 2 * i + 2, 2 * i + 3] for i in range(39)], np.int32)
    check_against_oracle(img, strip[None], [0], _K(110.0, W, H, 64.0, 48.3)[None], sf, cols[:1], cull=False)   # row 48: Z = 165
    # degenerate faces and duplicated vertices
    d, df = _sphere(2, (-0.2, 0.2, 2.0), 0.5)
    d = np.concatenate([d, d[:20]])                                           # vertices 162.. duplicate 0..19
    extra = np.array([[0, 0, 5], [3, 7, 3], [1, 162, 1], [0, 162, 5]], np.int32)   # zero area (index or position repeated)
    swap = df.copy()
    swap[df < 20] += 162                                                      # half the faces use the duplicates
    swap[::2] = df[::2]
    check_against_oracle(img, d[None], [0], K, np.concatenate([swap, extra]), cols[:1])
    # one triangle larger than the image
    big = np.array([[-50, -50, 4.0], [50, -50, 4.0], [0, 60, 4.0]], np.float32)
    check_against_oracle(img, big[None], [0], K, np.array([[0, 2, 1]], np.int32), cols[:1])
    # non-square 517 x 300 with R, t
    H2, W2 = 300, 517
    th = 0.3
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]], np.float32)
    Rt = np.concatenate([R, np.array([[0.1], [-0.2], [0.5]], np.float32)], 1)[None]
    e, ef = _sphere(3, (0.2, 0.0, 2.5), 0.7)
    g, _ = _sphere(3, (-0.6, 0.3, 3.5), 0.7)
    check_against_oracle(_images(1, H2, W2, 3), np.stack([e, g]), [0, 0], _K(300.0, W2, H2, 250.3, 140.7)[None], ef, cols, Rt=Rt)


def test_invariants():
    H, W = 80, 100
    imgs = _images(4, H, W, 5)
    K = np.stack([_K(90.0 + 5 * i, W, H) for i in range(4)])
    vs, f = zip(*[_sphere(2, ((-1) ** i * 0.3, 0.1 * i, 2.0 + 0.5 * i), 0.5) for i in range(6)])
    verts = np.stack(vs)
    f = f[0]
    idx = np.array([0, 1, 1, 2, 3, 3])
    cols = np.array(render.PALETTE[:6], np.float32)
    out, key, rgb = _device(imgs, verts, idx, K, f, cols)
    # P = 0 and alpha = 0 leave the images unchanged
    o0, k0, _ = _device(imgs, verts[:0], idx[:0], K, f, cols[:0])
    assert np.array_equal(o0, imgs) and (k0 == KEY_NONE).all()
    oa, ka, _ = _device(imgs, verts, idx, K, f, cols, alpha=0.0)
    assert np.array_equal(oa, imgs) and np.array_equal(ka, key)
    # the four images of one call equal each image alone
    for b in range(4):
        ps = np.nonzero(idx == b)[0]
        ob, kb, rb = _device(imgs[b:b + 1], verts[ps], np.zeros(len(ps), int), K[b:b + 1], f, cols[ps])
        assert np.array_equal(ob[0], out[b]) and np.array_equal(rb[0], rgb[b])
        ids = np.where(kb[0] == KEY_NONE, KEY_NONE, (kb[0] & np.uint64(0xFFFFFFFF)) % np.uint64(len(f)))
        ids_all = np.where(key[b] == KEY_NONE, KEY_NONE, (key[b] & np.uint64(0xFFFFFFFF)) % np.uint64(len(f)))
        assert np.array_equal(ids, ids_all)
    # two runs are equal
    out2, key2, rgb2 = _device(imgs, verts, idx, K, f, cols)
    assert np.array_equal(out, out2) and np.array_equal(key, key2) and np.array_equal(rgb, rgb2)
    # permuting the persons of a tie-free scene (disjoint depth ranges per image) changes no pixel
    perm = np.array([5, 3, 1, 0, 4, 2])
    op, kp, rp = _device(imgs, verts[perm], idx[perm], K, f, cols[perm])
    assert np.array_equal(op, out) and np.array_equal(rp, rgb)


def scale_scene(B=32, S=896, per=5, seed=0):
    """B images of S^2, per icospheres (subdivision 5: 10242 vertices, 20480 faces, radius 0.5 m) per image at 2-15 m."""
    rng = np.random.default_rng(seed)
    v, f = ro.icosphere(5)
    focal = S / (2 * np.tan(np.radians(60) / 2))
    K = np.stack([_K(focal, S, S) for _ in range(B)])
    verts, idx = [], []
    for b in range(B):
        for _ in range(per):
            z = rng.uniform(2, 15)
            xy = rng.uniform(-0.45, 0.45, 2) * S / focal * z
            verts.append(v * 0.5 + np.array([xy[0], xy[1], z], np.float32))
            idx.append(b)
    return _images(B, S, S, seed), np.stack(verts).astype(np.float32), np.array(idx), K, f


def test_scale_scene_batch_equals_single_images_and_oracle():
    imgs, verts, idx, K, f = scale_scene()
    cols = np.array([render.PALETTE[i % 10] for i in range(len(verts))], np.float32)
    out, key, rgb = check_against_oracle(imgs, verts, idx, K, f, cols, only=(0, 13, 31))
    for b in range(len(imgs)):
        ps = np.nonzero(idx == b)[0]
        ob, _, rb = _device(imgs[b:b + 1], verts[ps], np.zeros(len(ps), int), K[b:b + 1], f, cols[ps])
        assert np.array_equal(ob[0], out[b]) and np.array_equal(rb[0], rgb[b]), b


def test_forward_then_render_batch_equals_render_meshes_and_overlay(smplx_data, mean_params, tmp_path, monkeypatch):
    import argparse
    from PIL import Image
    import synthetic
    from multi_hmr_amd import Model, demo
    S, name = 448, "dinov2_vits14"
    sd = synthetic.make_state_dict(name, S, seed=7, depth_override=2, mean_params=mean_params)
    model = Model(backbone=name, img_size=S, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=2, precision="f16")
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    x = torch.randn(2, 3, S, S, generator=torch.Generator().manual_seed(3)).to(DEV)
    K = synthetic.get_camera_K(S, 2).to(DEV)
    o, ids = model(x, K=K, det_thresh=1e-6, nms_kernel_size=3, return_batched=True)
    P = o["v3d"].shape[0]
    assert P > 0
    faces = model.smpl_layer["neutral_10"].bm_x.faces
    imgs = torch.from_numpy(_images(2, S, S, 9)).to(DEV)
    out = render.render_batch(imgs, o["v3d"], ids, K, faces, alpha=0.8)
    host = [o["v3d"][p].cpu().numpy() for p in range(P)]
    idc = ids.cpu().numpy()
    for b in range(2):
        ps = [p for p in range(P) if idc[p] == b]
        kb = K[b].cpu().numpy()
        ref = render.render_meshes(imgs[b].cpu().numpy(), [host[p] for p in ps], [faces] * len(ps),
                                   {"focal": kb[[0, 1], [0, 1]], "princpt": kb[[0, 1], [2, 2]]},
                                   color=[render.PALETTE[p % len(render.PALETTE)] for p in ps], alpha=0.8)
        assert np.array_equal(ref, out[b].cpu().numpy()), b
    # overlay_human_meshes: the reference's tuple, persons read in place from the forward's block
    humans = model(x[:1], K=K[:1], det_thresh=0.05, nms_kernel_size=3)
    pil = Image.fromarray(_images(1, S, S, 4)[0])
    arr, cols = demo.overlay_human_meshes(humans, faces, K[:1], model, pil, alpha=0.8)
    assert isinstance(arr, np.ndarray) and arr.dtype == np.uint8 and arr.shape == (S, S, 3) and isinstance(cols, list)
    if len(humans) > 1:
        st = demo._stacked([h["v3d"] for h in humans])
        assert st.data_ptr() == humans[0]["v3d"].data_ptr()
    assert len(humans) == 0 or not np.array_equal(arr, np.asarray(pil))
    # the command line on a checkpoint in the reference's format: [input | overlay], width 2 W
    os.makedirs(tmp_path / "models" / "multiHMR")
    os.makedirs(tmp_path / "models" / "smplx")
    os.makedirs(tmp_path / "imgs")
    np.savez(tmp_path / "models" / "smplx" / "SMPLX_NEUTRAL.npz", **smplx_data)
    np.savez(tmp_path / "models" / "smpl_mean_params.npz", **mean_params)
    args = argparse.Namespace(backbone=name, img_size=[S, S], train_return_type="smpl", num_betas=10, nearness=True, xat_depth=2,
                              xat_num_heads=8, backbone_depth=2)
    torch.save({"args": args, "model_state_dict": sd}, tmp_path / "models" / "multiHMR" / "synth.pt")
    Image.fromarray(_images(1, 300, 517, 11)[0]).save(tmp_path / "imgs" / "a.png")
    monkeypatch.chdir(tmp_path)
    written = demo.main(["--img_folder", "imgs", "--out_folder", "out", "--model_name", "synth", "--det_thresh", "0.05"])
    assert len(written) == 1 and Image.open(written[0]).size == (2 * 517, 300)
