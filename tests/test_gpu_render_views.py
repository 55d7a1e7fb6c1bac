"""-m gpu: the multi-view render (mhmr_render_views through multi_hmr_amd.render.render_views): every view equals a one-view
render_batch call with that view's extrinsics byte for byte, a few views pass the numpy oracle of the render contract, the one-view
case equals mhmr_render_meshes, two calls are equal, and the demo's --extra_views / --save_rotating_video run end to end."""
import os

import numpy as np
import pytest
import torch

import render_oracle as ro
from multi_hmr_amd import demo, render
from test_gpu_render import check_against_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _K(f, W, H):
    return np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)


def scene(B, H=60, W=84, seed=0):
    """B images, two icospheres (subdivision 2) per image at 2.5-4 m, and one triangle whose box is far larger than the 128-pixel
    small-face limit in image 0; all meshes share one face array (the triangle's mesh repeats its first face)."""
    rng = np.random.default_rng(seed)
    v, f = ro.icosphere(2)
    verts, idx = [], []
    for b in range(B):
        for k in range(2):
            c = np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.3, 0.3), rng.uniform(2.5, 4.0)])
            verts.append(v * rng.uniform(0.3, 0.6) + c)
            idx.append(b)
    tri = np.repeat(np.array([[-0.9, -0.7, 3.2]]), len(v), 0)
    tri[f[0, 1]] = [0.9, -0.5, 3.6]
    tri[f[0, 2]] = [0.1, 0.8, 3.0]
    verts.append(tri)
    idx.append(0)
    imgs = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    K = np.stack([_K(70.0 + 4 * b, W, H) for b in range(B)])
    cols = np.array([render.PALETTE[i % len(render.PALETTE)] for i in range(len(verts))], np.float32)
    return imgs, np.stack(verts).astype(np.float32), np.array(idx), K, f, cols


def views(B, NV, seed=1):
    """[B, NV, 3, 4]: turns about (0, 0, 3) of up to +-100 degrees about y or x, plus views that push the meshes off screen, put
    them behind znear (partly or wholly) and the identity."""
    rng = np.random.default_rng(seed)
    Rt = np.zeros((B, NV, 3, 4))
    for b in range(B):
        for v in range(NV):
            kind = (v + b) % 6
            if kind == 0 and v == 0:
                Rt[b, v] = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
                continue
            axis = "xy"[rng.integers(0, 2)]
            Rt[b, v] = demo.orbit_extrinsics([0.0, 0.0, 3.0], axis, [rng.uniform(-100, 100)])[0]
            if kind == 3:
                Rt[b, v, 0, 3] += rng.choice([-8.0, 8.0])                 # off screen
            elif kind == 4:
                Rt[b, v, 2, 3] -= rng.uniform(2.6, 3.4)                   # across znear: some faces dropped
            elif kind == 5:
                Rt[b, v, 2, 3] -= 8.0                                     # behind the camera
    return Rt.astype(np.float32)


def _views(imgs, verts, idx, K, f, cols, Rt, **kw):
    out, key, rgb = render.render_views(torch.from_numpy(imgs).to(DEV), torch.from_numpy(verts).to(DEV), torch.as_tensor(idx),
                                        torch.from_numpy(K), f, torch.from_numpy(Rt), colors=cols, return_debug=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), key.cpu().numpy(), rgb.cpu().numpy()


def _batch(imgs, verts, idx, K, f, cols, Rt, **kw):
    out, key, rgb = render.render_batch(torch.from_numpy(imgs).to(DEV), torch.from_numpy(verts).to(DEV), torch.as_tensor(idx),
                                        torch.from_numpy(K), f, colors=cols, Rt=None if Rt is None else torch.from_numpy(Rt),
                                        return_debug=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), key.cpu().numpy(), rgb.cpu().numpy()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("NV", [1, 7, 60])
def test_every_view_equals_a_one_view_call(B, NV):
    imgs, verts, idx, K, f, cols = scene(B)
    Rt = views(B, NV)
    for smooth, cull in ((True, True), (False, False), (True, False)):
        out, key, rgb = _views(imgs, verts, idx, K, f, cols, Rt, smooth=smooth, cull_back=cull)
        assert out.shape == (B, NV) + imgs.shape[1:] and key.shape == (B, NV) + imgs.shape[1:3] and rgb.shape == out.shape
        drawn = empty = 0
        for v in range(NV):
            ob, kb, rb = _batch(imgs, verts, idx, K, f, cols, np.ascontiguousarray(Rt[:, v]), smooth=smooth, cull_back=cull)
            assert np.array_equal(out[:, v], ob) and np.array_equal(key[:, v], kb) and np.array_equal(rgb[:, v], rb), (smooth, cull, v)
            drawn += sum(int((kb[b] != -1).any()) for b in range(B))
            empty += sum(int((kb[b] == -1).all()) for b in range(B))
        assert drawn > 0 and (NV < 7 or empty > 0)                    # some views draw, and some draw nothing
        # the large triangle (its box ~37 x 34 pixels) goes through the workgroup pass and wins pixels of the identity view
        ids = (key[0, 0][key[0, 0] != -1] & 0xFFFFFFFF) // len(f)
        assert (ids == 2 * B).sum() > 0


def test_views_match_the_oracle():
    imgs, verts, idx, K, f, cols = scene(2, H=72, W=96, seed=3)
    Rt = views(2, 6, seed=4)
    out, key, rgb = _views(imgs, verts, idx, K, f, cols, Rt)
    checked = 0
    for v in (0, 1, 2, 4):
        o, k, r = check_against_oracle(imgs, verts, idx, K, f, cols, Rt=np.ascontiguousarray(Rt[:, v]), only=(0, 1))
        assert np.array_equal(out[:, v], o) and np.array_equal(key[:, v].view(np.uint64), k) and np.array_equal(rgb[:, v], r), v
        checked += int((k != np.uint64(0xFFFFFFFFFFFFFFFF)).any())
    assert checked >= 3


def test_one_view_equals_render_meshes():
    """mhmr_render_views with nviews = 1 against mhmr_render_meshes, with extrinsics and with NULL (identity) in both."""
    imgs, verts, idx, K, f, cols = scene(3, seed=5)
    Rt = views(3, 1, seed=6)
    dimg, dverts = torch.from_numpy(imgs).to(DEV), torch.from_numpy(verts).to(DEV)
    for R1, Rv in ((torch.from_numpy(Rt[:, 0].copy()), torch.from_numpy(Rt)), (None, None)):
        for smooth in (True, False):
            args = (dimg, dverts, torch.as_tensor(idx), torch.from_numpy(K), f, cols, 0.8)
            tail = (smooth, True, True, 3.0, 0.0, 0.5)
            a = render._render(*args, R1, None, *tail)
            b = render._render(*args, Rv, 1, *tail)
            assert a[0].shape == b[0][:, 0].shape
            for x, y in zip(a, b):
                assert torch.equal(x, y[:, 0])
    # identity extrinsics given explicitly equal NULL in every view
    eye = torch.zeros(3, 4, 3, 4)
    eye[..., :3] = torch.eye(3)
    a = render._render(dimg, dverts, torch.as_tensor(idx), torch.from_numpy(K), f, cols, 0.8, None, 4, True, True, True, 3.0, 0.0, 0.5)
    b = render.render_views(dimg, dverts, torch.as_tensor(idx), torch.from_numpy(K), f, eye, colors=cols, return_debug=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.equal(a[k][:, 0], a[k][:, 3]) for k in range(3))


def test_two_calls_are_equal():
    imgs, verts, idx, K, f, cols = scene(3, seed=7)
    Rt = views(3, 9, seed=8)
    first = _views(imgs, verts, idx, K, f, cols, Rt)
    second = _views(imgs, verts, idx, K, f, cols, Rt)
    assert all(np.array_equal(x, y) for x, y in zip(first, second))


def _apng_timeline(path):
    from PIL import Image
    png = Image.open(path)
    frames = []
    for k in range(png.n_frames):
        png.seek(k)
        frames += [np.asarray(png.convert("RGB"))] * int(round(png.info["duration"] / 100))
    return frames


def test_demo_extra_view_and_rotating_video(smplx_data, mean_params, tmp_path, monkeypatch):
    """demo.main with the reference's --extra_views 1 --save_rotating_video 1 on a checkpoint in the reference's format.  The forward
    is kept to its first two persons (random weights at a low threshold detect hundreds), or to none."""
    import argparse
    from PIL import Image
    import synthetic
    S, name = 448, "dinov2_vits14"
    sd = synthetic.make_state_dict(name, S, seed=7, depth_override=2, mean_params=mean_params)
    os.makedirs(tmp_path / "models" / "multiHMR")
    os.makedirs(tmp_path / "models" / "smplx")
    os.makedirs(tmp_path / "imgs")
    np.savez(tmp_path / "models" / "smplx" / "SMPLX_NEUTRAL.npz", **smplx_data)
    np.savez(tmp_path / "models" / "smpl_mean_params.npz", **mean_params)
    args = argparse.Namespace(backbone=name, img_size=[S, S], train_return_type="smpl", num_betas=10, nearness=True, xat_depth=2,
                              xat_num_heads=8, backbone_depth=2)
    torch.save({"args": args, "model_state_dict": sd}, tmp_path / "models" / "multiHMR" / "synth.pt")
    H, W = 300, 517
    Image.fromarray(np.random.default_rng(11).integers(0, 256, (H, W, 3)).astype(np.uint8)).save(tmp_path / "imgs" / "a.png")
    monkeypatch.chdir(tmp_path)

    keep = {"n": 2}
    real_forward, real_views = demo.forward_model, render.render_views
    calls = []

    def forward(*a, **k):
        return real_forward(*a, **k)[:keep["n"]]

    def spy(*a, **k):
        out = real_views(*a, **k)
        calls.append((torch.as_tensor(a[5]).clone(), out.cpu().numpy()))
        return out

    monkeypatch.setattr(demo, "forward_model", forward)
    monkeypatch.setattr(render, "render_views", spy)
    argv = ["--img_folder", "imgs", "--out_folder", "out", "--model_name", "synth", "--det_thresh", "1e-6", "--alpha", "0.8",
            "--extra_views", "1", "--save_rotating_video", "1"]
    written = demo.main(argv)
    assert written == [os.path.join("out", "a.png_synth.png"), os.path.join("out", "a.png_synth_rotating.png")]
    panels = np.asarray(Image.open(written[0]).convert("RGB"))
    assert panels.shape == (H, 3 * W, 3)
    photo, overlay, side = panels[:, :W], panels[:, W:2 * W], panels[:, 2 * W:]
    assert np.array_equal(photo, np.asarray(Image.open(tmp_path / "imgs" / "a.png").convert("RGB")))
    assert not np.array_equal(overlay, photo)
    # the extra view: view 1 of a 2-frame / 30 degree call, the persons turned +30 degrees about y over white
    assert len(calls) == 2 and calls[0][1].shape == (1, 6, H, W, 3) and calls[1][1].shape == (1, 60, H, W, 3)
    assert np.array_equal(side, calls[0][1][0, 1]) and (side != 255).any()
    c = calls[0][0][0, 1].double().numpy()
    assert np.allclose(c[:, :3], demo.orbit_extrinsics(np.zeros(3), "y", [30.0])[0][:, :3], atol=1e-7)
    # the rotating video: 134 frames of the photograph's size; 0 = the overlay, 5 = 0 degrees, 24 = +60 degrees about y
    frames = _apng_timeline(written[1])
    assert len(frames) == 134 and all(fr.shape == (H, W, 3) for fr in frames)
    assert np.array_equal(frames[0], overlay) and np.array_equal(frames[4], overlay)
    assert np.array_equal(frames[5], calls[1][1][0, 0]) and np.array_equal(frames[24], calls[1][1][0, 19])
    assert np.array_equal(frames[25], calls[1][1][0, 18]) and not np.array_equal(frames[5], frames[24])
    # nobody detected: a white third panel and no video
    keep["n"] = 0
    written = demo.main(argv[:3] + ["out0"] + argv[4:])
    assert written == [os.path.join("out0", "a.png_synth.png")]
    panels = np.asarray(Image.open(written[0]).convert("RGB"))
    assert panels.shape == (H, 3 * W, 3) and (panels[:, 2 * W:] == 255).all()
    assert np.array_equal(panels[:, W:2 * W], panels[:, :W]) and not os.path.exists(tmp_path / "out0" / "a.png_synth_rotating.png")
