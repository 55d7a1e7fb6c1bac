"""-m "not gpu": the multi-view render entry points (mhmr_render_views, include/mhmr.h) are declared and exported and refuse bad input
before any launch, their workspace grows with the view count, and the demo's rotating video (demo.create_rotating_video) turns the
persons as the reference does and orders its frames as the reference does (renderer calls replaced by a fake that paints each view)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from multi_hmr_amd import _lib, demo, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("mhmr_render_views_workspace_bytes", "mhmr_render_views")


def test_view_entries_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    for sym in SYMS:
        assert sym in declared and sym in _lib.EXPORTS, sym


def _desc(**kw):
    d = _lib.RenderDesc()
    d.B, d.H, d.W, d.P, d.V, d.F, d.vstride = 2, 48, 64, 3, 100, 196, 300
    d.znear, d.zfar, d.smooth, d.cull_back = 0.05, 100.0, 1, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _fake_pointers():
    """Non-NULL addresses that are never dereferenced: every call below is refused before anything is launched."""
    ptrs = {k: 256 for k in ("verts", "faces", "adj_off", "adj", "image_index", "K", "colors", "img_in", "workspace")}
    return {**ptrs, "img_out": 512}


def test_views_refuse_bad_input_before_launch():
    _lib.build()
    L = _lib.lib()
    good = L.mhmr_render_views_workspace_bytes(C.byref(_desc()), 4)
    assert good > 0
    # the one-view workspace is the one mhmr_render_meshes asks for
    assert L.mhmr_render_views_workspace_bytes(C.byref(_desc()), 1) == L.mhmr_render_workspace_bytes(C.byref(_desc()))
    ptrs = _fake_pointers()
    for nv, bad, rc in ((0, {}, -2), (-3, {}, -2), (32768, {}, -2), (2, dict(B=40000), -2), (1, dict(B=65536), -2),
                        (70000, dict(B=1), -2), (2, dict(P=70000, F=35000), -2), (4, dict(Rt=256), -1)):
        assert L.mhmr_render_views_workspace_bytes(C.byref(_desc(**bad)), nv) == rc, (nv, bad)
        assert L.mhmr_render_views(C.byref(_desc(**{**ptrs, **bad})), nv, None, None) == rc, (nv, bad)
    # the limits themselves are accepted: B NV = 65535, one view of the largest B
    assert L.mhmr_render_views_workspace_bytes(C.byref(_desc(B=5, H=4, W=4)), 13107) > 0
    assert L.mhmr_render_views_workspace_bytes(C.byref(_desc(B=65535, H=4, W=4)), 1) > 0
    # a workspace one byte short, null images, img_out aliasing img_in with more than one view
    assert L.mhmr_render_views(C.byref(_desc(**{**ptrs, "workspace_bytes": good - 1})), 4, None, None) == -2
    assert L.mhmr_render_views(C.byref(_desc(**{**ptrs, "img_in": None, "workspace_bytes": good})), 4, None, None) == -1
    assert L.mhmr_render_views(C.byref(_desc(**{**ptrs, "img_out": 256, "workspace_bytes": good})), 4, None, None) == -1
    assert L.mhmr_render_views(None, 4, None, None) == -1
    assert L.mhmr_render_views_workspace_bytes(None, 4) == -1


def test_workspace_grows_with_views_by_at_least_the_keys():
    _lib.build()
    L = _lib.lib()
    keys = 2 * 48 * 64 * 8
    ws = [L.mhmr_render_views_workspace_bytes(C.byref(_desc()), nv) for nv in (1, 2, 3, 7, 60)]
    for (n0, w0), (n1, w1) in zip(zip((1, 2, 3, 7, 60), ws), zip((2, 3, 7, 60), ws[1:])):
        assert w1 - w0 >= (n1 - n0) * keys, (n0, n1, w0, w1)
    # per view: the camera vertices (fp64) and normals (fp32), keys; once: the fp64 world normals
    assert ws[-1] >= 60 * (3 * 100 * 24 + 3 * 100 * 12 + keys) + 3 * 100 * 24


@pytest.mark.parametrize("axis", ["x", "y"])
def test_orbit_extrinsics_equal_the_reference_rotation(axis):
    g = np.random.default_rng(0)
    x = g.normal(size=(50, 3)) * 0.4 + np.array([0.1, -0.2, 4.0])
    c = x.mean(0)
    angles = [-60.0, -30.0, -1e-3, 0.0, 12.5, 30.0, 60.0]
    Rt = demo.orbit_extrinsics(c, axis, angles)
    assert Rt.dtype == np.float64 and Rt.shape == (len(angles), 3, 4)
    for a, rt in zip(angles, Rt):
        th = np.deg2rad(a)
        if axis == "y":       # reference demo.py:165-176, verbatim
            rotmat = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
        else:
            rotmat = np.array([[1, 0, 0], [0, np.cos(th), -np.sin(th)], [0, np.sin(th), np.cos(th)]])
        ref = (x - c) @ rotmat.T + c
        mine = x @ rt[:, :3].T + rt[:, 3]
        assert np.allclose(mine, ref, rtol=0, atol=1e-13), (a, np.abs(mine - ref).max())
    assert np.array_equal(demo.orbit_extrinsics(c, axis, [0.0])[0], np.concatenate([np.eye(3), np.zeros((3, 1))], 1))
    with pytest.raises(ValueError):
        demo.orbit_extrinsics(c, "z", [10.0])


def _expected_sequence(n, rng):
    """The reference's frame order (demo.py:193-225) as labels: 'central' or (axis, angle)."""
    sweep = lambda axis, r: [(axis, r * i / (n - 1)) for i in range(n)]
    out = ["central"] * (n // 4)
    for s in (sweep("y", rng), sweep("y", -rng), sweep("x", rng)):
        out += s + s[::-1][1:-1] + ["central"] * (n // 4)
    return out


class _FakeRenderer:
    """render_batch paints 'central' (0, 0, 255); render_views paints view v as (v % 256, v // 256, 7) and records its Rt."""

    def __init__(self):
        self.views_calls, self.batch_calls = [], 0

    def batch(self, images, verts, image_index, K, faces, colors=None, alpha=0.8, **kw):
        self.batch_calls += 1
        assert (images != 255).any()                                    # over the photograph
        out = images.clone()
        out[..., 0], out[..., 1], out[..., 2] = 0, 0, 255
        return out

    def views(self, images, verts, image_index, K, faces, Rt, colors=None, alpha=0.8, **kw):
        assert (images == 255).all()                                    # over white
        Rt = torch.as_tensor(Rt)
        self.views_calls.append(Rt.clone())
        B, NV = Rt.shape[:2]
        out = torch.empty((B, NV) + tuple(images.shape[1:]), dtype=torch.uint8)
        for v in range(NV):
            out[:, v, ..., 0], out[:, v, ..., 1], out[:, v, ..., 2] = v % 256, v // 256, 7
        return out


@pytest.mark.parametrize("n,rng,total", [(20, 60, 134), (2, 30, 6)])
def test_rotating_video_frame_sequence(n, rng, total, monkeypatch, tmp_path):
    fake = _FakeRenderer()
    monkeypatch.setattr(render, "render_batch", fake.batch)
    monkeypatch.setattr(render, "render_views", fake.views)
    monkeypatch.setattr(demo, "_stacked", torch.stack)                # keep the persons on the host: nothing is drawn here
    g = np.random.default_rng(1)
    humans = [{"v3d": torch.from_numpy(g.normal(size=(30, 3)).astype(np.float32) + np.float32([0.0, 0.0, 3.0 + k]))} for k in range(3)]
    H, W = 12, 17
    photo = Image.fromarray(g.integers(0, 200, (H, W, 3)).astype(np.uint8))
    K = torch.tensor([[[20.0, 0, W / 2], [0, 20.0, H / 2], [0, 0, 1]]])
    fn = str(tmp_path / "clip_rotating.mp4")
    frames = demo.create_rotating_video(humans, np.zeros((4, 3), np.int32), K, None, photo, fn=fn, n_frames=n, angle_range=rng)
    exp = _expected_sequence(n, rng)
    assert len(frames) == len(exp) == total
    assert fake.batch_calls == 1 and len(fake.views_calls) == 1       # one overlay, every rotated frame in one render_views call
    Rt = fake.views_calls[0].double().numpy()
    assert Rt.shape == (1, 3 * n, 3, 4)
    c = humans[0]["v3d"].numpy().mean(0)
    for i, (f, e) in enumerate(zip(frames, exp)):
        assert f.shape == (H, W, 3) and f.dtype == np.uint8
        if e == "central":
            assert (f == np.array([0, 0, 255], np.uint8)).all(), i
            continue
        assert (f[..., 2] == 7).all() and (f[..., :2] == f[0, 0, :2]).all(), i
        v = int(f[0, 0, 0]) + 256 * int(f[0, 0, 1])
        want = demo.orbit_extrinsics(c, e[0], [e[1]])[0]
        assert np.allclose(Rt[0, v], want, rtol=0, atol=1e-6), (i, e, v)
    # the animated PNG: the same frames at 100 ms each (Pillow merges equal neighbours into one longer frame)
    png = Image.open(str(tmp_path / "clip_rotating.png"))
    timeline = []
    for k in range(png.n_frames):
        png.seek(k)
        timeline += [np.asarray(png.convert("RGB"))] * int(round(png.info["duration"] / 100))
    assert len(timeline) == total and all(np.array_equal(a, b) for a, b in zip(timeline, frames))
    assert not os.path.exists(fn)
    # nobody: None, no file, no render call
    assert demo.create_rotating_video([], None, K, None, photo, fn=str(tmp_path / "none.mp4")) is None
    assert not os.path.exists(tmp_path / "none.png") and fake.batch_calls == 1


def test_render_views_checks_rt_shape():
    img = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    for bad in (torch.zeros(1, 3, 4), torch.zeros(1, 0, 3, 4), torch.zeros(1, 2, 4, 4)):
        with pytest.raises(ValueError):
            render.render_views(img, torch.zeros(0, 3, 3), [], torch.eye(3)[None], np.zeros((1, 3), np.int32), bad)
