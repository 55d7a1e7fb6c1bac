"""Time multi_hmr_amd.render.render_batch (csrc/render.hip) with hipEvents on two scenes:
  (a) B = 32 images of 896^2, 160 meshes the size of SMPL-X (icospheres of subdivision 5: 10242 vertices, 20480 faces, radius 0.5 m)
      at 2-15 m, five per image;
  (b) B = 1 image of 896^2, 3 such meshes.
Prints one JSON line per scene: median / min milliseconds per call over --iters calls, covered pixels, and the share of the 129 ms
headline forward step (bench.py, B = 32 at 896^2) the overlay of a whole batch would add.
Scene (c) is the demo's rotating video: one 896^2 image with 10 such meshes seen from the 60 views of a 20-frame / 60 degree video
(demo.create_rotating_video), drawn by one render_views call and, as the only way before it, by render_batch on the 600 meshes
replicated view-major over 60 copies of the image with one Rt each.  It prints both forms' times and workspace bytes and checks that
their images are byte-identical.
  python tools/render_bench.py [--iters 20] [--scene a|b|c|both|all]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ctypes  # noqa: E402

from multi_hmr_amd import _lib, demo, render  # noqa: E402
import render_oracle  # noqa: E402  (the icosphere generator)

STEP_MS = 129.0


def scene(B, per, S=896, seed=0):
    rng = np.random.default_rng(seed)
    v, f = render_oracle.icosphere(5)
    focal = S / (2 * np.tan(np.radians(60) / 2))
    K = torch.tensor([[focal, 0, S / 2], [0, focal, S / 2], [0, 0, 1]], dtype=torch.float32).repeat(B, 1, 1)
    verts, idx = [], []
    for b in range(B):
        for _ in range(per):
            z = rng.uniform(2, 15)
            xy = rng.uniform(-0.45, 0.45, 2) * S / focal * z
            verts.append(v * 0.5 + np.array([xy[0], xy[1], z], np.float32))
            idx.append(b)
    imgs = torch.from_numpy(rng.integers(0, 256, (B, S, S, 3)).astype(np.uint8))
    return imgs, torch.from_numpy(np.stack(verts).astype(np.float32)), torch.tensor(idx, dtype=torch.int32), K, f


def run(name, B, per, iters):
    dev = torch.device("cuda:0")
    imgs, verts, idx, K, f = scene(B, per)
    imgs, verts, idx, K = imgs.to(dev), verts.to(dev), idx.to(dev), K.to(dev)
    for _ in range(3):
        out = render.render_batch(imgs, verts, idx, K, f, alpha=0.8)
    _, key, _ = render.render_batch(imgs, verts, idx, K, f, alpha=0.8, return_debug=True)
    covered = int((key != -1).sum())
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = render.render_batch(imgs, verts, idx, K, f, alpha=0.8)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    del out
    med = float(np.median(ms))
    print(json.dumps(dict(scene=name, B=B, meshes=B * per, faces=int(B * per * len(f)), ms_median=round(med, 4),
                          ms_min=round(float(min(ms)), 4), covered_pixels=covered, frac_of_step=round(med / STEP_MS, 5))), flush=True)


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4)


def _workspace_bytes(B, H, W, P, V, F, nviews=None):
    d = _lib.RenderDesc()
    d.B, d.H, d.W, d.P, d.V, d.F, d.vstride = B, H, W, P, V, F, 3 * V
    L = _lib.lib()
    return int(L.mhmr_render_workspace_bytes(ctypes.byref(d)) if nviews is None else
               L.mhmr_render_views_workspace_bytes(ctypes.byref(d), nviews))


def run_views(iters, n_frames=20, angle_range=60):
    dev = torch.device("cuda:0")
    imgs, verts, idx, K, f = scene(1, 10)
    P, V, S = verts.shape[0], verts.shape[1], imgs.shape[1]
    angles = [angle_range * i / (n_frames - 1) for i in range(n_frames)]
    c = verts[0].mean(0).numpy()
    Rt = np.concatenate([demo.orbit_extrinsics(c, "y", angles), demo.orbit_extrinsics(c, "y", [-a for a in angles]),
                         demo.orbit_extrinsics(c, "x", angles)]).astype(np.float32)
    NV = len(Rt)
    imgs, verts, K = imgs.to(dev), verts.to(dev), K.to(dev)
    idx = torch.zeros(P, dtype=torch.int32, device=dev)
    Rt_v = torch.from_numpy(Rt)[None].to(dev)
    # the replicated form: view v is image v, holding persons v P .. v P + P - 1 (view-major: the persons keep their order)
    imgs_r = imgs.expand(NV, S, S, 3).contiguous()
    verts_r = verts.repeat(NV, 1, 1)
    idx_r = torch.arange(NV, dtype=torch.int32, device=dev).repeat_interleave(P)
    K_r = K.expand(NV, 3, 3).contiguous()
    Rt_r = torch.from_numpy(Rt).to(dev)
    cols = [render.PALETTE[p % len(render.PALETTE)] for p in range(P)]
    views = lambda: render.render_views(imgs, verts, idx, K, f, Rt_v, colors=cols, alpha=0.8, return_debug=True)
    repl = lambda: render.render_batch(imgs_r, verts_r, idx_r, K_r, f, colors=cols * NV, alpha=0.8, Rt=Rt_r, return_debug=True)
    ov, kv, rv = views()
    orr, kr, rr = repl()
    identical = bool(torch.equal(ov[0], orr) and torch.equal(rv[0], rr) and torch.equal(kv[0] == -1, kr == -1))
    covered = int((kv != -1).sum())
    del ov, kv, rv, orr, kr, rr
    run_v = lambda: render.render_views(imgs, verts, idx, K, f, Rt_v, colors=cols, alpha=0.8)
    run_r = lambda: render.render_batch(imgs_r, verts_r, idx_r, K_r, f, colors=cols * NV, alpha=0.8, Rt=Rt_r)
    tv, tr = _time(run_v, iters), _time(run_r, iters)
    print(json.dumps(dict(scene="c", images=1, views=NV, meshes=P, faces_drawn=int(NV * P * len(f)), covered_pixels=covered,
                          views_ms_median=tv[0], views_ms_min=tv[1], views_workspace_bytes=_workspace_bytes(1, S, S, P, V, len(f), NV),
                          replicated_ms_median=tr[0], replicated_ms_min=tr[1],
                          replicated_workspace_bytes=_workspace_bytes(NV, S, S, NV * P, V, len(f)),
                          replicated_vertex_bytes=int(verts_r.numel() * 4), images_identical=identical)), flush=True)
    if not identical:
        raise SystemExit("scene (c): render_views and the replicated render_batch differ")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--scene", choices=["a", "b", "c", "both", "all"], default="all")
    a = ap.parse_args()
    if a.scene in ("a", "both", "all"):
        run("a", 32, 5, a.iters)
    if a.scene in ("b", "both", "all"):
        run("b", 1, 3, a.iters)
    if a.scene in ("c", "all"):
        run_views(a.iters)
