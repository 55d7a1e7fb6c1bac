"""Time multi_hmr_amd.render.render_batch (csrc/render.hip) with hipEvents on two scenes:
  (a) B = 32 images of 896^2, 160 meshes the size of SMPL-X (icospheres of subdivision 5: 10242 vertices, 20480 faces, radius 0.5 m)
      at 2-15 m, five per image;
  (b) B = 1 image of 896^2, 3 such meshes.
Prints one JSON line per scene: median / min milliseconds per call over --iters calls, covered pixels, and the share of the 129 ms
headline forward step (bench.py, B = 32 at 896^2) the overlay of a whole batch would add.
  python tools/render_bench.py [--iters 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multi_hmr_amd import render  # noqa: E402
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--scene", choices=["a", "b", "both"], default="both")
    a = ap.parse_args()
    if a.scene in ("a", "both"):
        run("a", 32, 5, a.iters)
    if a.scene in ("b", "both"):
        run("b", 1, 3, a.iters)
