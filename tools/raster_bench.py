"""Time the differentiable rasteriser (multi_hmr_amd/raster.py, csrc/raster_grad.hip), forward + backward, against the torch route a user
has without it, on the same GPU, the same scene and the same keys: B images of 896 x 896 with meshes the size of SMPL-X (icospheres of
subdivision 5, V = 10242, F = 20480, radius 0.5 m, at 2 - 15 m, as tools/maps_bench.py): B = 1 with 2 meshes, B = 32 with 160.
  kernel   rasterize(verts, ..., keys=keys[, attributes=]) and autograd.grad of sum(depth g_depth [+ attributes g_attr]) to the vertices
           [and the attributes]: mhmr_render_maps (person / face / mask), mhmr_raster_interpolate, mhmr_raster_backward.
  torch    render_maps(keys=keys, amodal=False) for person / face, gather the three corners of every drawn pixel, project, form the edge
           functions, the perspective-correct weights, depth [and attributes] in fp32 torch, scatter into the maps; the same autograd.grad.
Both start from the keys of one render (not timed).  The two forms alternate inside each repetition; a time is a pair of device events
around the form on the current stream.  Prints one JSON line per size and channel count with median / best / worst in milliseconds and
the largest difference between the two routes' results; no gate: a loss is printed as a loss.
  python tools/raster_bench.py [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multi_hmr_amd import _lib, maps, rasterize  # noqa: E402
import render_oracle  # noqa: E402  (the icosphere generator)

DEV = "cuda:0"
S = 896


def make_scene(B, per_image, seed=0):
    g = np.random.default_rng(seed)
    v, faces = render_oracle.icosphere(5)
    focal = S / (2 * np.tan(np.radians(60) / 2))
    K = torch.tensor([[focal, 0, S / 2], [0, focal, S / 2], [0, 0, 1]], dtype=torch.float32).repeat(B, 1, 1).to(DEV)
    P = B * per_image
    z = g.uniform(2, 15, P)
    xy = g.uniform(-0.45, 0.45, (P, 2)) * S / focal * z[:, None]
    offs = np.concatenate([xy, z[:, None]], 1).astype(np.float32)
    verts = torch.from_numpy(v[None] * np.float32(0.5) + offs[:, None]).to(DEV)
    idx = torch.arange(P, dtype=torch.int32) // per_image
    return verts, idx, K, faces, torch.from_numpy(v).to(DEV)


def torch_route(verts, attr, idx, K, faces_t, keys):
    """depth [B, S, S] and attributes [B, S, S, C] (or None) in fp32 torch from the person / face maps."""
    m = maps.render_maps(verts, idx, K, faces_t, (S, S), keys=keys, amodal=False)
    b, r, c = torch.nonzero(m.person >= 0, as_tuple=True)
    p, f = m.person[b, r, c].long(), m.face[b, r, c].long()
    corners = faces_t[f]                                                # [n, 3]
    X = verts[p[:, None], corners]                                      # [n, 3, 3]
    Kb = K[b]
    sx = Kb[:, 0, 0, None] * X[..., 0] / X[..., 2] + Kb[:, 0, 2, None]
    sy = Kb[:, 1, 1, None] * X[..., 1] / X[..., 2] + Kb[:, 1, 2, None]
    A = (sx[:, 1] - sx[:, 0]) * (sy[:, 2] - sy[:, 0]) - (sy[:, 1] - sy[:, 0]) * (sx[:, 2] - sx[:, 0])
    px, py = c.float() + 0.5, r.float() + 0.5
    w = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        e = (sx[:, k] - sx[:, j]) * (py - sy[:, j]) - (sy[:, k] - sy[:, j]) * (px - sx[:, j])
        w.append(e / A / X[:, i, 2])
    w = torch.stack(w, 1)
    Z = 1.0 / w.sum(1)
    depth = torch.zeros(m.person.shape, device=DEV).index_put((b, r, c), Z)
    out = None
    if attr is not None:
        a = attr[corners]                                               # the shared table [V, C]
        out = torch.zeros(m.person.shape + (attr.shape[-1],), device=DEV).index_put((b, r, c), ((w * Z[:, None])[..., None] * a).sum(1))
    return depth, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    print(json.dumps({"library": _lib.built_source_hash(), "device": torch.cuda.get_device_name(0)}))
    for B, per_image, channels in ((1, 2, (0, 3)), (32, 5, (0, 3))):
        verts0, idx, K, faces, template = make_scene(B, per_image)
        faces_t = torch.from_numpy(faces.astype(np.int64)).to(DEV)
        keys = rasterize(verts0, idx, K, faces, (S, S), want=("depth",)).keys
        g = torch.Generator(device=DEV).manual_seed(1)
        g_depth = torch.randn((B, S, S), device=DEV, generator=g)
        for C_ in channels:
            g_attr = torch.randn((B, S, S, C_), device=DEV, generator=g) if C_ else None

            def kernel():
                v = verts0.clone().requires_grad_(True)
                a = template.clone().requires_grad_(True) if C_ else None
                r = rasterize(v, idx, K, faces, (S, S), attributes=a, keys=keys, want=("depth", "attributes") if C_ else ("depth",))
                loss = (r.depth * g_depth).sum() + ((r.attributes * g_attr).sum() if C_ else 0.0)
                return r, torch.autograd.grad(loss, [v] + ([a] if C_ else []))

            def plain():
                v = verts0.clone().requires_grad_(True)
                a = template.clone().requires_grad_(True) if C_ else None
                depth, out = torch_route(v, a, idx, K, faces_t, keys)
                loss = (depth * g_depth).sum() + ((out * g_attr).sum() if C_ else 0.0)
                return depth, torch.autograd.grad(loss, [v] + ([a] if C_ else []))

            forms = {"kernel": kernel, "torch": plain}
            times = {n: [] for n in forms}
            last = {}
            for rep in range(args.warmup + args.reps):
                for n, fn in forms.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    last[n] = fn()
                    t1.record()
                    t1.synchronize()
                    if rep >= args.warmup:
                        times[n].append(t0.elapsed_time(t1))
            stat = lambda t: {"median_ms": round(float(np.median(t)), 4), "best_ms": round(min(t), 4), "worst_ms": round(max(t), 4)}
            r, gk = last["kernel"]
            depth_t, gt = last["torch"]
            rel = lambda x, y: float(((x - y).abs().max() / y.abs().max().clamp_min(1e-30)).detach())
            line = {"B": B, "P": B * per_image, "C": C_, "H": S, "W": S, "V": int(verts0.shape[1]), "F": int(len(faces)),
                    "pixels_drawn": int(r.mask.sum()), "kernel": stat(times["kernel"]), "torch": stat(times["torch"]),
                    "torch_median_over_kernel_median": round(float(np.median(times["torch"]) / np.median(times["kernel"])), 3),
                    "torch_best_over_kernel_worst": round(min(times["torch"]) / max(times["kernel"]), 3),
                    "depth_maxdiff_over_max": rel(depth_t, r.depth.detach()), "g_verts_maxdiff_over_max": rel(gt[0], gk[0])}
            if C_:
                line["g_attr_maxdiff_over_max"] = rel(gt[1], gk[1])
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
