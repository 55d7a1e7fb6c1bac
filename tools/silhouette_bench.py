"""Time the silhouette term (multi_hmr_amd/silhouette.py, csrc/silhouette.hip), forward + backward, against what a user has without it,
on the same GPU and the same scene: B images of 896 x 896 with meshes the size of SMPL-X (icospheres of subdivision 5, V = 10242,
F = 20480, radius 0.5 m, at 2 - 15 m, as tools/raster_bench.py): B = 1 with 2 meshes, B = 32 with 160.  The masks are the visible
pixels of the same meshes moved sideways by 5 cm.
  kernel   silhouette_loss(verts, ..., masks) and autograd.grad of loss.sum() to the vertices: one mhmr_silhouette call.
  torch    the same two terms with today's tools: the capped distance map of every `allowed` map (scipy's
           distance_transform_edt on the host where scipy is importable, else a separable torch form: two cummax passes down the columns
           and a minimum over 2 R + 1 shifts along the rows), F.grid_sample of it at the projected vertices, and for the uncovered pixels
           (mask and not the person's visible pixels) a chunked torch.cdist against the projected vertices; the same autograd.grad.
           It is no oracle: fp32, the modal instead of the amodal cover, nearest vertex instead of nearest splat.
The two forms alternate inside each repetition; a time is a pair of device events around the form on the current stream.  Also timed
alone: distance_transform of the `allowed` maps and of the splat maps (the two transforms inside mhmr_silhouette), so the split between
the transforms and the rest can be read off.  One JSON line per size, printed and written to --out; no gate: a loss is printed as a loss.
  python tools/silhouette_bench.py [--reps 10] [--warmup 2] [--out profiles/silhouette_bench.txt]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multi_hmr_amd import _lib, distance_transform, maps, silhouette_loss  # noqa: E402
import render_oracle  # noqa: E402  (the icosphere generator)

try:
    from scipy import ndimage
except ImportError:
    ndimage = None

DEV = "cuda:0"
S = 896
SIGMA, R = 8.0, 64


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
    return verts, idx, K, faces


def visible(verts, idx, K, faces):
    """[P, S, S] bool: each person's visible pixels."""
    person = maps.render_maps(verts, idx, K, faces, (S, S), amodal=False).person.reshape(-1, S, S)
    return person[idx.long().to(DEV)] == torch.arange(len(verts), device=DEV).reshape(-1, 1, 1)


def others(masks, idx, B):
    union = torch.zeros((B, S, S), dtype=torch.int32, device=DEV).index_add_(0, idx.long().to(DEV), masks.to(torch.int32))
    return masks | ((union[idx.long().to(DEV)] - masks.to(torch.int32)) > 0)


def capped_distance(allowed):
    """phi [P, S, S] float32 = min(distance to the nearest on-pixel, sqrt(R R + 1))."""
    cap = float(np.sqrt(R * R + 1))
    if ndimage is not None:
        host = allowed.cpu().numpy()
        out = np.stack([ndimage.distance_transform_edt(~m) if m.any() else np.full(m.shape, cap) for m in host])
        return torch.from_numpy(np.minimum(out, cap).astype(np.float32)).to(DEV)
    rows = torch.arange(S, device=DEV, dtype=torch.int32).reshape(1, S, 1)
    far = 4 * S
    up = torch.cummax(torch.where(allowed, rows, -far), 1).values                              # the last on-row at or above
    down = -torch.cummax(torch.where(allowed, -rows, -far).flip(1), 1).values.flip(1)           # the first on-row at or below
    dy = torch.minimum(rows - up, down - rows).clamp(max=R + 1).float()
    g = F.pad(dy * dy, (R, R), value=float(R * R + 1))
    best = torch.full_like(dy, float(R * R + 1))
    for dx in range(-R, R + 1):
        best = torch.minimum(best, g[:, :, R + dx:R + dx + S] + float(dx * dx))
    return best.sqrt()


def torch_route(verts, idx, K, masks, allowed, cover):
    P, V = verts.shape[:2]
    Kp = K[idx.long().to(DEV)]
    u = Kp[:, 0, 0, None] * verts[..., 0] / verts[..., 2] + Kp[:, 0, 2, None]
    v = Kp[:, 1, 1, None] * verts[..., 1] / verts[..., 2] + Kp[:, 1, 2, None]
    inside = (u >= 0) & (u < S) & (v >= 0) & (v < S)
    phi = capped_distance(allowed)
    grid = torch.stack([(u - 0.5) / (S - 1) * 2 - 1, (v - 0.5) / (S - 1) * 2 - 1], -1).reshape(P, 1, V, 2)
    sample = F.grid_sample(phi[:, None], grid, mode="bilinear", padding_mode="border", align_corners=True).reshape(P, V)
    s = sample * sample / SIGMA ** 2
    outside = torch.where(inside, s / (1 + s), torch.zeros_like(s)).sum(1)
    uncovered = []
    todo = masks & ~cover
    for p in range(P):
        ys, xs = torch.nonzero(todo[p], as_tuple=True)
        pts = torch.stack([xs.float() + 0.5, ys.float() + 0.5], 1)
        pi = torch.stack([u[p], v[p]], 1)[inside[p]]
        total = verts.new_zeros(())
        if len(pts) and len(pi):
            for chunk in pts.split(8192):
                d = torch.cdist(chunk, pi)
                m = d.min(1).values
                total = total + torch.where(m <= R, m * m, torch.zeros_like(m)).sum() / SIGMA ** 2
        uncovered.append(total)
    return outside + torch.stack(uncovered)


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    out = fn()
    t1.record()
    t1.synchronize()
    return out, t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "silhouette_bench.txt"))
    args = ap.parse_args()
    lines = [{"library": _lib.built_source_hash(), "device": torch.cuda.get_device_name(0),
              "host_distance_maps": "scipy.ndimage.distance_transform_edt" if ndimage is not None else "separable torch (no scipy)"}]
    print(json.dumps(lines[0]), flush=True)
    for B, per_image in ((1, 2), (32, 5)):
        verts0, idx, K, faces = make_scene(B, per_image)
        moved = verts0 + torch.tensor([0.05, 0.0, 0.0], device=DEV)
        masks = visible(moved, idx, K, faces)
        allowed = others(masks, idx, B)
        cover = visible(verts0, idx, K, faces)
        reps = args.reps if B == 1 else max(2, args.reps // 3)

        def kernel():
            v = verts0.clone().requires_grad_(True)
            s = silhouette_loss(v, idx, K, faces, masks, sigma=SIGMA, max_dist=R)
            return s, torch.autograd.grad(s.loss.sum(), v)[0]

        def plain():
            v = verts0.clone().requires_grad_(True)
            loss = torch_route(v, idx, K, masks, allowed, cover)
            return loss, torch.autograd.grad(loss.sum(), v)[0]

        Kp = K[idx.long().to(DEV)]
        c = (Kp[:, 0, 0, None] * verts0[..., 0] / verts0[..., 2] + Kp[:, 0, 2, None]).floor().long()
        r = (Kp[:, 1, 1, None] * verts0[..., 1] / verts0[..., 2] + Kp[:, 1, 2, None]).floor().long()
        ok = (c >= 0) & (c < S) & (r >= 0) & (r < S)
        splats = torch.zeros_like(masks).reshape(len(verts0), -1)
        splats.scatter_(1, torch.where(ok, r * S + c, torch.zeros_like(c)), ok)
        splats = splats.reshape(masks.shape)
        forms = {"kernel": kernel, "torch": plain, "transform_allowed": lambda: distance_transform(allowed, R),
                 "transform_splats": lambda: distance_transform(splats, R)}
        times = {n: [] for n in forms}
        last = {}
        for rep in range(args.warmup + reps):
            for n, fn in forms.items():
                last[n], ms = timed(fn)
                if rep >= args.warmup:
                    times[n].append(ms)
        stat = lambda t: {"median_ms": round(float(np.median(t)), 4), "best_ms": round(min(t), 4), "worst_ms": round(max(t), 4)}
        s, gk = last["kernel"]
        lt, gt = last["torch"]
        med = {n: float(np.median(t)) for n, t in times.items()}
        line = {"B": B, "P": B * per_image, "H": S, "W": S, "V": int(verts0.shape[1]), "F": int(len(faces)), "sigma": SIGMA, "max_dist": R,
                "reps": reps, "outside_vertices": int(s.outside_vertices.sum()), "uncovered_px": int(s.uncovered_px.sum()),
                **{n: stat(t) for n, t in times.items()},
                "torch_median_over_kernel_median": round(med["torch"] / med["kernel"], 3),
                "torch_best_over_kernel_worst": round(min(times["torch"]) / max(times["kernel"]), 3),
                "transforms_share_of_kernel": round((med["transform_allowed"] + med["transform_splats"]) / med["kernel"], 3),
                "loss_kernel": float(s.loss.sum().detach()), "loss_torch": float(lt.sum().detach()),
                "g_verts_maxdiff_over_max": float(((gt - gk).abs().max() / gk.abs().max().clamp_min(1e-30)))}
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(line) + "\n" for line in lines))


if __name__ == "__main__":
    main()
