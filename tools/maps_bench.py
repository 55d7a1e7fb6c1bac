"""Time the per-pixel maps (multi_hmr_amd/maps.py, csrc/render_maps.hip) against the torch expressions on the key tensor that a user
writes without them, on the same GPU and the same scene: B images of 896 x 896 with 5 meshes the size of SMPL-X each (icospheres of
subdivision 5, V = 10242, F = 20480, radius 0.5 m, at 2 - 15 m: the scenes of tools/render_bench.py; B = 32: 160 meshes, and B = 1).
  maps        render_maps(keys=..., amodal=False): person / face / depth maps + visible_px / bbox / zmin (mhmr_render_maps, two launches)
              against torch: person = where(none, -1, low // F), depth = (key >> 32) reinterpreted, visible_px = bincount(person).
              The torch route has no bbox, zmin or face map; the kernel's time includes them.
  labels      the same with face_labels (L = 14): + label map and label_px, against torch's + label = labels[face] and a second bincount.
  points      render_maps(keys=..., points=v3d, amodal=False) minus `maps`: mhmr_render_point_visibility on every vertex, against the
              fp32 torch form (project, gather the depth at the pixel, compare).  The torch form rounds differently and is no oracle.
  amodal      render_maps(keys=..., amodal=True) minus `maps`: mhmr_render_amodal, against one render_batch per person (what the
              definition says; the only route of today), timed with --slow-reps repetitions.
  render      render_batch(return_debug=True) of the whole scene, for scale: what producing the keys costs.
The forms of a part are timed alternately (--reps after --warmup); a time is a host clock around the call ending in a device
synchronise.  Prints one JSON line per part and size with median / best / worst in milliseconds; there is no gate: a loss is printed
as a loss.
  python tools/maps_bench.py [--reps 20] [--warmup 3] [--slow-reps 2] [--batches 32 1]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multi_hmr_amd import maps, render  # noqa: E402
import render_oracle  # noqa: E402  (the icosphere generator)

DEV = "cuda:0"
S, PER_IMAGE = 896, 5


def make_scene(B, seed=0):
    """Scenes (a) and (b) of tools/render_bench.py: 5 meshes the size of SMPL-X per image (icospheres of subdivision 5: 10242 vertices,
    20480 faces, radius 0.5 m) at 2 - 15 m; 14 labels in contiguous face ranges."""
    g = np.random.default_rng(seed)
    v, faces = render_oracle.icosphere(5)
    focal = S / (2 * np.tan(np.radians(60) / 2))
    K = torch.tensor([[focal, 0, S / 2], [0, focal, S / 2], [0, 0, 1]], dtype=torch.float32).repeat(B, 1, 1).to(DEV)
    P = B * PER_IMAGE
    z = g.uniform(2, 15, P)
    xy = g.uniform(-0.45, 0.45, (P, 2)) * S / focal * z[:, None]
    offs = np.concatenate([xy, z[:, None]], 1).astype(np.float32)
    verts = torch.from_numpy(v[None] * np.float32(0.5) + offs[:, None]).to(DEV)
    idx = torch.arange(P, dtype=torch.int32) // PER_IMAGE
    labels = (np.arange(len(faces)) * 14 // len(faces)).astype(np.uint8)
    return verts, idx, K, faces, labels


def timed(forms, reps, warmup):
    """forms: {name: callable}; alternates them.  -> {name: [seconds]}"""
    out = {n: [] for n in forms}
    for r in range(warmup + reps):
        for n, f in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if r >= warmup:
                out[n].append(time.perf_counter() - t0)
    return out


def stat(ts):
    ts = sorted(ts)
    return {"median_ms": round(1e3 * ts[len(ts) // 2], 4), "best_ms": round(1e3 * ts[0], 4), "worst_ms": round(1e3 * ts[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slow-reps", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 1])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "maps_bench needs the GPU"
    for B in a.batches:
        verts, idx, K, faces, labels = make_scene(B)
        P, F = int(verts.shape[0]), len(faces)
        black = torch.zeros(B, S, S, 3, dtype=torch.uint8, device=DEV)
        _, keys, _ = render.render_batch(black, verts, idx, K, faces, smooth=False, return_debug=True)
        lab_dev = torch.from_numpy(labels).to(DEV)
        L = int(labels.max()) + 1
        idx_dev = idx.to(DEV).long()
        size = (S, S)

        def torch_maps(with_labels=False):
            none = keys == -1
            low = keys & 0xFFFFFFFF
            person = torch.where(none, -1, low // F).int()
            depth = torch.where(none, 0, keys >> 32).int().view(torch.float32)
            visible = torch.bincount(person[~none].long(), minlength=P)
            if not with_labels:
                return person, depth, visible
            face = torch.where(none, 0, low % F)
            label = torch.where(none, 255, lab_dev[face].long()).to(torch.uint8)
            label_px = torch.bincount(person[~none].long() * L + label[~none].long(), minlength=P * L).view(P, L)
            return person, depth, visible, label, label_px

        def torch_points():
            Kp = K[idx_dev]
            Z = verts[..., 2]
            u = Kp[:, 0, 0, None] * verts[..., 0] / Z + Kp[:, 0, 2, None]
            v = Kp[:, 1, 1, None] * verts[..., 1] / Z + Kp[:, 1, 2, None]
            c, r = u.floor().long(), v.floor().long()
            inside = (c >= 0) & (c < S) & (r >= 0) & (r < S) & (Z >= render.ZNEAR)
            k = keys[idx_dev[:, None].expand_as(c), r.clamp(0, S - 1), c.clamp(0, S - 1)]
            depth = (k >> 32).int().view(torch.float32)
            seen = (k == -1) | (Z <= depth + 0.03)
            return torch.where(inside, seen.to(torch.uint8), torch.full_like(seen, 2, dtype=torch.uint8))

        def amodal_by_renders():
            out = torch.zeros(P, dtype=torch.int64, device=DEV)
            for p in range(P):
                b = int(idx[p])
                _, k, _ = render.render_batch(black[b:b + 1], verts[p:p + 1], idx[p:p + 1] * 0, K[b:b + 1], faces, smooth=False, return_debug=True)
                out[p] = (k != -1).sum()
            return out

        ours = lambda **kw: maps.render_maps(verts, idx, K, faces, size, keys=keys, **kw)
        # the two routes agree before they are timed
        m = ours(face_labels=labels, points=verts)
        tm = torch_maps(True)
        assert torch.equal(m.person, tm[0]) and torch.equal(m.depth.view(torch.int32), tm[1].view(torch.int32))
        assert torch.equal(m.visible_px.long(), tm[2]) and torch.equal(m.label, tm[3]) and torch.equal(m.label_px.long(), tm[4])
        assert torch.equal(m.amodal_px.long(), amodal_by_renders())
        agree = float((m.point_visibility == torch_points()).float().mean())
        head = {"B": B, "P": P, "H": S, "W": S, "V": int(verts.shape[1]), "F": F, "L": L, "pixels_drawn": int((keys != -1).sum()),
                "mean_occlusion": round(float(m.occlusion.mean()), 4), "point_codes_equal_to_fp32_torch": round(agree, 6)}
        print(json.dumps({"part": "scene", **head}), flush=True)
        t = timed({"maps": lambda: ours(amodal=False), "torch_maps": torch_maps,
                   "labels": lambda: ours(amodal=False, face_labels=labels), "torch_labels": lambda: torch_maps(True),
                   "maps+points": lambda: ours(amodal=False, points=verts), "torch_points": torch_points,
                   "maps+amodal": lambda: ours(amodal=True),
                   "render": lambda: render.render_batch(black, verts, idx, K, faces, smooth=False, return_debug=True)}, a.reps, a.warmup)
        slow = timed({"amodal_by_renders": amodal_by_renders}, a.slow_reps, 1)
        med = lambda n: sorted(t[n])[len(t[n]) // 2]
        for part, new, old in (("maps", "maps", "torch_maps"), ("labels", "labels", "torch_labels")):
            print(json.dumps({"part": part, "B": B, "kernel": stat(t[new]), "torch": stat(t[old]),
                              "torch_over_kernel": round(med(old) / med(new), 3)}), flush=True)
        pts = med("maps+points") - med("maps")
        print(json.dumps({"part": "points", "B": B, "points": P * int(verts.shape[1]), "maps+points": stat(t["maps+points"]),
                          "kernel_minus_maps_ms": round(1e3 * pts, 4), "torch": stat(t["torch_points"]),
                          "torch_over_kernel": round(med("torch_points") / max(pts, 1e-9), 3)}), flush=True)
        amo = med("maps+amodal") - med("maps")
        sl = sorted(slow["amodal_by_renders"])
        print(json.dumps({"part": "amodal", "B": B, "maps+amodal": stat(t["maps+amodal"]), "kernel_minus_maps_ms": round(1e3 * amo, 4),
                          "one_render_per_person": stat(sl), "renders_over_kernel": round(sl[len(sl) // 2] / max(amo, 1e-9), 3)}), flush=True)
        print(json.dumps({"part": "render", "B": B, "render_batch": stat(t["render"])}), flush=True)


if __name__ == "__main__":
    main()
