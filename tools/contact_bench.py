"""Time the contacts between persons (multi_hmr_amd/contact.py, csrc/contact.hip) against a chunked torch implementation of the same
contract (include/mhmr.h, mhmr_contact_desc) on the same GPU and the same scene.  Meshes the size of SMPL-X: closed icospheres of
subdivision 5 (V = 10242, F = 20480), radius 0.5 m.
  pair        2 persons overlapping (centres 0.64 m apart): both ordered pairs evaluated, about a third of the vertices in reach.
  row         8 persons in a row in one image, centres 0.99 m apart: each touches its neighbours (1 cm of overlap), 14 ordered pairs.
  crowd       160 persons in 32 images, 5 per image, scattered over 4 x 4 x 13 m: mostly apart, the boxes decide.
The torch form builds the pair list on the host from the boxes (a synchronisation the kernel does not need), gathers the vertices in
reach, and evaluates them against all faces in chunks whose [v, F, 3] temporaries stay near 64 MB: the closest point by the region
method (the same barycentric form as the kernel), the winding number where the vertex is in the un-inflated box, the minimum over b.
Both forms are checked against each other before they are timed (the +inf pattern and the largest difference are printed).  The forms
are timed alternately (--reps after --warmup; the torch form --slow-reps after 1); a time is a host clock around the call ending in a
device synchronise.  Prints one JSON line per case with median / best / worst in milliseconds; there is no gate: a loss is printed as
a loss.
  python tools/contact_bench.py [--reps 10] [--warmup 3] [--slow-reps 2] [--cases pair row crowd]"""
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

from multi_hmr_amd import contacts  # noqa: E402
import contact_oracle  # noqa: E402  (the icosphere generator)

DEV = "cuda:0"
CHUNK = 256


def make_scene(case, seed=0):
    v, faces = contact_oracle.icosphere(5)
    v = 0.5 * v
    if case == "pair":
        centres, idx = np.array([[0.3, -0.2, 6.0], [0.9, -0.1, 6.2]]), [0, 0]
    elif case == "row":
        centres, idx = np.array([[0.99 * k - 3.5, 0.0, 6.0] for k in range(8)]), [0] * 8
    else:
        g = np.random.default_rng(seed)
        centres = np.concatenate([g.uniform(-2, 2, (160, 2)), g.uniform(2, 15, (160, 1))], 1)
        idx = (np.arange(160) // 5).tolist()
    verts = torch.from_numpy((v[None] + centres[:, None]).astype(np.float32)).to(DEV)
    return verts, idx, faces


def torch_contacts(verts, idx, faces_dev, max_dist=0.10, tau=0.01):
    """sdf [P, V] and pair_distance [P, P] of the contract in chunked torch (fp32)."""
    P, V = verts.shape[:2]
    m = torch.tensor(max_dist, dtype=torch.float32, device=verts.device)
    lo, hi = verts.amin(1), verts.amax(1)
    ilo, ihi = lo - m, hi + m
    img = torch.as_tensor(idx, device=verts.device)
    hit = (ilo[:, None] <= ihi[None]).all(-1) & (ilo[None] <= ihi[:, None]).all(-1) & (img[:, None] == img[None])
    hit &= ~torch.eye(P, dtype=torch.bool, device=verts.device)
    sdf = torch.full((P, V), float("inf"), device=verts.device)
    pd = torch.full((P, P), float("inf"), device=verts.device)
    dot = lambda x, y: (x * y).sum(-1)
    for a, b in hit.nonzero().tolist():                                 # the host-built pair list
        va = verts[a]
        live = ((ilo[b] <= va) & (va <= ihi[b])).all(-1).nonzero()[:, 0]
        if not len(live):
            continue
        A, B, C = (verts[b][faces_dev[:, k]] for k in range(3))
        ab, ac = (B - A)[None], (C - A)[None]
        s_all = []
        for c0 in range(0, len(live), CHUNK):
            p = va[live[c0:c0 + CHUNK]][:, None]
            ap, bp, cp = p - A[None], p - B[None], p - C[None]
            d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
            vc, vb, va_ = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
            e, h = d4 - d3, d5 - d6
            one, zero = torch.ones_like(d1), torch.zeros_like(d1)
            ns, nt, den = vb, vc, va_ + vb + vc
            for cond, s_, t_, d_ in (((va_ <= 0) & (e >= 0) & (h >= 0), h, e, e + h), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6),
                                     ((d6 >= 0) & (d5 <= d6), zero, one, one), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3),
                                     ((d3 >= 0) & (d4 <= d3), one, zero, one), ((d1 <= 0) & (d2 <= 0), zero, zero, one)):
                ns, nt, den = torch.where(cond, s_, ns), torch.where(cond, t_, nt), torch.where(cond, d_, den)
            s_, t_ = (ns / den)[..., None], (nt / den)[..., None]
            off = ap - s_ * ab - t_ * ac
            d = dot(off, off).amin(1).sqrt()
            inbox = ((lo[b] <= p[:, 0]) & (p[:, 0] <= hi[b])).all(-1)
            la, lb, lc = ap.norm(dim=-1), bp.norm(dim=-1), cp.norm(dim=-1)
            num = -dot(ap, torch.linalg.cross(bp, cp))
            dn = la * lb * lc + dot(ap, bp) * lc + dot(bp, cp) * la + dot(cp, ap) * lb
            w = torch.atan2(num, dn).sum(1) / (2 * np.pi)
            s_all.append(torch.where(inbox & (w.abs() > 0.5), -d, d))
        s = torch.cat(s_all)
        pd[a, b] = torch.where(s.min() <= m, s.min(), pd[a, b])
        s = torch.where(s <= m, s, torch.full_like(s, float("inf")))
        sdf[a, live] = torch.minimum(sdf[a, live], s)
    return sdf, pd


def timed(forms, reps, warmup):
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slow-reps", type=int, default=2)
    ap.add_argument("--cases", nargs="+", default=["pair", "row", "crowd"])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "contact_bench needs the GPU"
    for case in a.cases:
        verts, idx, faces = make_scene(case)
        faces_dev = torch.from_numpy(faces).to(DEV).long()
        P, V, F = int(verts.shape[0]), int(verts.shape[1]), len(faces)
        c = contacts(verts, idx, faces)
        sdf_t, pd_t = torch_contacts(verts, idx, faces_dev)
        fin = torch.isfinite(c.sdf) & torch.isfinite(sdf_t)
        pairs = int(torch.isfinite(c.pair_distance).sum())
        head = {"case": case, "P": P, "V": V, "F": F, "pairs_within_max_dist": pairs, "vertices_within_max_dist": int(torch.isfinite(c.sdf).sum()),
                "inside_vertices": int(c.inside_count.sum()), "contact_vertices": int(c.contact_count.sum()),
                "max_penetration_m": round(float(c.penetration_depth.max()), 5),
                "inf_pattern_differs_from_torch": int((torch.isfinite(c.sdf) != torch.isfinite(sdf_t)).sum()),
                "sign_differs_from_torch": int((torch.sign(c.sdf[fin]) != torch.sign(sdf_t[fin])).sum()),
                "max_abs_diff_to_torch_m": float((c.sdf[fin].abs() - sdf_t[fin].abs()).abs().max()) if fin.any() else 0.0}
        print(json.dumps({"part": "scene", **head}), flush=True)
        t = timed({"contacts": lambda: contacts(verts, idx, faces),
                   "contacts_sdf_only": lambda: contacts(verts, idx, faces, want=("sdf",))}, a.reps, a.warmup)
        slow = timed({"torch": lambda: torch_contacts(verts, idx, faces_dev)}, a.slow_reps, 1)
        med = lambda ts: sorted(ts)[len(ts) // 2]
        print(json.dumps({"part": "time", "case": case, "kernel": stat(t["contacts"]), "kernel_sdf_only": stat(t["contacts_sdf_only"]),
                          "torch": stat(slow["torch"]), "torch_over_kernel": round(med(slow["torch"]) / med(t["contacts"]), 1)}), flush=True)


if __name__ == "__main__":
    main()
