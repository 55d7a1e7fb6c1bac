"""Time the differentiable body model (BodyModel.differentiable: mhmr_body_forward + mhmr_body_backward) against the torch-op formulation
of smplx's lbs with autograd (tools/eval_bench.py TorchBody + the einsum projection) on the same GPU: SMPL-X, all four cotangents,
256 persons and 1 person.
  fwd_bwd   forward + backward of the scalar sum(cotangent * output), the two forms timed alternately (--reps repetitions after
            --warmup); a time is a host clock around the call ending in a device synchronise.  "faster" is true only if this path's
            worst repetition beats the torch path's best.
  backward  the backward alone by device events (torch.autograd.grad from the four outputs to pose / betas / expression / transl, ten
            calls per repetition), and its share of the HBM roofline: (basis bytes x ceil(G / 8) + cotangent and saved vertex / joint
            bytes) over 6.29 TB/s (the measured copy rate of the MI355X), divided by the time of the whole call -- two launches, the
            workspace allocation and torch's backward of the cat / slice ops included, so a lower bound for the kernels.
Prints one JSON line per measurement.
  python tools/body_bwd_bench.py [--reps 15] [--warmup 3]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from multi_hmr_amd import BodyModel  # noqa: E402
import gt_oracle as go  # noqa: E402  (the seeded input generators)
import synthetic  # noqa: E402
from eval_bench import DEV, HBM_BYTES_PER_S, TorchBody, alternate, report  # noqa: E402

IMG = 448
NAMES = ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose", "betas", "expression", "transl")


def make_case(bm, G, seed):
    g = torch.Generator().manual_seed(seed)
    pose, transl, K = go.random_pose(g, G, 55), go.random_transl(g, G), go.camera_K(IMG, G, g).to(DEV)
    coef = torch.cat([torch.randn(G, 11, generator=g), 0.5 * torch.randn(G, 10, generator=g)], 1)
    V, NJ = bm.num_vertices, bm.num_out_joints
    cot = [torch.randn(G, V, 3, generator=g), torch.randn(G, NJ, 3, generator=g), torch.randn(G, V, 2, generator=g) / IMG,
           torch.randn(G, NJ, 2, generator=g) / IMG]
    leaves = [t.to(DEV).requires_grad_() for t in (pose, coef, transl)]
    return leaves, K, [c.to(DEV) for c in cot]


def hip_outputs(bm, leaves, K):
    p, c, t = leaves
    out = bm.differentiable(global_orient=p[:, 0], body_pose=p[:, 1:22], jaw_pose=p[:, 22], leye_pose=p[:, 23], reye_pose=p[:, 24],
                            left_hand_pose=p[:, 25:40], right_hand_pose=p[:, 40:], betas=c[:, :11], expression=c[:, 11:], transl=t, K=K)
    return [out.vertices, out.joints, out.v2d, out.j2d]


def torch_outputs(body, leaves, K):
    p, c, t = leaves
    v, j = body(p, c, t)
    proj = lambda x: torch.einsum("bij,bkj->bki", K, x / x[:, :, -1:])[:, :, :2]
    return [v, j, proj(v), proj(j)]


def part(bm, body, G, a):
    leaves, K, cot = make_case(bm, G, seed=100 + G)

    def step(outputs):
        for t in leaves:
            t.grad = None
        sum((o * w).sum() for o, w in zip(outputs(), cot)).backward()
        return [t.grad for t in leaves]
    forms = {"hip": lambda: step(lambda: hip_outputs(bm, leaves, K)), "torch": lambda: step(lambda: torch_outputs(body, leaves, K))}
    gh, gt = forms["hip"](), forms["torch"]()
    diff = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(gh, gt))
    report(f"body_fwd_bwd_{G}_smplx", alternate(forms, a.reps, a.warmup), dict(persons=G, max_rel_diff_of_gradients_between_forms=diff))

    outs = hip_outputs(bm, leaves, K)
    for _ in range(a.warmup):
        torch.autograd.grad(outs, leaves, grad_outputs=cot, retain_graph=True)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            torch.autograd.grad(outs, leaves, grad_outputs=cot, retain_graph=True)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 10)
    passes = math.ceil(G / 8)
    io_bytes = sum(int(t.numel()) * 4 for t in cot) + int(outs[0].numel() + outs[1].numel()) * 4
    floor_ms = (bm.basis_bytes * passes + io_bytes) / HBM_BYTES_PER_S * 1e3
    med = float(np.median(ms))
    report(f"body_backward_{G}_smplx", {"hip": ms}, dict(persons=G, basis_bytes=bm.basis_bytes, passes=passes, cotangent_and_vertex_bytes=io_bytes,
                                                        hbm_floor_ms=round(floor_ms, 4), fraction_of_hbm_roofline=round(floor_ms / med, 3),
                                                        note="time of the whole backward call by device events"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("body_bwd_bench measures on the GPU; there is none here")
    data = synthetic.make_smplx_data(0)
    bm, body = BodyModel(data, "smplx", num_betas=11), TorchBody(data)
    for G in (256, 1):
        part(bm, body, G, a)
