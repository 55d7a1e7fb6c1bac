"""Time the differentiable prediction decode (Model.decode_readout: mhmr_heads_decode + mhmr_lbs_forward forwards; mhmr_body_forward,
mhmr_heads_place_backward, mhmr_body_backward, mhmr_heads_decode_backward backwards) against the torch-op formulation on the same GPU:
roma-style torch ops for the 6D decode and the rotation vectors, torch ops for the distance chain, the placement and the projection,
around BodyModel.differentiable.  256 persons (32 images x 8) and 1 person, all fourteen cotangents.
  fwd_bwd    forward + backward of the scalar sum(cotangent * output), the two forms timed alternately (--reps repetitions after
             --warmup); a time is a host clock around the call ending in a device synchronise.  "faster" is true only if this path's
             worst repetition beats the torch path's best.
  placement  mhmr_heads_place_backward alone by device events (ten calls per repetition) against its HBM floor: (V + 127) points x
             (12 B u + 12 B + 8 B cotangents read + 12 B written) per person over 6.29 TB/s, the bytes computed here from the shapes.
Prints one JSON line per measurement.
  python tools/heads_bwd_bench.py [--reps 15] [--warmup 3]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from multi_hmr_amd import BodyModel, Model, _lib  # noqa: E402
import heads_oracle as ho  # noqa: E402  (the seeded input and cotangent generators)
import synthetic  # noqa: E402
from eval_bench import DEV, HBM_BYTES_PER_S, alternate, report  # noqa: E402

S, NB, NAME = 448, 10, "dinov2_vits14"


def rotmat_to_rotvec(R):
    """roma.rotmat_to_rotvec with torch ops on the device: the four candidate quaternions, the argmax picks one."""
    d = torch.diagonal(R, dim1=-2, dim2=-1)
    tr = d.sum(-1)
    cand = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        q = [None] * 4
        q[i], q[j], q[k], q[3] = 1 - tr + 2 * R[..., i, i], R[..., j, i] + R[..., i, j], R[..., k, i] + R[..., i, k], R[..., k, j] - R[..., j, k]
        cand.append(torch.stack(q, -1))
    cand.append(torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1], 1 + tr], -1))
    choice = torch.cat([d, tr[..., None]], -1).argmax(-1)
    q = torch.gather(torch.stack(cand, -2), -2, choice[..., None, None].expand(*choice.shape, 1, 4)).squeeze(-2)
    q = q / q.norm(dim=-1, keepdim=True)
    q = torch.where(q[..., 3:] < 0, -q, q)
    angle = 2 * torch.atan2(q[..., :3].norm(dim=-1), q[..., 3])
    small = angle.abs() <= 1e-3
    a = torch.where(small, torch.ones_like(angle), angle)
    scale = torch.where(small, 2 + angle ** 2 / 12 + 7 * angle ** 4 / 2880, a / torch.sin(a / 2))
    return scale[..., None] * q[..., :3]


def torch_decode(bm, readout, offset, idx, K, fn, center=15):
    P = readout.shape[0]
    M = readout[:, :318].reshape(P, 53, 2, 3)
    x, y = M[:, :, 0], M[:, :, 1]
    x = x / x.norm(dim=-1, keepdim=True)
    y = y - (x * y).sum(-1, keepdim=True) * x
    y = y / y.norm(dim=-1, keepdim=True)
    rotmat = torch.stack((x, y, torch.cross(x, y, dim=-1)), -1)
    rotvec = rotmat_to_rotvec(rotmat)
    shape, cam0, expr = readout[:, 318:318 + NB], readout[:, 318 + NB], readout[:, 318 + NB + 3:]
    Kp = K[idx[0]]
    dist = torch.clamp(torch.exp(cam0 * (Kp[:, 0, 0] / fn)) - 1e-10, 0.0, 50.0)
    loc = (torch.stack([idx[2], idx[1]], 1).float() + 0.5 + offset) * 14
    out = bm.differentiable(global_orient=rotvec[:, 0], body_pose=rotvec[:, 1:22], jaw_pose=rotvec[:, 52], left_hand_pose=rotvec[:, 22:37],
                            right_hand_pose=rotvec[:, 37:52], betas=shape, expression=expr)
    transl = torch.einsum("bij,bj->bi", torch.inverse(Kp), torch.cat([loc, torch.ones_like(loc[:, :1])], 1)) * dist[:, None]
    c = out.joints[:, [center]]
    v3d, j3d = out.vertices - c + transl[:, None], out.joints - c + transl[:, None]
    proj = lambda p: torch.einsum("bij,bkj->bki", Kp, p / p[:, :, -1:])[:, :, :2]
    return dict(offset=offset, loc=loc, rotmat=rotmat, rotvec=rotvec, shape=shape, expression=expr, dist_postprocessed=cam0[:, None],
                dist=dist[:, None], v3d=v3d, v2d=proj(v3d), j3d=j3d, j2d=proj(j3d), transl=transl, transl_pelvis=j3d[:, 0:1])


def make_case(model, P, B, seed):
    hp = model.x_attention_head
    init = torch.cat([hp.init_body_pose, hp.init_betas, hp.init_cam, hp.init_expression], 1).flatten().cpu()
    readout, offset, idx, K = ho.make_inputs(init, P, B, S // 14, S, seed)
    cot = ho.make_cotangents(P, 10475, S, seed + 1, nb=NB)
    leaves = [readout.to(DEV).requires_grad_(), offset.to(DEV).requires_grad_()]
    return leaves, tuple(i.to(DEV) for i in idx), K.to(DEV), {k: v.to(DEV) for k, v in cot.items()}


def part(model, bm, P, B, a):
    leaves, idx, K, cot = make_case(model, P, B, seed=200 + P)
    fn = float(ho.focal_norm(S))

    def step(outputs):
        for t in leaves:
            t.grad = None
        out = outputs()
        sum((out[k] * w).sum() for k, w in cot.items()).backward()
        return [t.grad for t in leaves]
    forms = {"hip": lambda: step(lambda: model.decode_readout(leaves[0], leaves[1], idx, K)),
             "torch": lambda: step(lambda: torch_decode(bm, leaves[0], leaves[1], idx, K, fn))}
    gh, gt = forms["hip"](), forms["torch"]()
    diff = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(gh, gt))
    report(f"heads_fwd_bwd_{P}", alternate(forms, a.reps, a.warmup), dict(persons=P, images=B, max_rel_diff_of_gradients_between_forms=diff))

    # the placement backward alone
    V, NJ = bm.num_vertices, bm.num_out_joints
    with torch.no_grad():
        out = model.decode_readout(leaves[0].detach(), leaves[1].detach(), idx, K)
        c = out["j3d"][:, [15]]
        U, UJ = (out["v3d"] - out["transl"][:, None] + c).contiguous(), (out["j3d"] - out["transl"][:, None] + c).contiguous()   # stand-ins of the right size and scale
    L = _lib.lib()
    nbytes = int(L.mhmr_heads_place_workspace_bytes(V, NJ, P))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    gx_v, gx_j, gt_tot = torch.empty(P, V, 3, device=DEV), torch.empty(P, NJ, 3, device=DEV), torch.empty(P, 3, device=DEV)
    d = _lib.HeadsPlaceDesc()
    d.P, d.V, d.NJ, d.center_joint = P, V, NJ, 15
    keep = dict(verts_u=U, joints_u=UJ, transl=out["transl"].contiguous(), K=K, det_b=idx[0].to(torch.int32).contiguous(), g_v3d=cot["v3d"],
                g_j3d=cot["j3d"], g_v2d=cot["v2d"], g_j2d=cot["j2d"], g_transl=cot["transl"], gx_v=gx_v, gx_j=gx_j, g_transl_total=gt_tot,
                workspace=ws)
    for n, t in keep.items():
        setattr(d, n, t.data_ptr())
    d.workspace_bytes = nbytes
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: _lib.check(L.mhmr_heads_place_backward(C.byref(d), stream), "mhmr_heads_place_backward")
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 10)
    nbytes_io = P * (V + NJ) * (12 + 12 + 8 + 12)
    floor_ms = nbytes_io / HBM_BYTES_PER_S * 1e3
    report(f"heads_place_backward_{P}", {"hip": ms}, dict(persons=P, points_per_person=V + NJ, bytes=nbytes_io, hbm_floor_ms=round(floor_ms, 5),
                                                         fraction_of_hbm_floor=round(floor_ms / float(np.median(ms)), 3),
                                                         note="two launches (streaming pass + finish) by device events"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("heads_bwd_bench measures on the GPU; there is none here")
    data, mean = synthetic.make_smplx_data(0), synthetic.make_mean_params(0)
    model = Model(backbone=NAME, img_size=S, smplx_data=data, mean_params=mean, backbone_depth=1, precision="f16").to(DEV).eval()
    bm = BodyModel(data, "smplx", num_betas=NB)
    for P, B in ((256, 32), (1, 1)):
        part(model, bm, P, B, a)
