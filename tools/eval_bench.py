"""Time the ground-truth path against the dense torch formulation the reference uses, on the same GPU, with random (non-zero) inputs:
  gt       GroundTruth.prepare for 32 images x 8 humans with SMPL-X annotations (mhmr_body_forward + mhmr_gt_targets) against
           prepare_gt written with torch ops as train.py:58-182 has it (dense lbs, einsum projection, the per-human Python loop of the
           occlusion rule);
  body     mhmr_body_forward alone for 256 persons, and its share of the HBM roofline: basis bytes x ceil(G / 8) over 6.29 TB/s (the
           measured copy rate of the MI355X) divided by the time of the whole call (three launches), so a lower bound for the kernel;
  metrics  the 3DPW metric path for 64 matches (smplx2smpl, PVE / PA-PVE, H36M MPJPE / PA-MPJPE: two mhmr_sparse_regress + two
           mhmr_eval_mesh_errors) against the dense 6890 x 10475 matmul + batched SVD registration.
  validation  evaluate_dataset on the synthetic ViT-L 896^2 model over 64 images: image by image (batched=False, batches of 1) against
           the batched evaluation (batched=True) in batches of 8 and of 32, per image, with the split into prepare / forward / evaluator
           and the share of an epoch.
The two forms of a part are timed alternately (--reps repetitions after --warmup); a time is a host clock around the call ending in a
device synchronise.  Prints one JSON line per part with median / best / worst of both forms; "faster" is true only if the new path's
worst repetition beats the torch path's best.
  python tools/eval_bench.py [--part gt|body|metrics|validation|all] [--reps 15] [--warmup 3]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multi_hmr_amd import BodyModel, GroundTruth, SparseRegressor  # noqa: E402
from multi_hmr_amd.constants import H36M_TO_J14, SMPLX_EXTRA_JOINT_VERTS  # noqa: E402
from multi_hmr_amd.evaluate import mesh_errors  # noqa: E402
import gt_oracle as go  # noqa: E402  (the seeded annotation generator)
import synthetic  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
DEV = "cuda:0"


class TorchBody:
    """smplx.lbs.lbs + the extra joints with torch ops on the device (dense J_regressor, dense skinning matmul, 4x4 chain)."""

    def __init__(self, data, num_betas=11):
        t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(DEV)
        sd = np.asarray(data["shapedirs"])
        self.v_template, self.J_regressor, self.weights = t(data["v_template"]), t(data["J_regressor"]), t(data["weights"])
        self.shapedirs = t(np.concatenate([sd[:, :, :num_betas], sd[:, :, 300:310]], -1))
        pd = np.asarray(data["posedirs"])
        self.posedirs = t(pd.reshape(-1, pd.shape[-1]).T)
        self.parents = [int(p) for p in np.asarray(data["kintree_table"])[0].astype(np.int64)]
        self.extra = torch.tensor(SMPLX_EXTRA_JOINT_VERTS, device=DEV)
        self.lmk = torch.from_numpy(np.asarray(data["f"], dtype=np.int64)[np.asarray(data["lmk_faces_idx"], dtype=np.int64)]).to(DEV)
        self.bary = t(data["lmk_bary_coords"])

    def __call__(self, pose, coef, transl):
        B, J = pose.shape[0], pose.shape[1]
        v_shaped = self.v_template + torch.einsum("bl,mkl->bmk", coef, self.shapedirs)
        Jt = torch.einsum("bik,ji->bjk", v_shaped, self.J_regressor)
        rv = pose.reshape(-1, 3)
        angle = torch.norm(rv + 1e-8, dim=1, keepdim=True)
        d = rv / angle
        z = torch.zeros_like(angle)
        Km = torch.cat([z, -d[:, 2:3], d[:, 1:2], d[:, 2:3], z, -d[:, 0:1], -d[:, 1:2], d[:, 0:1], z], 1).view(-1, 3, 3)
        R = (torch.eye(3, device=DEV) + torch.sin(angle)[:, None] * Km + (1 - torch.cos(angle))[:, None] * torch.bmm(Km, Km)).view(B, J, 3, 3)
        v_posed = torch.matmul((R[:, 1:] - torch.eye(3, device=DEV)).reshape(B, -1), self.posedirs).view(B, -1, 3) + v_shaped
        rel = Jt.clone()
        rel[:, 1:] -= Jt[:, self.parents[1:]]
        T = torch.zeros(B, J, 4, 4, device=DEV)
        T[:, :, :3, :3], T[:, :, :3, 3], T[:, :, 3, 3] = R, rel, 1
        chain = [T[:, 0]]
        for i in range(1, J):
            chain.append(torch.matmul(chain[self.parents[i]], T[:, i]))
        G = torch.stack(chain, 1)
        A = G - torch.nn.functional.pad(torch.matmul(G, torch.nn.functional.pad(Jt, [0, 1]).unsqueeze(-1)), [3, 0])
        Tv = torch.matmul(self.weights, A.view(B, J, 16)).view(B, -1, 4, 4)
        v = torch.matmul(Tv, torch.nn.functional.pad(v_posed, [0, 1], value=1.0).unsqueeze(-1))[:, :, :3, 0]
        lm = torch.einsum("blfi,lf->bli", v[:, self.lmk.reshape(-1)].view(B, -1, 3, 3), self.bary)
        j = torch.cat([G[:, :, :3, 3], v[:, self.extra], lm], 1)
        return v + transl[:, None], j + transl[:, None]


def torch_prepare_gt(y, body, img_size=448, patch=14):
    """train.py:58-182 (the SMPL-X family) with torch ops, the occlusion loop included."""
    valid = y["valid_humans"]
    bs, nh = valid.shape
    ib, ih = torch.where(valid > 0)
    n = int(valid.sum())
    K = y["K"][ib]
    s = lambda k: y[k][ib, ih].reshape(n, -1, 3)
    pose = torch.cat([s("smplx_root_pose"), s("smplx_body_pose"), s("smplx_jaw_pose"), s("smplx_leye_pose"), s("smplx_reye_pose"),
                      s("smplx_left_hand_pose"), s("smplx_right_hand_pose")], 1)
    coef = torch.cat([y["smplx_shape"][ib, ih], torch.zeros(n, 10, device=DEV)], 1)
    verts, jts = body(pose, coef, y["smplx_transl"][ib, ih])
    proj = lambda x: torch.einsum("bij,bkj->bki", K, x / x[:, :, -1:])[:, :, :2]
    t = dict(j2d=proj(jts), v2d=proj(verts), transl=jts[:, 15], transl_pelvis=jts[:, 0], dist=jts[:, 0, -1], v3d=verts, j3d=jts)
    fn = img_size / (2 * np.tan(np.radians(60) / 2))
    t["dist_postprocessed"] = torch.log(t["dist"] + 1e-10) * (fn / K[:, 0, 0])
    n_patch = img_size // patch
    pk_loc = proj(t["transl"].unsqueeze(1)).squeeze(1)
    pk_idx = torch.clamp((pk_loc // patch).int(), 0, n_patch - 1)
    t["offset"], t["loc"] = (pk_loc - (pk_idx + 0.5) * patch) / patch, pk_loc
    scores, visible = torch.zeros(bs, n_patch, n_patch, device=DEV), torch.ones(n, device=DEV)
    for k in range(n):
        i, _x, _y = int(ib[k]), pk_idx[k, 1], pk_idx[k, 0]
        if scores[i, _x, _y] == 1:
            visible[k] = 0
        else:
            scores[i, _x, _y] = 1
    vis = torch.where(visible)[0]
    out = {k: v[vis] for k, v in t.items()}
    out["idx"] = (ib[vis], pk_idx[vis, 1], pk_idx[vis, 0], torch.zeros_like(ib[vis]))
    out["scores"] = scores
    return out


def torch_metrics(v_hat, c_hat, v_gt, c_gt, s2s_dense, h36m_dense):
    """train.py:372-429 batched over the matches with torch ops (dense matmuls, SVD registration as roma does it)."""
    def pair(a_hat, a):
        e = (torch.sqrt(((a - a_hat) ** 2).sum(-1)) * 1000).mean(-1)
        xm, ym = a_hat.mean(1, keepdim=True), a.mean(1, keepdim=True)
        xh, yh = a_hat - xm, a - ym
        U, S, Vh = torch.linalg.svd(yh.transpose(1, 2) @ xh)
        d = torch.det(U @ Vh)
        D = torch.ones_like(S)
        D[:, -1] = d
        R = (U * D[:, None]) @ Vh
        sc = (S * D).sum(-1) / (xh ** 2).sum((1, 2))
        pa = sc[:, None, None] * (a_hat @ R.transpose(1, 2)) + (ym - sc[:, None, None] * (xm @ R.transpose(1, 2)))
        return e, (torch.sqrt(((a - pa) ** 2).sum(-1)) * 1000).mean(-1)
    v_ctx, vh_ctx = v_gt - c_gt[:, None], s2s_dense @ (v_hat - c_hat[:, None])
    pve, pa = pair(vh_ctx, v_ctx)
    h, hh = h36m_dense @ v_ctx, h36m_dense @ vh_ctx
    mp, pamp = pair((hh - hh[:, :1])[:, H36M_TO_J14], (h - h[:, :1])[:, H36M_TO_J14])
    return pve, pa, mp, pamp


def alternate(forms, reps, warmup):
    """forms: {name: callable}; timed alternately -> {name: [ms, ...]}."""
    ms = {k: [] for k in forms}
    for r in range(warmup + reps):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    return ms


def report(part, ms, extra=None):
    out = dict(part=part)
    for k, v in ms.items():
        out[k] = dict(median_ms=round(float(np.median(v)), 4), best_ms=round(min(v), 4), worst_ms=round(max(v), 4), reps=len(v))
    if "hip" in ms and "torch" in ms:
        out["faster"] = bool(max(ms["hip"]) < min(ms["torch"]))
        out["median_ratio_torch_over_hip"] = round(float(np.median(ms["torch"]) / np.median(ms["hip"])), 2)
    out.update(extra or {})
    print(json.dumps(out), flush=True)
    return out


def part_gt(data, a):
    y = go.make_y("smplx", 7, 448, [8] * 32)
    y = {k: v.to(DEV) for k, v in y.items()}
    builder, body = GroundTruth(448, smplx_neutral=BodyModel(data, "smplx", num_betas=11)), TorchBody(data)
    g, t = builder.prepare(dict(y)), torch_prepare_gt(dict(y), body)
    same = all(torch.equal(x.long(), z.long()) for x, z in zip(g["idx"], t["idx"])) and torch.equal(g["scores"], t["scores"])
    dv = float((g["v3d"] - t["v3d"]).abs().max())
    ms = alternate({"hip": lambda: builder.prepare(dict(y)), "torch": lambda: torch_prepare_gt(dict(y), body)}, a.reps, a.warmup)
    return report("gt_prepare_32x8_smplx", ms, dict(humans=256, visible=int(g["v3d"].shape[0]), idx_and_scores_identical=same, v3d_max_abs_diff_m=dv))


def part_body(data, a):
    bm = BodyModel(data, "smplx", num_betas=11)
    g = torch.Generator().manual_seed(1)
    G = 256
    pose, transl = go.random_pose(g, G, 55).to(DEV), go.random_transl(g, G).to(DEV)
    kw = dict(global_orient=pose[:, 0], body_pose=pose[:, 1:22], jaw_pose=pose[:, 22], leye_pose=pose[:, 23], reye_pose=pose[:, 24],
              left_hand_pose=pose[:, 25:40], right_hand_pose=pose[:, 40:], betas=torch.randn(G, 11, generator=g).to(DEV),
              expression=torch.randn(G, 10, generator=g).to(DEV), transl=transl)
    for _ in range(a.warmup):
        bm(**kw)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            bm(**kw)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 10)
    floor_ms = bm.basis_bytes * math.ceil(G / 8) / HBM_BYTES_PER_S * 1e3
    med = float(np.median(ms))
    return report("body_forward_256_smplx", {"hip": ms}, dict(basis_bytes=bm.basis_bytes, passes=math.ceil(G / 8), hbm_floor_ms=round(floor_ms, 4),
                                                             fraction_of_hbm_roofline=round(floor_ms / med, 3),
                                                             note="time of the whole call (pose + vertex + joint launches, host allocations) by device events"))


def part_metrics(a):
    s2s, h36m = synthetic.make_smplx2smpl(0), synthetic.make_h36m_regressor(0)
    rs, rh = SparseRegressor(s2s), SparseRegressor(h36m)
    s2s_d, h36m_d = torch.from_numpy(s2s.toarray()).to(DEV), torch.from_numpy(h36m).to(DEV)
    g = torch.Generator().manual_seed(2)
    M = 64
    v_gt = (torch.randn(M, 6890, 3, generator=g) * 0.3 + torch.randn(M, 1, 3, generator=g) * 3).to(DEV)
    v_hat = (torch.randn(M, 10475, 3, generator=g) * 0.3 + torch.randn(M, 1, 3, generator=g) * 3).to(DEV)
    c_gt, c_hat = v_gt[:, 0].contiguous(), v_hat[:, 0].contiguous()
    j14 = torch.tensor(H36M_TO_J14, device=DEV)

    def hip():
        vh = rs(v_hat, c_hat)
        pve, pa = mesh_errors(vh, v_gt, None, c_gt)
        h, hh = rh(v_gt, c_gt), rh(vh)
        mp, pamp = mesh_errors(hh[:, j14], h[:, j14], hh[:, 0], h[:, 0])
        return pve, pa, mp, pamp
    diff = max(float((x - z).abs().max() / z.abs().max()) for x, z in zip(hip(), torch_metrics(v_hat, c_hat, v_gt, c_gt, s2s_d, h36m_d)))
    ms = alternate({"hip": hip, "torch": lambda: torch_metrics(v_hat, c_hat, v_gt, c_gt, s2s_d, h36m_d)}, a.reps, a.warmup)
    return report("metrics_3dpw_64_matches", ms, dict(max_rel_diff_between_forms=diff, dense_matrix_bytes=int(s2s_d.numel() * 4), csr_nnz=rs.nnz))


def part_validation(data, a):
    """The validation loop on the synthetic ViT-L 896^2 model over the same 64 images and ground truth (4 humans per image), three forms
    timed alternately: evaluate_dataset(batched=False) in batches of 1 (image by image, host matching), batched=True in batches of 8 and
    of 32.  The synthetic weights make no meaningful detections, so every form runs ``use_gt_idx=True`` (the ground truth's cells through the is_training
    forward: one prediction per annotated human), which leaves the evaluator the work it has behind a detector that finds everybody.
    A repetition's time is taken twice, by device events and by the host clock around the whole call (its one final read included).
    The split into prepare / forward / evaluator comes from a second pass with a synchronise after every phase (their sum exceeds the
    pipelined time above).  "faster" asks that the batch-32 form's worst repetition beats the per-image form's best."""
    from multi_hmr_amd import Evaluator, Model, evaluate_dataset
    S, name, n_img, humans = 896, "dinov2_vitl14", 64, 4
    mean = synthetic.make_mean_params(0)
    model = Model(backbone=name, img_size=S, smplx_data=data, mean_params=mean, precision="f16")
    model.load_state_dict(synthetic.make_state_dict(name, S, seed=0, mean_params=mean), strict=True)
    model = model.to(DEV).eval()
    builder = GroundTruth(S, patch_size=14, smplx_neutral=BodyModel(data, "smplx", num_betas=11))
    g = torch.Generator().manual_seed(0)
    ys = [go.make_y("smplx", 100 + i, S, [humans], depth=2.6) for i in range(n_img)]
    xs = [torch.randn(1, 3, S, S, generator=g).to(DEV) for _ in range(n_img)]

    def batches(bs):
        out = []
        for i in range(0, n_img, bs):
            y = {k: (torch.cat([t[k] for t in ys[i:i + bs]]).to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in ys[i].items()}
            out.append((torch.cat(xs[i:i + bs]), y))
        return out
    clone = lambda bl: [(x, {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in y.items()}) for x, y in bl]   # prepare writes into y
    forms = {"per_image_b1": (batches(1), False), "batched_b8": (batches(8), True), "batched_b32": (batches(32), True)}
    run = lambda bl, batched: evaluate_dataset(model, bl, builder, use_gt_idx=True, evaluator=Evaluator(), batched=batched)
    summaries = {k: run(clone(v[0]), v[1]) for k, v in forms.items()}
    wall, devt = {k: [] for k in forms}, {k: [] for k in forms}
    for r in range(a.warmup + a.reps):
        for k, v in forms.items():
            fresh = clone(v[0])                                                 # outside the clock
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            run(fresh, v[1])
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                wall[k].append((time.perf_counter() - t0) * 1e3 / n_img)
                devt[k].append(e0.elapsed_time(e1) / n_img)

    def split(bl, batched):
        t = dict(prepare=0.0, forward=0.0, evaluator=0.0)
        ev = Evaluator()

        def timed(key, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            t[key] += (time.perf_counter() - t0) * 1e3 / n_img
            return out
        for x, y in clone(bl):
            gt = timed("prepare", lambda: builder.prepare(y))
            out = timed("forward", lambda: model(x, idx=gt["idx"], K=gt["K"], is_training=True))
            if batched:
                timed("evaluator", lambda: ev.update_batched(out, gt["idx"][0], gt))
            else:
                pelvis = out["transl_pelvis"] if "transl_pelvis" in out else out["j3d"][:, :1]
                pred = [dict(v3d=out["v3d"][i], j3d=out["j3d"][i], j2d=out["j2d"][i], transl_pelvis=pelvis[i]) for i in range(int(gt["idx"][0].shape[0]))]
                timed("evaluator", lambda: ev.update(pred, gt))
        timed("evaluator", ev.summary)
        return {k: round(v, 4) for k, v in t.items()}
    for k, v in forms.items():
        split(*v)                                                               # warm
    stat = lambda v: dict(median_ms=round(float(np.median(v)), 4), best_ms=round(min(v), 4), worst_ms=round(max(v), 4), reps=len(v))
    out = dict(part="validation_vitl896_64_images", unit="ms per image", humans_per_image=humans)
    for k, v in forms.items():
        out[k] = dict(wall=stat(wall[k]), device=stat(devt[k]), split_synchronised=split(*v),
                      summary={m: round(float(summaries[k][m]), 6) for m in ("pve", "pa_pve", "mpjpe", "pa_mpjpe", "matched", "count")})
    out["faster"] = bool(max(wall["batched_b32"]) < min(wall["per_image_b1"]))
    out["median_ratio_b1_over_b32"] = round(float(np.median(wall["per_image_b1"]) / np.median(wall["batched_b32"])), 3)
    out["margin_ms"] = round(min(wall["per_image_b1"]) - max(wall["batched_b32"]), 4)
    # share of an epoch of 100 training steps followed by three validation sets of 1000 images (the sizes are an assumption of this line)
    for tag, step_ms in (("frozen_backbone_14ms_step", 14.0), ("all_blocks_bf16_1700ms_step", 1700.0)):
        out["epoch_share_" + tag] = {k: round(3000 * float(np.median(wall[k])) / (3000 * float(np.median(wall[k])) + 100 * step_ms), 4) for k in forms}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["gt", "body", "metrics", "validation", "all"], default="all")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench measures on the GPU; there is none here")
    data = synthetic.make_smplx_data(0)
    if a.part in ("gt", "all"):
        part_gt(data, a)
    if a.part in ("body", "all"):
        part_body(data, a)
    if a.part in ("metrics", "all"):
        part_metrics(a)
    if a.part in ("validation", "all"):
        part_validation(data, a)
