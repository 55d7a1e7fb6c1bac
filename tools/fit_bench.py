"""Time the keypoint fit (KeypointFitter.fit: one call of mhmr_fit_keypoints for the whole loop, on the keypoint body model) against the
loop the README showed before it -- Model.decode_readout + the same objective in torch ops + torch.optim.Adam, driven from Python, which
skins the whole mesh and runs the full body backward every iteration -- on the same GPU, same persons, same targets, same settings.
  8 and 160 persons (1 and 20 images x 8), 50 steps, GMOF with the default priors, pose + shape + depth + loc optimised.
  Each repetition times both forms, alternating, by device events around the whole call (50 steps); medians are reported, and "faster" is
  true only if the fit's worst repetition beats the loop's best.  The final objectives of the two forms are reported side by side, not
  gated: the loop's forward is lbs.hip's mesh (f16 correctives), the fit's is the fp32 body layer, and 50 Adam steps carry the two apart.
  --trace-only runs the fit alone (for a kernel trace in a run of its own: launch-gap share = 1 - kernel time / event time).
Prints one JSON line per measurement.
  python tools/fit_bench.py [--reps 7] [--warmup 2] [--steps 50] [--trace-only]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from multi_hmr_amd import KeypointFitter, Model  # noqa: E402
import heads_oracle as ho  # noqa: E402  (the seeded input generator)
import synthetic  # noqa: E402

DEV = "cuda:0"
S, NB, NAME = 448, 10, "dinov2_vits14"
SIGMA, LR = 30.0, 0.01


def make_case(model, P, B, seed):
    hp = model.x_attention_head
    init = torch.cat([hp.init_body_pose, hp.init_betas, hp.init_cam, hp.init_expression], 1).flatten().cpu()
    readout, offset, idx, K = ho.make_inputs(init, P, B, S // 14, S, seed)
    g = torch.Generator().manual_seed(seed + 1)
    r, o, K = readout.to(DEV), offset.to(DEV), K.to(DEV)
    idx = tuple(i.to(DEV) for i in idx)
    with torch.no_grad():
        target = model.decode_readout(r + 0.05 * torch.randn(r.shape, generator=g).to(DEV), o + 0.05 * torch.randn(o.shape, generator=g).to(DEV), idx, K)["j2d"]
    return r, o, idx, K, target.contiguous(), torch.ones(P, 127, device=DEV)


def torch_loop(model, fitter, r0, o0, idx, K, kp, conf, steps):
    """The hand-written loop: decode_readout -> the objective in torch -> backward -> torch.optim.Adam."""
    nb = NB
    mask = fitter.column_mask(nb).to(DEV)
    W = r0.shape[1]
    r, o = r0.clone().requires_grad_(), o0.clone().requires_grad_()
    opt = torch.optim.Adam([r, o], lr=fitter.lr, betas=fitter.betas, eps=fitter.eps)
    w = fitter.weights
    E = None
    for it in range(steps + 1):
        opt.zero_grad(set_to_none=True)
        out = model.decode_readout(r, o, idx, K)
        s = ((out["j2d"] - kp) ** 2).sum(-1) / (fitter.sigma ** 2)
        E = (conf * (s / (1 + s))).sum(1)
        E = E + w["pose"] * ((r[:, :318] - r0[:, :318]) ** 2).sum(1) + w["shape"] * ((r[:, 318:318 + nb] - r0[:, 318:318 + nb]) ** 2).sum(1)
        E = E + w["depth"] * (r[:, 318 + nb] - r0[:, 318 + nb]) ** 2 + w["expression"] * ((r[:, 318 + nb + 3:] - r0[:, 318 + nb + 3:]) ** 2).sum(1)
        E = E + w["loc"] * ((o - o0) ** 2).sum(1)
        if it == steps:
            break
        E.sum().backward()
        r.grad *= mask[:W]
        o.grad *= mask[W:]
        opt.step()
    return E.detach()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def part(model, P, B, a):
    r, o, idx, K, kp, conf = make_case(model, P, B, seed=300 + P)
    fitter = KeypointFitter(model, sigma=SIGMA, robust="gmof", lr=LR)
    forms = {"fit": lambda: fitter.fit(r, o, idx, K, kp, conf, steps=a.steps).objective[-1],
             "loop": lambda: torch_loop(model, fitter, r, o, idx, K, kp, conf, a.steps)}
    if a.trace_only:
        forms.pop("loop")
    ms, last = {k: [] for k in forms}, {}
    for rep in range(a.warmup + a.reps):
        for name, fn in forms.items():                     # the forms alternate inside every repetition
            t, last[name] = timed(fn)
            if rep >= a.warmup:
                ms[name].append(t)
    out = dict(part=f"keypoint_fit_{P}", persons=P, images=B, steps=a.steps, launches_per_step_fit=14)
    for k, v in ms.items():
        out[k] = dict(median_ms=round(float(np.median(v)), 4), best_ms=round(min(v), 4), worst_ms=round(max(v), 4), reps=len(v),
                      median_us_per_step=round(float(np.median(v)) / (a.steps + 1) * 1e3, 2))
    if "loop" in ms:
        out["faster"] = bool(max(ms["fit"]) < min(ms["loop"]))
        out["median_ratio_loop_over_fit"] = round(float(np.median(ms["loop"]) / np.median(ms["fit"])), 2)
        out["max_rel_diff_of_final_objective_between_forms"] = float(((last["fit"] - last["loop"]).abs() / last["loop"].abs()).max())
    first = fitter.fit(r, o, idx, K, kp, conf, steps=0).objective[0]
    out["objective_first_to_last_mean"] = [round(float(first.mean()), 4), round(float(last["fit"].mean()), 4)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fit_bench measures on the GPU; there is none here")
    data, mean = synthetic.make_smplx_data(0), synthetic.make_mean_params(0)
    model = Model(backbone=NAME, img_size=S, smplx_data=data, mean_params=mean, backbone_depth=1, precision="f16").to(DEV).eval()
    for P, B in ((8, 1), (160, 20)):
        part(model, P, B, a)
