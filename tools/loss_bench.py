"""Time the training loss (multi_hmr_amd.loss: mhmr_loss_forward / mhmr_loss_backward) against the reference's formulation restated
with torch ops (elementwise differences, abs / sum / mean chains, torch.where masks, nan_to_num, autograd for the gradients) on the
same GPU and the same seeded inputs (tests/loss_oracle.make_inputs, V = 10475, J = 127):
  fwd      the eleven values;
  fwdbwd   the values and the gradient of total with respect to every prediction,
at 32 images x 8 persons (P = 256) and at one person.  The two forms of a part are timed alternately (--reps repetitions after
--warmup); a time is a host clock around the call ending in a device synchronise, so it contains the host work of either form.
"faster" is true only if this path's worst repetition beats the torch path's best.
  roofline the C entries alone at P = 256, 50 calls between two device events: forward reads 108 MB, backward reads 108 MB and
           writes 54 MB, against 6.29 TB/s (the measured copy rate of the MI355X).  The host issues the launches back to back; where it
           is slower than the GPU the figure is a lower bound of the kernels' share.
Prints one JSON line per part.
  python tools/loss_bench.py [--reps 15] [--warmup 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multi_hmr_amd import Loss, _lib, loss_and_grads  # noqa: E402
from multi_hmr_amd.loss import _Prepared  # noqa: E402
import loss_oracle as lo  # noqa: E402  (the seeded input maker)

HBM_BYTES_PER_S = 6.29e12
DEV = "cuda:0"
S = 448.0


def torch_loss(h, y, epoch, img_size, a):
    """The reference's formulation (loss.py:8-40, 47-115) with torch ops."""
    def l1(d, dims=None):
        d = d.abs()
        return (d.sum(dims) if dims is not None else d).mean(0)
    tgt = (y["scores"] >= 1).to(torch.int64).unsqueeze(-1)
    pos, neg = tgt.eq(1).float(), tgt.lt(1).float()
    pred = h["scores"]
    lp = (torch.log(pred + 1e-7) * torch.pow(1 - pred, 2) * pos).sum()
    ln = (torch.log(1 - pred + 1e-7) * torch.pow(pred, 2) * torch.pow(1 - tgt, 4) * neg).sum()
    npos = pos.sum()
    t = {"bce": -ln if npos == 0 else -(lp + ln) / npos}                     # (a host synchronisation, as in the reference)
    t["offset"] = l1(h["offset"] - y["offset"], -1)
    t["rotmat"] = l1(h["rotmat"] - y["rotmat"], [1, 2, 3])
    sd = min(h["shape"].shape[1], y["shape"].shape[1])
    t["shape"] = l1(h["shape"][:, :sd] - y["shape"][:, :sd], -1)
    t["dist"] = l1(h["dist_postprocessed"].squeeze(1) - y["dist_postprocessed"])
    t["transl"] = l1(h["transl"] - y["transl"], -1)
    c, ch = y["transl_pelvis"].reshape(-1, 1, 3), h["transl_pelvis"].reshape(-1, 1, 3)
    for k in ("j3d", "v3d"):
        t[k] = ((y[k] - c) - (h[k] - ch)).abs().sum(-1).mean(-1).mean(0)
    for k in ("v2d", "j2d"):
        i = torch.where(((y[k] > 0).int() * (y[k] < img_size).int()).sum(-1) == 2)
        t[k] = l1(h[k][i[0], i[1]] - y[k][i[0], i[1]], -1)
    t = {k: torch.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0) for k, v in t.items()}
    total = sum(getattr(a, "alpha_" + k) * t[k] for k in lo.KEYS[1:9])
    if epoch >= a.start_2d_epoch:
        total = total + a.alpha_j2d * t["j2d"] + a.alpha_v2d * t["v2d"]
    return total, dict(t, total=total)


def alternate(forms, reps, warmup):
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


def inputs(P, B, G):
    h, y = lo.make_inputs(11, P, 10475, 127, B=B, G=G, img_size=S)
    return {k: torch.from_numpy(v).to(DEV) for k, v in h.items()}, {k: torch.from_numpy(v).to(DEV) for k, v in y.items()}


def part_compare(P, B, G, a):
    args, epoch = lo.default_args(), lo.DEFAULTS["start_2d_epoch"]
    h, y = inputs(P, B, G)
    loss = Loss(args)

    def torch_fwdbwd():
        leaves = {k: v.detach().requires_grad_(True) for k, v in h.items()}
        torch_loss(leaves, y, epoch, S, args)[0].backward()
        return leaves

    def hip_fwd():
        with torch.no_grad():
            return loss(h, y, epoch=epoch, img_size=S)

    with torch.no_grad():
        tv = torch_loss(h, y, epoch, S, args)[1]
    hv = hip_fwd()[1]
    diff = max(abs(float(hv[k]) - float(tv[k])) / max(abs(float(tv[k])), 1e-30) for k in lo.KEYS)
    gh, gt = loss_and_grads(h, y, epoch, S, args)[1], torch_fwdbwd()
    gdiff = max(float((gh[k] - gt[k].grad).abs().max() / gt[k].grad.abs().max()) for k in gh)
    extra = dict(persons=P, images=B, max_rel_diff_of_values=diff, max_rel_diff_of_gradients=gdiff)
    report(f"loss_fwd_{P}_persons", alternate({"hip": hip_fwd, "torch": lambda: torch.no_grad()(torch_loss)(h, y, epoch, S, args)}, a.reps, a.warmup), extra)
    report(f"loss_fwdbwd_{P}_persons", alternate({"hip": lambda: loss_and_grads(h, y, epoch, S, args), "torch": torch_fwdbwd}, a.reps, a.warmup), extra)


def part_roofline(a, P=256, B=32, G=32, calls=50):
    args, epoch = lo.default_args(), lo.DEFAULTS["start_2d_epoch"]
    h, y = inputs(P, B, G)
    pr = _Prepared(h, y, epoch, S, args)
    pr.forward()
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    ws = torch.empty(L.mhmr_loss_workspace_bytes() // 8, dtype=torch.float64, device=DEV)
    grads = {n: torch.empty_like(t) for n, t in pr.hat.items()}
    g = _lib.LossGrads()
    for n, t in grads.items():
        setattr(g, n, t.data_ptr())
    one = torch.ones(1, device=DEV)
    fwd = lambda: _lib.check(L.mhmr_loss_forward(C.byref(pr.desc), ws.data_ptr(), ws.numel() * 8, pr.out.data_ptr(), stream), "forward")
    bwd = lambda: _lib.check(L.mhmr_loss_backward(C.byref(pr.desc), pr.out.data_ptr(), one.data_ptr(), C.byref(g), stream), "backward")
    big = sum(pr.hat[k].numel() for k in ("j3d", "v3d", "j2d", "v2d")) * 4
    for name, fn, nbytes in (("forward", fwd, 2 * big), ("backward", bwd, 3 * big)):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / calls)
        floor = nbytes / HBM_BYTES_PER_S * 1e6
        med = float(np.median(us))
        print(json.dumps(dict(part=f"loss_{name}_roofline_{P}_persons", bytes=nbytes, hbm_floor_us=round(floor, 2), median_us=round(med, 2),
                              best_us=round(min(us), 2), worst_us=round(max(us), 2), fraction_of_hbm_roofline=round(floor / med, 3),
                              note=f"{calls} back-to-back calls of the C entry between two device events")), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench measures on the GPU; there is none here")
    part_compare(256, 32, 32, a)
    part_compare(1, 1, 32, a)
    part_roofline(a)
