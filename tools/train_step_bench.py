"""Time the tail of the training step at the headline shape: ViT-L 896^2, 32 images, 8 persons per image, f16, from
stored features.  One process, one model, two optimisers over the same parameters, alternating repetitions after warm-up; device events
and medians as tools/feature_grad_bench.py takes them, plus the host's wall time to issue each form (before any synchronisation).
  step    forward_features + backward of a random-cotangent scalar on read-out, offset and scores (train_heads and train_detection on), then
          torch.optim.Adam.step() + Model.repack_heads()   against   HeadsAdam.step()
  tail    the parts alone, gradients already in place: torch.optim.Adam.step(), Model.repack_heads(), HeadsAdam.step(), and the C entry
          mhmr_adam_step by itself on the table the last step left
The bytes HeadsAdam.step() moves come from its segment table (multi_hmr_amd.optim.table_bytes); the achieved fraction of the HBM rate is
bytes / median time / 8 TB/s.
  python tools/train_step_bench.py [--reps 10] [--warmup 2] [--images 32] [--persons 8] [--backbone dinov2_vitl14] [--size 896]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import synthetic  # noqa: E402
from multi_hmr_amd import HeadsAdam, Model, _lib  # noqa: E402
from multi_hmr_amd.optim import table_bytes  # noqa: E402
from eval_bench import DEV, report  # noqa: E402

HBM_BYTES_PER_S = 8.0e12          # MI355X: 8 TB/s


def timed(forms, a, setup=None):
    """-> ({name: [device ms]}, {name: [host ms to issue]}) of each form's callable, alternating; ``setup()`` (untimed) runs before each."""
    ms, host = {k: [] for k in forms}, {k: [] for k in forms}
    for r in range(a.warmup + a.reps):
        for name, fn in forms.items():
            if setup:
                setup()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
                host[name].append((t1 - t0) * 1e3)
    return ms, host


def main(a):
    S, B, q = a.size, a.images, a.persons
    smplx_data, mean_params = synthetic.make_smplx_data(0), synthetic.make_mean_params(0)
    m = Model(backbone=a.backbone, img_size=S, smplx_data=smplx_data, mean_params=mean_params, precision="f16")
    m.load_state_dict(synthetic.make_state_dict(a.backbone, S, seed=0, mean_params=mean_params), strict=True)
    m = m.to(DEV).eval().train_heads_(True).train_detection_(True)
    G = S // 14
    x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(0)).to(DEV)
    K = synthetic.get_camera_K(S, B).to(DEV)
    idx = tuple(t.to(DEV) for t in synthetic.make_pinned_idx(B, G, q, seed=0))
    Pn = int(idx[0].shape[0])
    g = torch.Generator(device=DEV).manual_seed(11)
    cr = torch.randn(Pn, 318 + m.num_betas + 13, generator=g, device=DEV)
    co, cs = torch.randn(Pn, 2, generator=g, device=DEV), torch.randn(B, G, G, 1, generator=g, device=DEV)
    f = m.backbone_features(x).clone()
    del x
    kw = dict(idx=idx, K=K, is_training=True, return_readout=True, train_heads=True, train_detection=True)
    params = m.heads_parameters() + m.detection_parameters()
    opt_t = torch.optim.Adam(params, lr=1e-6)
    opt_h = HeadsAdam(m, lr=1e-6)

    def grads():
        for p in params:
            p.grad = None
        out = m.forward_features(f, **kw)
        ((out["readout"] * cr).sum() + (out["offset"] * co).sum() + (out["scores"] * cs).sum()).backward()

    def step_torch():
        grads()
        opt_t.step()
        m.repack_heads()

    def step_heads_adam():
        grads()
        opt_h.step()
    shape = dict(backbone=a.backbone, size=S, images=B, persons=Pn, dtype=m.packed_precision, parameters=len(params),
                 elements=int(sum(p.numel() for p in params)))
    ms, host = timed({"torch_adam_plus_repack_heads": step_torch, "heads_adam": step_heads_adam}, a)
    med = lambda v: float(np.median(v))
    lines = [report("training_step_from_stored_features", ms, dict(
        shape, host_issue_ms={k: round(med(v), 4) for k, v in host.items()},
        median_ratio_torch_over_heads_adam=round(med(ms["torch_adam_plus_repack_heads"]) / med(ms["heads_adam"]), 3),
        heads_adam_faster=bool(max(ms["heads_adam"]) < min(ms["torch_adam_plus_repack_heads"])),
        note="forward_features + backward of a random-cotangent scalar + the optimiser tail; no decode_readout or loss (the same in both)"))]
    tab = opt_h._table
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def kernel_alone():      # the launch of the last HeadsAdam.step() again: its table is on the device and its gradients are still alive
        _lib.check(L.mhmr_adam_step(tab["host"], tab["device"].data_ptr(), len(tab["rows"]), 0.9, 0.999, 1e-8, 0.0, None, 0, None, stream),
                   "mhmr_adam_step")

    def setup_tail():
        grads()
        opt_h.step()         # (untimed) leaves a table whose gradient pointers are this repetition's
    ms, host = timed({"torch_adam_step": opt_t.step, "repack_heads": m.repack_heads, "heads_adam_step": opt_h.step,
                      "mhmr_adam_step_alone": kernel_alone}, a, setup=setup_tail)
    nbytes = table_bytes(opt_h._table["host"])
    t_h = med(ms["heads_adam_step"])
    lines.append(report("optimiser_tail_alone", ms, dict(
        shape, host_issue_ms={k: round(med(v), 4) for k, v in host.items()},
        torch_tail_ms=round(med(ms["torch_adam_step"]) + med(ms["repack_heads"]), 4),
        median_ratio_torch_tail_over_heads_adam=round((med(ms["torch_adam_step"]) + med(ms["repack_heads"])) / t_h, 3),
        heads_adam_bytes=nbytes, heads_adam_segments=len(opt_h._table["rows"]), heads_adam_chunks=opt_h._table["chunks"],
        heads_adam_fraction_of_hbm=round(nbytes / (t_h * 1e-3) / HBM_BYTES_PER_S, 4),
        kernel_alone_fraction_of_hbm=round(nbytes / (med(ms["mhmr_adam_step_alone"]) * 1e-3) / HBM_BYTES_PER_S, 4),
        note="gradients in place before the first event; heads_adam_step is the whole Python call (table fill, the 120-byte-per-segment "
             "table copy, the launch); mhmr_adam_step_alone is the C entry on the table that call left")))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("# tools/train_step_bench.py: the training step from stored features with torch.optim.Adam + repack_heads() against HeadsAdam, "
                 "and the optimiser tail alone\n")
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--persons", type=int, default=8)
    ap.add_argument("--backbone", default="dinov2_vitl14")
    ap.add_argument("--size", type=int, default=896)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_bench measures on the GPU; there is none here")
    main(a)
