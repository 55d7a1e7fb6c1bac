"""Time the heads-from-stored-features path at the headline shape: ViT-L 896^2, 32 images (131072 context rows,
C = 1024), 8 persons per image, f16; device events, medians, alternating repetitions after warm-up.  Three parts, one JSON line each:
  product       mhmr_rows_times_weight alone at the two shapes the backward uses -- n = 512 (to_kv16 of one decoder layer) and n = 1024 (the
                detector) -- and mhmr_detect_feature_grad (the same product with its left operand formed in registers, plus the row pass),
                each against its fp32-MFMA floor 2 rows n C FLOP over 155 TFLOP/s
  backwards     ``backward()`` of the heads' node (read-out and offset cotangents) and of the detector's node (scores cotangent) through
                Model.forward_features, without and with ``features.requires_grad`` (the g_feat outputs)
  step          one training step (forward + backward of a random-cotangent scalar on read-out, offset and scores, train_heads and
                train_detection on) from images (Model.forward) against one from stored features (Model.forward_features); decode_readout
                and the loss are the same work in both and are left out
  python tools/feature_grad_bench.py [--reps 10] [--warmup 2] [--images 32] [--persons 8] [--backbone dinov2_vitl14] [--size 896]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import synthetic  # noqa: E402
from multi_hmr_amd import Model, _lib, detect_train  # noqa: E402
from eval_bench import DEV, report  # noqa: E402

FP32_MFMA_FLOPS = 155e12          # the measured fp32 matrix rate the other backward benches use


def timed(forms, a, setup=None):
    """{name: [ms]} of each form's callable, alternating; ``setup[name]()`` (untimed) runs first and its result is the callable's argument."""
    ms = {k: [] for k in forms}
    for r in range(a.warmup + a.reps):
        for name, fn in forms.items():
            arg = setup[name]() if setup else None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn(arg) if setup else fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    return ms


def product_part(rows, C_, a):
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=DEV).manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    out = torch.empty(rows, C_, device=DEV)
    ops = {n: (rn(rows, n), (rn(n, C_) * n ** -0.5).half()) for n in (512, C_)}
    hid16, w2, b2, gs = torch.relu(rn(rows, C_)).half(), rn(C_) * C_ ** -0.5, rn(1) * 0.2, rn(rows)
    dl_ws = torch.empty(int(L.mhmr_detect_feature_grad_workspace_bytes(rows)) // 4, device=DEV)

    def plain(n):
        left, w16 = ops[n]
        return lambda: _lib.check(L.mhmr_rows_times_weight(left.data_ptr(), n, w16.data_ptr(), C_, out.data_ptr(), C_, rows, n, C_, 0, _lib.DT_F16,
                                                           stream), "mhmr_rows_times_weight")

    def fused():
        _lib.check(L.mhmr_detect_feature_grad(hid16.data_ptr(), C_, ops[C_][1].data_ptr(), C_, w2.data_ptr(), b2.data_ptr(), gs.data_ptr(), rows, C_, 1,
                                              _lib.DT_F16, out.data_ptr(), C_, dl_ws.data_ptr(), dl_ws.numel() * 4, stream), "mhmr_detect_feature_grad")
    ms = timed({"to_kv_n512": plain(512), f"detector_n{C_}_plain": plain(C_), f"detector_n{C_}_fused": fused}, a)
    extra = dict(rows=rows, C=C_, dtype="f16")
    for name, n in (("to_kv_n512", 512), (f"detector_n{C_}_plain", C_), (f"detector_n{C_}_fused", C_)):
        floor = 2.0 * rows * n * C_ / FP32_MFMA_FLOPS * 1e3
        extra[name + "_gflop"] = round(2.0 * rows * n * C_ / 1e9, 2)
        extra[name + "_fp32_mfma_floor_ms"] = round(floor, 4)
        extra[name + "_fraction_of_fp32_mfma_peak"] = round(floor / float(np.median(ms[name])), 4)
    extra["materialised_hidden_cotangent_bytes_avoided"] = rows * C_ * 4
    return report(f"rows_times_weight_{rows}_rows", ms, extra)


def model_parts(a):
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
    kw = dict(idx=idx, K=K, is_training=True, return_readout=True, train_heads=True, train_detection=True)

    def clear():
        for p in m.parameters():
            p.grad = None

    def scalar(out, heads, detector):
        t = 0
        if heads:
            t = t + (out["readout"] * cr).sum() + (out["offset"] * co).sum()
        if detector:
            t = t + (out["scores"] * cs).sum()
        return t

    def pending(heads, detector, leaf):
        def make():
            clear()
            return scalar(m.forward_features(f.clone().requires_grad_() if leaf else f, **kw), heads, detector)
        return make
    setup = {"heads_without_g_feat": pending(True, False, False), "heads_with_g_feat": pending(True, False, True),
             "detector_without_g_feat": pending(False, True, False), "detector_with_g_feat": pending(False, True, True)}
    ms = timed({k: (lambda t: t.backward()) for k in setup}, a, setup)
    shape = dict(backbone=a.backbone, size=S, images=B, persons=Pn, rows=B * G * G, C=m.embed_dim, dtype=m.packed_precision)
    lines = [report("backwards_with_and_without_g_feat", ms, dict(
        shape, g_feat_bytes=B * G * G * m.embed_dim * 4,
        heads_g_feat_cost_ms=round(float(np.median(ms["heads_with_g_feat"]) - np.median(ms["heads_without_g_feat"])), 4),
        detector_g_feat_cost_ms=round(float(np.median(ms["detector_with_g_feat"]) - np.median(ms["detector_without_g_feat"])), 4),
        note="device events around backward() alone; the forward of each repetition runs before the first event"))]

    def step_images():
        clear()
        scalar(m(x, **kw), True, True).backward()

    def step_features():
        clear()
        scalar(m.forward_features(f, **kw), True, True).backward()

    def step_features_leaf():
        clear()
        scalar(m.forward_features(f.clone().requires_grad_(), **kw), True, True).backward()
    ms = timed({"from_images": step_images, "from_stored_features": step_features, "from_stored_features_with_features_grad": step_features_leaf}, a)
    lines.append(report("training_step", ms, dict(
        shape, median_ratio_images_over_features=round(float(np.median(ms["from_images"]) / np.median(ms["from_stored_features"])), 2),
        features_faster=bool(max(ms["from_stored_features"]) < min(ms["from_images"])),
        note="forward + backward of a random-cotangent scalar on read-out, offset and scores; train_heads and train_detection on; no "
             "decode_readout, loss or optimiser (the same in both)")))
    return lines


def main(a):
    G = a.size // 14
    lines = [product_part(a.images * G * G, synthetic.VIT_CFG[a.backbone]["embed_dim"], a)] + model_parts(a)
    with open(a.out, "w") as fh:
        fh.write("# tools/feature_grad_bench.py: heads from stored features -- the rows-times-weight product against its fp32-MFMA floor, the two "
                 "backwards without / with g_feat, a training step from images against one from stored features\n")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_grad.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_grad_bench measures on the GPU; there is none here")
    main(a)
