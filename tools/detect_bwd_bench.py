"""Time the backward of the detection head mlp_classif at the headline shape (rows = 32 x 4096 = 131072 context rows, C = 1024, f16), three
paths by device events, alternating repetitions after warm-up:
  fused        mhmr_detect_backward: row pass, fp64 column sums, the dW1 product with its left operand formed in registers (no [rows, C]
               fp32 array: 72 MB of workspace)
  materialise  the comparison path: dl and the hidden layer's cotangent dhid [rows, C] fp32 (512 MB) by torch ops, mhmr_grad_ctx_gemm on it
               for dW1, torch column sums for db1, dw2, db2
  torch        torch autograd of the same two layers on device tensors (fp32 X = the 16-bit context's values, fp32 matmuls): forward +
               backward, as autograd needs both
"faster" follows the project's convention: true only if the fused path's worst repetition beats the other path's best.  The fused path's
fraction of the fp32 MFMA peak is taken against the floor of the dW1 product alone, 2 C C rows FLOP (275 GFLOP) over 155 TFLOP/s.
One JSON line per measurement, printed and written to --out (default profiles/detect_bwd_bench.txt).
  python tools/detect_bwd_bench.py [--reps 10] [--warmup 2] [--rows 131072] [--C 1024]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from multi_hmr_amd import _lib, detect_train  # noqa: E402
from eval_bench import DEV, report  # noqa: E402

FP32_MFMA_FLOPS = 155e12          # the peak tools/hph_bwd_bench.py uses for the to_kv gradient


def main(a):
    L, rows, C_, Kc = _lib.lib(), a.rows, a.C, a.C + 128
    g = torch.Generator(device=DEV).manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    ctx16 = rn(rows, Kc).half()
    W1, b1 = (rn(C_, C_) * C_ ** -0.5).half().float(), rn(C_) * 0.1
    w2, b2, gs = rn(C_) * C_ ** -0.5, rn(1) * 0.2, rn(rows)
    X = ctx16[:, :C_].float()
    hid16 = torch.relu(X @ W1.T + b1).half()
    stream = torch.cuda.current_stream().cuda_stream
    out = {}

    def fused():
        out["fused"] = detect_train.detect_backward(hid16, ctx16, w2, b2, gs, rows, C_, True, _lib.DT_F16, stream)

    nb_mat = int(L.mhmr_grad_ctx_gemm_workspace_bytes(rows, C_, C_))
    ws_mat = torch.empty(nb_mat, dtype=torch.uint8, device=DEV)

    def materialise():
        h = hid16.float()
        p = torch.sigmoid(h @ w2 + b2)
        dl = torch.where((p >= 1e-4) & (p <= 1 - 1e-4), gs * p * (1 - p), torch.zeros((), device=DEV))
        mask = hid16 > 0
        dhid = (dl[:, None] * w2[None, :]) * mask                      # [rows, C] fp32: what the fused path never stores
        dW1 = torch.empty(C_, C_, device=DEV)
        _lib.check(L.mhmr_grad_ctx_gemm(dhid.data_ptr(), C_, ctx16.data_ptr(), Kc, dW1.data_ptr(), rows, C_, C_, C_, _lib.DT_F16, ws_mat.data_ptr(),
                                        nb_mat, stream), "mhmr_grad_ctx_gemm")
        out["materialise"] = (dW1, dhid.sum(0), dl @ h, dl.sum().reshape(1))

    leaves = [t.clone().requires_grad_() for t in (W1, b1, w2, b2)]

    def torch_autograd():
        hid = torch.relu(X @ leaves[0].T + leaves[1])
        p = torch.clamp(torch.sigmoid(hid @ leaves[2] + leaves[3]), 1e-4, 1 - 1e-4)
        out["torch"] = torch.autograd.grad((p * gs).sum(), leaves)

    forms = {"fused": fused, "materialise": materialise, "torch": torch_autograd}
    ms = {k: [] for k in forms}
    for r in range(a.warmup + a.reps):
        for name, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    rel = lambda x, y: float((x.reshape(-1) - y.reshape(-1)).abs().max() / y.abs().max())
    diffs = {f"max_rel_diff_{n}_fused_vs_{k}": rel(out["fused"][i], out[k][i]) for k in ("materialise", "torch")
             for i, n in enumerate(("dW1", "db1", "dw2", "db2"))}
    flop = 2.0 * C_ * C_ * rows
    floor_ms = flop / FP32_MFMA_FLOPS * 1e3
    med = float(np.median(ms["fused"]))
    extra = dict(rows=rows, C=C_, dtype="f16", gflop_dW1=round(flop / 1e9, 2), fp32_mfma_floor_ms=round(floor_ms, 4),
                 fused_fraction_of_fp32_mfma_peak=round(floor_ms / med, 4),
                 fused_workspace_bytes=int(L.mhmr_detect_backward_workspace_bytes(rows, C_)), materialised_cotangent_bytes=rows * C_ * 4,
                 fused_faster_than_materialise=bool(max(ms["fused"]) < min(ms["materialise"])),
                 fused_faster_than_torch=bool(max(ms["fused"]) < min(ms["torch"])), **diffs,
                 note="device events around each path; fused = 5 launches; torch = forward + backward of the two layers")
    line = report(f"detect_backward_{rows}_rows", ms, extra)
    with open(a.out, "w") as f:
        f.write("# tools/detect_bwd_bench.py: backward of mlp_classif, fused (mhmr_detect_backward) against materialise-then-mhmr_grad_ctx_gemm and torch autograd\n")
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=32 * 4096)
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_bwd_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detect_bwd_bench measures on the GPU; there is none here")
    main(a)
