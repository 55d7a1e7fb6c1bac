"""Time the decoder stack's forward + backward (anny_hph.HPH.differentiable: mhmr_xattn_layers_forward / mhmr_xattn_layers_backward) against
the same computation in torch ops with autograd on the same GPU (oracle/anny_hph_ref.forward on device tensors), in the Multi-HMR
configuration (dim 1024, 8 heads, mlp 1024, depth 2): 256 persons over 32 images of N = 4096 context tokens, and 1 person in 1 image.
  fwd_bwd   forward + backward of sum(cotangent * output) with respect to the queries and every parameter, the two forms timed alternately
            (--reps repetitions after --warmup); a time is a host clock around the call ending in a device synchronise.  "faster" is true
            only if this path's worst repetition beats the torch path's best.
  to_kv     mhmr_grad_ctx_gemm alone (the to_kv gradient: [2 inner, Kc] = dkv^T ctx16 over B N rows) by device events against its floor,
            2 * 2 inner * Kc * rows FLOP over the 155 TFLOP/s of the fp32 MFMA, computed here from the shapes.
One JSON line per measurement, printed and written to --out (default profiles/hph_bwd_bench.txt).
  python tools/hph_bwd_bench.py [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from multi_hmr_amd import _lib  # noqa: E402
from multi_hmr_amd.anny_hph import HPH  # noqa: E402
from oracle import anny_hph_ref  # noqa: E402
from eval_bench import DEV, alternate, report  # noqa: E402

DIM, HEADS, MLP, DEPTH = 1024, 8, 1024, 2
FP32_MFMA_FLOPS = 155e12


def stack_part(counts, N, a, lines):
    sd, x, context, mask = anny_hph_ref.make_case(seed=3, dim=DIM, depth=DEPTH, heads=HEADS, mlp=MLP, counts=counts, N=N)
    m = HPH(dim=DIM, depth=DEPTH, heads=HEADS, dim_head=32, mlp_dim=MLP, precision="f16")
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    for p in m.parameters():
        p.requires_grad_(True)
    x, context, mask = x.to(DEV), context.to(DEV), mask.to(DEV)
    cot = torch.randn(x.shape, generator=torch.Generator().manual_seed(4)).to(DEV) * mask[:, :, None]
    # the torch form sees the operands the kernels see: the context and to_kv.weight rounded to fp16
    tsd = {k: (v.half().float() if ".1.fn.to_kv." in k else v).to(DEV).requires_grad_() for k, v in sd.items()}
    tctx = context.half().float()
    xh, xt = x.clone().requires_grad_(), x.clone().requires_grad_()

    def hip():
        xh.grad = None
        for p in m.parameters():
            p.grad = None
        (m.differentiable(xh, context, mask) * cot).sum().backward()
        return xh.grad

    def ref():
        xt.grad = None
        for v in tsd.values():
            v.grad = None
        (anny_hph_ref.forward(tsd, xt, tctx, mask, depth=DEPTH, heads=HEADS) * cot).sum().backward()
        return xt.grad
    gh, gt = hip(), ref()
    diff = float((gh - gt).abs().max() / gt.abs().max())
    P = int(sum(counts))
    lines.append(report(f"hph_stack_fwd_bwd_{P}", alternate({"hip": hip, "torch": ref}, a.reps, a.warmup),
                        dict(persons=P, images=len(counts), N=N, max_rel_diff_of_g_x_between_forms=diff)))


def to_kv_part(rows, a, lines):
    L, Nn, Kc = _lib.lib(), 64 * HEADS, 1152
    G = torch.randn(rows, Nn, device=DEV)
    ctx = torch.randn(rows, Kc, device=DEV).half()
    dW = torch.empty(Nn, Kc, device=DEV)
    nbytes = int(L.mhmr_grad_ctx_gemm_workspace_bytes(rows, Nn, Kc))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: _lib.check(L.mhmr_grad_ctx_gemm(G.data_ptr(), Nn, ctx.data_ptr(), Kc, dW.data_ptr(), rows, Nn, Kc, 1024 + 99, _lib.DT_F16,
                                                   ws.data_ptr(), nbytes, stream), "mhmr_grad_ctx_gemm")
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    flop = 2.0 * Nn * Kc * rows
    floor_ms = flop / FP32_MFMA_FLOPS * 1e3
    lines.append(report(f"to_kv_gradient_{rows}_rows", {"hip": ms}, dict(rows=rows, Nn=Nn, Kc=Kc, gflop=round(flop / 1e9, 2), fp32_mfma_floor_ms=round(floor_ms, 4),
                                                                         fraction_of_floor=round(floor_ms / float(np.median(ms)), 4),
                                                                         note="two launches (row slices + finishing pass) by device events")))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hph_bwd_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hph_bwd_bench measures on the GPU; there is none here")
    lines = []
    stack_part((8,) * 32, 4096, a, lines)
    stack_part((1,), 4096, a, lines)
    to_kv_part(32 * 4096, a, lines)
    with open(a.out, "w") as f:
        f.write("# tools/hph_bwd_bench.py: decoder stack forward + backward, HIP against torch ops on the same GPU; to_kv gradient against its fp32 MFMA floor\n")
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
