"""Time the backward of the last backbone block next to the forward of the same run, by device events, medians
of alternating repetitions after warm-up.  Per configuration -- ViT-L 896^2 with 8 and 32 images, ViT-S 672^2 with 16 --
  tape            mhmr_attention_f32_tape on random (Q | K | V) of the configuration's shape
  attention_bwd   mhmr_attention_f32_backward on the same operands
  block_bwd       mhmr_vit_block_backward (tape + backward) on a random block and stream
  forward         Model.forward in training mode (the inference kernels; no gradient)
  train_step      Model.forward(train_backbone=True) with n = 1 + backward of a random-cotangent scalar on the scores: the tap, the feature
                  cotangent of the detector, the final norm and one block
The attention lines carry the fraction of the 155 TFLOP/s fp32 matrix rate that their useful products reach (tape 4 T^2 64 per head and
image, backward 14 T^2 64: seven products, of which the kernels compute nine -- S and dP twice in the query pass).
One JSON line per measurement, printed and appended to --out (default profiles/backbone_bwd_bench.txt).
--embed: instead, one line per configuration for the backward of the token embedding
  embed_bwd       mhmr_vit_embed_backward through backbone_train.embed_backward, stored table 37 x 37
appended to --embed-out (default profiles/embed_bwd_bench.txt).
--precision bf16 (default f32 = the lines above, unchanged): block_bwd is timed in BOTH forms, alternating inside
every repetition (block_bwd = f32, block_bwd_bf16), a line `linears_bf16` times the twelve products of a block (four linears x forward,
input side, weight side, conversions included) on the bf16 entries with their rate against the dense bf16 peak, and the model's
train_step runs with train_backbone_(1, precision="bf16").  Default --out is then profiles/backbone_bwd_bench_bf16.txt.
--attention bf16 (default f32 = the lines above, unchanged): per configuration a line `attention_bf16` with the
tape and the attention backward in BOTH forms (mhmr_attention_f32_* and mhmr_attention_bf16_*, alternating inside every repetition, the
wrappers' workspace allocation inside the bracket) and a line `block_backward_bf16_attention` with the block in three forms, alternating:
block_bwd (f32), block_bwd_bf16 (bf16 linears) and block_bwd_bf16_attention (bf16 linears and bf16 attention), with the three workspace
sizes; the model's train_step runs with train_backbone_(1, precision=--precision, attention="bf16").  Default --out is then
profiles/backbone_bwd_bench_bf16_attention.txt.
  python tools/backbone_bwd_bench.py [--config all|vitl_896_8|vitl_896_32|vits_672_16] [--reps 3] [--warmup 1] [--skip-model] [--embed]
                                     [--precision f32|bf16] [--attention f32|bf16]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import synthetic  # noqa: E402
from multi_hmr_amd import Model, _lib, backbone_train as bt  # noqa: E402
from multi_hmr_amd.constants import VIT_CFG  # noqa: E402
from eval_bench import DEV, report  # noqa: E402

FP32_MFMA_FLOPS = 155e12
BF16_MFMA_FLOPS = 2.5e15            # dense bf16 matrix peak of the MI355X
CONFIGS = {"vitl_896_8": ("dinov2_vitl14", 896, 8), "vitl_896_32": ("dinov2_vitl14", 896, 32), "vits_672_16": ("dinov2_vits14", 672, 16)}


def timed(forms, a):
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
    return ms


def kernels(name, backbone, S, B, a):
    Cd, H = VIT_CFG[backbone]["embed_dim"], VIT_CFG[backbone]["num_heads"]
    T = (S // 14) ** 2 + 1
    Tp = (T + 63) // 64 * 64
    M = B * Tp
    g = torch.Generator(device=DEV).manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    shape = dict(config=name, backbone=backbone, size=S, images=B, T=T, Tp=Tp, C=Cd, H=H)
    qkv, dO = rn(M, 3 * Cd), rn(M, Cd)
    qkv[:, :Cd] *= 2.0
    if a.attention == "bf16":
        return attention_bf16_lines(shape, qkv, dO, rn, a)
    out32, lse = bt.attention_tape(qkv, B, T, Tp, H)
    dqkv = torch.empty(M, 3 * Cd, device=DEV)
    ms = timed({"tape": lambda: bt.attention_tape(qkv, B, T, Tp, H),
                "attention_bwd": lambda: bt.attention_backward(qkv, out32, lse, dO, B, T, Tp, H, dqkv=dqkv)}, a)
    unit = float(B) * H * T * T * 64
    med = lambda v: sorted(v)[len(v) // 2]
    lines = [report("attention", ms, dict(shape, tape_gflop=round(4 * unit / 1e9, 1), backward_gflop=round(14 * unit / 1e9, 1),
                                          tape_fraction_of_fp32_mfma_peak=round(4 * unit / FP32_MFMA_FLOPS / (med(ms["tape"]) * 1e-3), 4),
                                          backward_fraction_of_fp32_mfma_peak=round(14 * unit / FP32_MFMA_FLOPS / (med(ms["attention_bwd"]) * 1e-3), 4)))]
    del qkv, dO, out32, lse, dqkv
    params = dict(ln1_w=1 + 0.1 * rn(Cd), ln1_b=0.1 * rn(Cd), qkv_w=rn(3 * Cd, Cd) * Cd ** -0.5, qkv_b=0.1 * rn(3 * Cd), proj_w=rn(Cd, Cd) * Cd ** -0.5,
                  proj_b=0.1 * rn(Cd), ls1=0.5 + 0.1 * rn(Cd), ln2_w=1 + 0.1 * rn(Cd), ln2_b=0.1 * rn(Cd), fc1_w=rn(4 * Cd, Cd) * Cd ** -0.5,
                  fc1_b=0.1 * rn(4 * Cd), fc2_w=rn(Cd, 4 * Cd) * (4 * Cd) ** -0.5, fc2_b=0.1 * rn(Cd), ls2=0.5 + 0.1 * rn(Cd))
    x_in, g_out = rn(M, Cd), rn(M, Cd)
    forms = {"block_bwd": lambda: bt.block_backward(params, x_in, g_out, B, T, Tp, H)}
    if a.precision == "bf16":
        forms["block_bwd_bf16"] = lambda: bt.block_backward(params, x_in, g_out, B, T, Tp, H, precision="bf16")
    ms = timed(forms, a)
    lin = 3 * 2.0 * M * 12 * Cd * Cd                       # tape, input side and weight side of the four linears
    if a.precision == "bf16":
        lines.append(linears_bf16(shape, params, M, Cd, lin, a))
        lines.append(report("block_backward_bf16", ms, dict(shape, workspace_bytes=int(_lib.lib().mhmr_vit_block_backward_workspace_bytes_p(B, Tp, Cd, 1)),
                                                            workspace_bytes_f32=int(_lib.lib().mhmr_vit_block_backward_workspace_bytes(B, Tp, Cd)),
                                                            linear_gflop=round(lin / 1e9, 1), attention_gflop=round(18 * unit / 1e9, 1),
                                                            median_ratio_f32_over_bf16=round(med(ms["block_bwd"]) / med(ms["block_bwd_bf16"]), 2),
                                                            note="tape + backward in both forms, alternating; attention, LayerNorm and the column "
                                                                 "sums are the fp32 kernels in both")))
        return lines
    lines.append(report("block_backward", ms, dict(shape, workspace_bytes=int(_lib.lib().mhmr_vit_block_backward_workspace_bytes(B, Tp, Cd)),
                                                   linear_gflop=round(lin / 1e9, 1), attention_gflop=round(18 * unit / 1e9, 1),
                                                   fraction_of_fp32_mfma_peak=round((lin + 18 * unit) / FP32_MFMA_FLOPS / (med(ms["block_bwd"]) * 1e-3), 4),
                                                   note="tape + backward; the linears run on the person head's fp32 kernels (16-row tiles)")))
    return lines


def block_params(rn, Cd):
    return dict(ln1_w=1 + 0.1 * rn(Cd), ln1_b=0.1 * rn(Cd), qkv_w=rn(3 * Cd, Cd) * Cd ** -0.5, qkv_b=0.1 * rn(3 * Cd), proj_w=rn(Cd, Cd) * Cd ** -0.5,
                proj_b=0.1 * rn(Cd), ls1=0.5 + 0.1 * rn(Cd), ln2_w=1 + 0.1 * rn(Cd), ln2_b=0.1 * rn(Cd), fc1_w=rn(4 * Cd, Cd) * Cd ** -0.5,
                fc1_b=0.1 * rn(4 * Cd), fc2_w=rn(Cd, 4 * Cd) * (4 * Cd) ** -0.5, fc2_b=0.1 * rn(Cd), ls2=0.5 + 0.1 * rn(Cd))


def attention_bf16_lines(shape, qkv, dO, rn, a):
    """The attention pair and the block with and without bf16-operand attention, the forms alternating."""
    L = _lib.lib()
    B, T, Tp, Cd, H = shape["images"], shape["T"], shape["Tp"], shape["C"], shape["H"]
    M = B * Tp
    med = lambda v: sorted(v)[len(v) // 2]
    o32, l32 = bt.attention_tape(qkv, B, T, Tp, H)
    o16, l16 = bt.attention_bf16_tape(qkv, B, T, Tp, H)
    dqkv = torch.empty(M, 3 * Cd, device=DEV)
    ms = timed({"tape": lambda: bt.attention_tape(qkv, B, T, Tp, H), "tape_bf16": lambda: bt.attention_bf16_tape(qkv, B, T, Tp, H),
                "attention_bwd": lambda: bt.attention_backward(qkv, o32, l32, dO, B, T, Tp, H, dqkv=dqkv),
                "attention_bwd_bf16": lambda: bt.attention_bf16_backward(qkv, o16, l16, dO, B, T, Tp, H, dqkv=dqkv)}, a)
    unit = float(B) * H * T * T * 64
    lines = [report("attention_bf16", ms, dict(shape, tape_gflop=round(6 * unit / 1e9, 1), backward_gflop=round(18 * unit / 1e9, 1),
                                               workspace_bytes=int(L.mhmr_attention_bf16_workspace_bytes(B, Tp, Cd, H)),
                                               workspace_bytes_f32=int(L.mhmr_attention_f32_backward_workspace_bytes(B, Tp, H)),
                                               tape_bf16_tflops=round(6 * unit / (med(ms["tape_bf16"]) * 1e-3) / 1e12, 1),
                                               backward_bf16_tflops=round(18 * unit / (med(ms["attention_bwd_bf16"]) * 1e-3) / 1e12, 1),
                                               median_ratio_tape_f32_over_bf16=round(med(ms["tape"]) / med(ms["tape_bf16"]), 2),
                                               median_ratio_backward_f32_over_bf16=round(med(ms["attention_bwd"]) / med(ms["attention_bwd_bf16"]), 2),
                                               note="the bf16 flop counts are the products the kernels compute (the tape S twice, the backward S and "
                                                    "dP twice); its times include the fp32 -> bf16 conversions"))]
    del o32, l32, o16, l16, dqkv
    params = block_params(rn, Cd)
    x_in, g_out = rn(M, Cd), rn(M, Cd)
    ms = timed({"block_bwd": lambda: bt.block_backward(params, x_in, g_out, B, T, Tp, H),
                "block_bwd_bf16": lambda: bt.block_backward(params, x_in, g_out, B, T, Tp, H, precision="bf16"),
                "block_bwd_bf16_attention": lambda: bt.block_backward(params, x_in, g_out, B, T, Tp, H, precision="bf16", attention="bf16")}, a)
    wsb = L.mhmr_vit_block_backward_workspace_bytes_pa
    lines.append(report("block_backward_bf16_attention", ms, dict(
        shape, workspace_bytes_f32=int(wsb(B, Tp, Cd, 0, 0)), workspace_bytes_bf16=int(wsb(B, Tp, Cd, 1, 0)), workspace_bytes=int(wsb(B, Tp, Cd, 1, 1)),
        median_ratio_bf16_over_bf16_attention=round(med(ms["block_bwd_bf16"]) / med(ms["block_bwd_bf16_attention"]), 2),
        median_ratio_f32_over_bf16_attention=round(med(ms["block_bwd"]) / med(ms["block_bwd_bf16_attention"]), 2),
        note="tape + backward in three forms, alternating: exact fp32, bf16 linears, bf16 linears and bf16 attention")))
    return lines


def linears_bf16(shape, params, M, Cd, lin_flop, a):
    """The twelve products of a block on the bf16 entries (conversions included), preallocated operands and workspace."""
    L = _lib.lib()
    g = torch.Generator(device=DEV).manual_seed(6)
    act = torch.randn(M, 4 * Cd, generator=g, device=DEV)       # every activation / cotangent is a view of these two
    cot = torch.randn(M, 4 * Cd, generator=g, device=DEV)
    out = torch.empty(M, 4 * Cd, device=DEV)
    dW, db = torch.empty(4 * Cd * Cd, device=DEV), torch.empty(4 * Cd, device=DEV)
    nbytes = int(L.mhmr_linear_bf16_workspace_bytes(M, 4 * Cd, Cd))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    s = lambda: torch.cuda.current_stream().cuda_stream
    shapes = [("qkv_w", 3 * Cd, Cd), ("proj_w", Cd, Cd), ("fc1_w", 4 * Cd, Cd), ("fc2_w", Cd, 4 * Cd)]

    def run():
        for f, N, K in shapes:
            W = params[f]
            _lib.check(L.mhmr_linear_bf16(act.data_ptr(), 4 * Cd, W.data_ptr(), K, None, out.data_ptr(), 4 * Cd, M, N, K, ws.data_ptr(), nbytes, s()), f)
            _lib.check(L.mhmr_linear_bf16_backward_input(cot.data_ptr(), 4 * Cd, W.data_ptr(), K, None, 0, out.data_ptr(), 4 * Cd, M, N, K, ws.data_ptr(),
                                                         nbytes, s()), f)
            _lib.check(L.mhmr_linear_bf16_backward_weight(cot.data_ptr(), 4 * Cd, act.data_ptr(), 4 * Cd, dW.data_ptr(), K, db.data_ptr(), M, N, K,
                                                          ws.data_ptr(), nbytes, s()), f)
    ms = timed({"linears_bf16": run}, a)
    t = sorted(ms["linears_bf16"])[len(ms["linears_bf16"]) // 2] * 1e-3
    return report("linears_bf16", ms, dict(shape, linear_gflop=round(lin_flop / 1e9, 1), tflops=round(lin_flop / t / 1e12, 1),
                                           fraction_of_bf16_mfma_peak=round(lin_flop / BF16_MFMA_FLOPS / t, 4), workspace_bytes=nbytes,
                                           note="4 linears x (forward, input side, weight side + bias sums), fp32 -> bf16 conversions included"))


def embed(name, backbone, S, B, a):
    """mhmr_vit_embed_backward on a random image batch and stream cotangent of the configuration's shape."""
    Cd, G = VIT_CFG[backbone]["embed_dim"], S // 14
    Tp = (G * G + 1 + 63) // 64 * 64
    g = torch.Generator(device=DEV).manual_seed(4)
    x, gs = torch.randn(B, 3, S, S, generator=g, device=DEV) + 0.5, torch.randn(B * Tp, Cd, generator=g, device=DEV)
    ms = timed({"embed_bwd": lambda: bt.embed_backward(x, gs, B, G, 37, Tp)}, a)
    med = sorted(ms["embed_bwd"])[len(ms["embed_bwd"]) // 2]
    flop = 2.0 * B * G * G * Cd * 588
    return [report("embed_backward", ms, dict(config=name, backbone=backbone, size=S, images=B, G=G, M=37, Tp=Tp, C=Cd, patch_weight_gflop=round(flop / 1e9, 1),
                                              workspace_bytes=int(_lib.lib().mhmr_vit_embed_backward_workspace_bytes(B, G, 37, Cd)),
                                              fraction_of_fp32_mfma_peak=round(flop / FP32_MFMA_FLOPS / (med * 1e-3), 4),
                                              note="one call: g_patch_w (fp32 MFMA chain, image gathered), g_patch_b, g_cls, g_pos (fp64); the wrapper's "
                                                   "allocations and the upload of the resampling matrix are inside the bracket"))]


def model_level(name, backbone, S, B, a):
    smplx_data, mean_params = synthetic.make_smplx_data(0), synthetic.make_mean_params(0)
    m = Model(backbone=backbone, img_size=S, smplx_data=smplx_data, mean_params=mean_params, precision="f16")
    m.load_state_dict(synthetic.make_state_dict(backbone, S, seed=0, mean_params=mean_params), strict=True)
    m = m.to(DEV).eval().train_backbone_(1, precision=a.precision, attention=a.attention)
    G = S // 14
    x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(0)).to(DEV)
    K = synthetic.get_camera_K(S, B).to(DEV)
    idx = tuple(t.to(DEV) for t in synthetic.make_pinned_idx(B, G, 1, seed=0))
    cs = torch.randn(B, G, G, 1, generator=torch.Generator(device=DEV).manual_seed(5), device=DEV)

    def step():
        for p in m.backbone_parameters(1):
            p.grad = None
        out = m(x, idx=idx, K=K, is_training=True, train_backbone=True)
        (out["scores"] * cs).sum().backward()
    ms = timed({"forward": lambda: m(x, idx=idx, K=K, is_training=True), "train_step": step}, a)
    med = lambda v: sorted(v)[len(v) // 2]
    return [report("model", ms, dict(config=name, backbone=backbone, size=S, images=B, dtype=m.packed_precision, trainable_blocks=1,
                                     **({"backward_precision": a.precision} if a.precision != "f32" else {}),
                                     **({"backward_attention": a.attention} if a.attention != "f32" else {}),
                                     image_blocks=m._nsplit(B), median_ratio_train_step_over_forward=round(med(ms["train_step"]) / med(ms["forward"]), 2),
                                     note="train_step = the forward with the tap + backward of a random-cotangent scalar on the scores (detector's "
                                          "feature cotangent, final norm, one block); no optimiser step, no re-pack"))]


def main(a):
    names = list(CONFIGS) if a.config == "all" else [a.config]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.embed:                                              # the embedding backward alone, into a file of its own
        with open(a.embed_out, "a") as fh:
            fh.write("# tools/backbone_bwd_bench.py --embed: mhmr_vit_embed_backward through backbone_train.embed_backward\n")
            for name in names:
                for line in embed(name, *CONFIGS[name], a):
                    fh.write(json.dumps(line) + "\n")
        return
    with open(a.out, "a") as fh:
        fh.write("# tools/backbone_bwd_bench.py: attention tape / backward, block backward and a train_backbone step next to the forward\n")
        for name in names:
            backbone, S, B = CONFIGS[name]
            for line in kernels(name, backbone, S, B, a) + ([] if a.skip_model else model_level(name, backbone, S, B, a)):
                fh.write(json.dumps(line) + "\n")
                fh.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="all", choices=["all"] + list(CONFIGS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--precision", default="f32", choices=["f32", "bf16"], help="bf16: also time the bf16-operand form (section 30)")
    ap.add_argument("--attention", default="f32", choices=["f32", "bf16"], help="bf16: time the bf16-operand attention next to the others (section 31)")
    ap.add_argument("--out", default=None, help="default profiles/backbone_bwd_bench.txt (profiles/backbone_bwd_bench_bf16.txt with --precision bf16, "
                                                "profiles/backbone_bwd_bench_bf16_attention.txt with --attention bf16)")
    ap.add_argument("--embed", action="store_true", help="time the embedding backward (section 29) instead, appended to --embed-out")
    ap.add_argument("--embed-out", default=os.path.join(ROOT, "profiles", "embed_bwd_bench.txt"))
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "backbone_bwd_bench_bf16_attention.txt" if a.attention == "bf16" else
                             "backbone_bwd_bench_bf16.txt" if a.precision == "bf16" else "backbone_bwd_bench.txt")
    if not torch.cuda.is_available():
        raise SystemExit("backbone_bwd_bench measures on the GPU; there is none here")
    main(a)
