"""TEST INFRASTRUCTURE: the decoder layer stack restated in torch on the CPU, parametrised by dtype and differentiated by autograd -- the
reference of the backward kernels (csrc/hph_bwd.hip).  Built from oracle/anny_hph_ref.forward; on real rows that is
also the Multi-HMR decoder (tests/test_gpu_hph.py::test_layer_stack_against_fp64).  The context and to_kv.weight are rounded to the 16-bit
operand type first: the kernels take those as exact numbers.  The scalar is sum(cotangent * output) over the real rows."""
from __future__ import annotations

import torch

from oracle import anny_hph_ref

TDT = {"f16": torch.float16, "bf16": torch.bfloat16, None: None}      # None: no rounding (finite-difference checks)

#: the four stack cases of the issue: (dim, heads, mlp, depth, counts, N)
STACK_CASES = {
    "small": (256, 8, 512, 2, (9, 0, 1, 17), 256),
    "multihmr": (1024, 8, 1024, 2, (130, 0, 1, 65, 9), 256),
    "anny": (512, 16, 2048, 8, (130, 0, 1, 65, 9), 256),
    "long": (256, 8, 512, 2, (3,), 4096),
}


def stack_case(name, seed=11):
    dim, heads, mlp, depth, counts, N = STACK_CASES[name]
    sd, x, context, mask = anny_hph_ref.make_case(seed=seed, dim=dim, depth=depth, heads=heads, mlp=mlp, counts=counts, N=N)
    g = torch.Generator().manual_seed(seed + 1000)
    cot = torch.empty(x.shape).normal_(0, 1, generator=g) * mask[:, :, None]
    return dict(sd=sd, x=x, context=context, mask=mask, cot=cot, depth=depth, heads=heads, dim=dim, mlp=mlp)


def stack_operands(case, precision, dtype):
    """The numbers the kernels see, in `dtype`: fp32 weights and queries, the context and to_kv.weight rounded to the 16-bit type."""
    tdt = TDT[precision]
    rnd = (lambda v: v.to(tdt)) if tdt is not None else (lambda v: v)
    sd = {k: (rnd(v) if ".1.fn.to_kv." in k else v).to(dtype).clone() for k, v in case["sd"].items()}      # (copies: the case stays as it is)
    return sd, case["x"].to(dtype).clone(), rnd(case["context"]).to(dtype)


def stack_scalar(case, sd, x, context):
    y = anny_hph_ref.forward(sd, x, context, case["mask"].to(x.dtype), depth=case["depth"], heads=case["heads"])
    real = case["mask"].bool()
    return (case["cot"].to(x.dtype)[real] * y[real]).sum()


def stack_grads(case, precision, dtype):
    """{"x": d scalar / d x [B', nmax, dim], <state_dict key>: gradient} in `dtype`."""
    sd, x, context = stack_operands(case, precision, dtype)
    names = list(sd)
    leaves = [x.requires_grad_()] + [sd[k].requires_grad_() for k in names]
    grads = torch.autograd.grad(stack_scalar(case, sd, x, context), leaves)
    return dict(zip(["x"] + names, grads))


def four_x(got, ref64, yard32):
    """The 4x rule of DESIGN.md section 16 for one tensor: (kernel error, yardstick error, ratio, passes).  Errors are maximum absolute
    differences against fp64; the bound is 4x the error of the same computation in fp32 torch on the CPU.  A yardstick of exactly 0 (a
    sum over one row) demands the exact bits."""
    if ref64.numel() == 0:
        return 0.0, 0.0, 0.0, True
    err = float((got.double().cpu() - ref64).abs().max())
    yard = float((yard32.double() - ref64).abs().max())
    return err, yard, (err / yard if yard > 0 else float("inf") if err > 0 else 0.0), err <= 4 * yard


# ------------------------------------------------------------------------------------------------------ the whole head
def _round_st(x, tdt):
    """x rounded to the 16-bit operand type, with the straight-through gradient."""
    return x if tdt is None else x + (x.detach().to(tdt).to(x.dtype) - x.detach())


def embedd_camera(K, G, num_bands=16, max_resolution=64):
    """oracle/multihmr_ref.embedd_camera (model.py:160-187) in the dtype of K: the ROW index is fed as pixel-x, the COLUMN as pixel-y."""
    import numpy as np
    dt, bs = K.dtype, K.shape[0]
    pts = torch.stack([torch.arange(G).reshape(-1, 1).repeat(1, G), torch.arange(G).reshape(1, -1).repeat(G, 1)], -1).to(dt)
    pts = (pts * 14 + 7).reshape(1, -1, 2).repeat(bs, 1, 1)
    rays = torch.einsum("bij,bkj->bki", torch.inverse(K), torch.cat([pts, torch.ones_like(pts[..., :1])], -1))
    freq = torch.stack([torch.linspace(1.0, max_resolution / 2, num_bands, dtype=dt) for _ in range(3)], dim=0)
    feat = (rays[:, :, :, None] * freq[None, None, :, :]).reshape(bs, rays.shape[1], -1)
    return torch.cat([rays, torch.sin(np.pi * feat), torch.cos(np.pi * feat)], dim=-1).reshape(bs, G, G, 3 + 6 * num_bands)


def head_operands(sd, precision, dtype):
    """Head parameters in `dtype` (copies); to_kv.weight rounded to the 16-bit type first."""
    tdt = TDT[precision]
    keep = ("mlp_offset.", "x_attention_head.")
    return {k: (v.to(tdt) if ".1.fn.to_kv." in k and tdt is not None else v).to(dtype).clone() for k, v in sd.items() if k.startswith(keep)}


def head_forward(sd, zc, zq, feat, K, idx, depth, heads, G, precision, num_bands=16, max_resolution=64):
    """mhmr_hph_forward up to the read-out, in the dtype of its arguments: -> (readout [P, 318 + nb + 3 + 10], offset [P, 2]).
    zc [P, C] = the features at the detected cells (mlp_offset's input), zq [P, C + E] = features | camera embedding at those cells (the
    queries' input), feat [B, N, C] the features the context is built from; zc and zq are separate arguments so that their cotangents
    (g_zc, g_token) can be taken.  The camera embedding of the context is computed from K here.  The context -- with the value tables
    added at the detected cells -- is rounded to the 16-bit operand type (straight-through), as hph_inputs_kernel writes it."""
    from oracle import multihmr_ref as mr
    h = "x_attention_head."
    tdt, dtype = TDT[precision], feat.dtype
    B, N, C_ = feat.shape
    offset = mr.mlp2(sd, "mlp_offset", zc)
    counts, idx_det_0 = mr.rebatch_dense(idx[0])
    xc = zq + sd[h + "cross_queries_x"][idx[1]] + sd[h + "cross_queries_y"][idx[2]]
    nmax, Bp = int(counts.max()), counts.shape[0]
    rows, cols, start = [], [], 0
    for i, c in enumerate(counts.tolist()):
        rows += [i] * c
        cols += list(range(c))
        start += c
    mask = feat.new_zeros(Bp, nmax)
    mask[rows, cols] = 1
    xpad = feat.new_zeros(Bp, nmax, xc.shape[1]).index_put((torch.tensor(rows), torch.tensor(cols)), xc)
    z_K = embedd_camera(K.to(dtype), G, num_bands, max_resolution)                 # [B, G, G, E]
    images = torch.unique(idx[0], sorted=True)
    z_all = torch.cat([feat.reshape(B, G, G, C_), z_K], -1)[images]                               # [B', G, G, Cc]
    add = sd[h + "cross_values_x"][idx[1]] + sd[h + "cross_values_y"][idx[2]]
    z_all = z_all.index_put((idx_det_0, idx[1], idx[2]), add, accumulate=True)
    context = _round_st(z_all.reshape(Bp, N, -1), tdt)
    init_pose, init_betas, init_cam, init_expr = [sd[h + n].to(dtype) for n in ("init_body_pose", "init_betas", "init_cam", "init_expression")]
    expand = lambda t: t.expand(Bp, nmax, -1)
    token = torch.cat([xpad, expand(init_pose), expand(init_betas), expand(init_cam)], dim=-1)
    out = mr.transformer_decoder(sd, h + "transformer.", token, context, mask, depth, heads)
    out = out[rows, cols]
    lin = lambda n: torch.nn.functional.linear(out, sd[h + n + ".weight"], sd[h + n + ".bias"])
    readout = torch.cat([lin("decpose") + init_pose, lin("decshape") + init_betas, lin("deccam") + init_cam, lin("decexpression") + init_expr], 1)
    return readout, offset


def head_grads(sd_all, feat, K, idx, cot_readout, cot_offset, depth, heads, G, precision, dtype, num_bands=16, max_resolution=64):
    """Gradients of sum(cot_readout * readout) + sum(cot_offset * offset): {parameter name: gradient, "g_zc": [P, C], "g_token": [P, C + E]}.
    The init_* buffers ride along in sd without gradient."""
    from oracle import multihmr_ref as mr
    sd = head_operands(sd_all, precision, dtype)
    names = [k for k in sd if "init_" not in k]
    for k in names:
        sd[k].requires_grad_()
    feat = feat.to(dtype)
    B, N, C_ = feat.shape
    rows = idx[1] * G + idx[2]
    zc = feat[idx[0], rows].clone().requires_grad_()
    z_K = embedd_camera(K.to(dtype), G, num_bands, max_resolution).reshape(B, N, -1)
    zq = torch.cat([feat[idx[0], rows], z_K[idx[0], rows]], 1).clone().requires_grad_()
    readout, offset = head_forward(sd, zc, zq, feat, K, idx, depth, heads, G, precision, num_bands, max_resolution)
    s = (readout * cot_readout.to(dtype)).sum() + (offset * cot_offset.to(dtype)).sum()
    grads = torch.autograd.grad(s, [zc, zq] + [sd[k] for k in names], allow_unused=True)
    out = dict(zip(["g_zc", "g_token"] + names, grads))
    return {k: (v if v is not None else torch.zeros_like(zc if k == "g_zc" else zq if k == "g_token" else sd[k])) for k, v in out.items()}, \
        readout.detach(), offset.detach()
