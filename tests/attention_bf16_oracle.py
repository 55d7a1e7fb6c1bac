"""Oracle of the attention with bf16 operands: the contract of mhmr_attention_bf16_tape / _backward as one closed
form in a chosen dtype, a torch.autograd.Function with that backward, oracle/dinov2_ref's Attention computing through it, and the block
oracle with rounded linears and / or rounded attention.

r() is ``linear_bf16_oracle.round_bf16`` (``torch.Tensor.bfloat16()``).  Per (image, head), over the T real rows:
    S = QSCALE * r(Q) r(K)^T      lse = log2 sum exp2(S)      P = exp2(S - lse)      O = r(P) r(V)      D = rowsum(dO * O)
    dP = r(dO) r(V)^T      dS = P (dP - D)      dV = r(P)^T r(dO)      dQ = 0.125 r(dS) r(K)      dK = 0.125 r(dS)^T r(Q)
S is not rounded, the rounded P is the normalised one, D takes the unrounded dO and the unrounded O.  Layouts are the library's (tests/
backbone_bwd_oracle.py)."""
import copy
import types

import torch

import backbone_bwd_oracle as bo
import linear_bf16_oracle as lo
from oracle import dinov2_ref

QSCALE = 0.18033688011112042        # include/mhmr.h MHMR_ATTN_QSCALE = 64^-0.5 * log2(e); a torch scalar takes the tensor's dtype


def _core(q, k, v, do, rounding):
    """q, k, v [..., T, 64] un-scaled, do [..., T, 64] or None -> (o, lse2, dq, dk, dv), the last three None without ``do``."""
    r = lo.round_bf16 if rounding else (lambda t: t)
    qr, kr, vr = r(q), r(k), r(v)
    s = (qr @ kr.transpose(-2, -1)) * QSCALE
    m = s.max(-1, keepdim=True).values
    lse = m + torch.log2(torch.exp2(s - m).sum(-1, keepdim=True))
    p = torch.exp2(s - lse)
    pr = r(p)
    o = pr @ vr
    if do is None:
        return o, lse.squeeze(-1), None, None, None
    dor = r(do)
    d = (do * o).sum(-1, keepdim=True)
    ds = p * (dor @ vr.transpose(-2, -1) - d)
    dsr = r(ds)
    return o, lse.squeeze(-1), (dsr @ kr) * 0.125, (dsr.transpose(-2, -1) @ qr) * 0.125, pr.transpose(-2, -1) @ dor


def attention_closed_form(qkv, dO, B, T, Tp, H, dtype=torch.float64, rounding=True):
    """qkv [B*Tp, 3C], dO [B*Tp, >= C] -> (out [B*Tp, C], lse2 [B, H, Tp], dqkv [B*Tp, 3C]) in ``dtype``; rows >= T are zeros."""
    C = qkv.shape[1] // 3
    q, k, v = (qkv.to(dtype).reshape(B, Tp, 3, H, 64)[:, :T, i].permute(0, 2, 1, 3) for i in range(3))      # [B, H, T, 64]
    do = dO.to(dtype).reshape(B, Tp, -1)[:, :T, :C].reshape(B, T, H, 64).permute(0, 2, 1, 3)
    o, lse2, dq, dk, dv = _core(q, k, v, do, rounding)
    out = torch.zeros(B, Tp, C, dtype=dtype)
    out[:, :T] = o.permute(0, 2, 1, 3).reshape(B, T, C)
    lse = torch.zeros(B, H, Tp, dtype=dtype)
    lse[:, :, :T] = lse2
    dqkv = torch.zeros(B, Tp, 3, H, 64, dtype=dtype)
    for i, t in enumerate((dq, dk, dv)):
        dqkv[:, :T, i] = t.permute(0, 2, 1, 3)
    return out.reshape(B * Tp, C), lse, dqkv.reshape(B * Tp, 3 * C)


class RoundedAttention(torch.autograd.Function):
    """(q, k, v) [B, H, T, 64] un-scaled -> o, with the contract's backward.  ``rounding`` False: r is the identity."""

    @staticmethod
    def forward(ctx, q, k, v, rounding):
        ctx.save_for_backward(q, k, v)
        ctx.rounding = rounding
        return _core(q, k, v, None, rounding)[0]

    @staticmethod
    def backward(ctx, do):
        q, k, v = ctx.saved_tensors
        _, _, dq, dk, dv = _core(q, k, v, do, ctx.rounding)
        return dq, dk, dv, None


def with_rounded_attention(module, rounding=True):
    """A deep copy of ``module`` whose dinov2_ref.Attention submodules compute their softmax product through ``RoundedAttention`` (their
    two linears are called as they are: rounded or not); every other submodule is untouched."""
    m = copy.deepcopy(module)

    def forward(self, x):
        B, T, C = x.shape
        qkv = self.qkv(x).reshape(B, T, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        o = RoundedAttention.apply(qkv[0], qkv[1], qkv[2], rounding)
        return self.proj(o.transpose(1, 2).reshape(B, T, C))
    for att in [s for s in m.modules() if isinstance(s, dinov2_ref.Attention)]:
        att.forward = types.MethodType(forward, att)
    return m


def rounded(module, linears=True, attention=True):
    """``module`` with rounded linears and / or rounded attention."""
    if attention:
        module = with_rounded_attention(module)
    if linears:
        module = lo.with_rounded_linears(module)
    return module


def rounded_block_backward(blk, x_in, g_out, B, T, Tp, dtype=torch.float64, linears=True, attention=True):
    """``backbone_bwd_oracle.block_backward`` of ``blk`` with bf16-operand linears and / or attention (same arguments, same dict)."""
    return bo.block_backward(rounded(blk, linears, attention), x_in, g_out, B, T, Tp, dtype)
