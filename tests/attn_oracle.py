"""TEST INFRASTRUCTURE: the ViT attention (csrc/attention.hip, csrc/attention_f32.hip) restated in torch on the CPU, for a test that reads
out the softmax weight of EVERY key of every query.

The read-out.  V is one-hot inside a window of 64 keys, V[j0 + d, d] = 2^e and zero elsewhere, so out[q, d] = 2^e w[q, j0 + d]: one output
element is the weight of one key for one query, and a wrong mask, a dropped key or a key counted twice moves it by its whole size instead
of by 1 / T of an average.  The windows of one length ride as the images of ONE launch (same Q and K, another V per image).

Three computations of the same weights:
  weights64     fp64 softmax_2(q k^T) on the rounded operands: the reference;
  yardstick16   a model of the 16-bit kernels' arithmetic: fp32 scores, level = row maximum of key tile 0, p = op16(exp2(s - level)) rounded
                to nearest, fp32 sums, one division, the output rounded to op16.  Its own error against fp64 is the unit the kernels are
                gated in (the 4x rule of DESIGN.md section 16);
  yardstick32   plain fp32 torch softmax(q k^T / 8) v for mhmr_attention_f32, its result split into the [hi | lo] op16 pair the kernel
                stores and added up again (the pair is the output FORMAT: 22 significand bits in f16, 16 in bf16)."""
from __future__ import annotations

import functools
import math

import torch

from multi_hmr_amd._lib import ATTN_QSCALE

TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
U = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}           # unit roundoff of the operand types
F16_MIN_NORMAL = 2.0 ** -14
H, D, KB = 2, 64, 64                                 # heads of every case (different data per head), head dimension, key tile = window
E16 = 6                                              # read-out scale 2^e of the 16-bit forms: the smallest weight at T = 1025 stays a normal f16
E32 = 14                                             # ... of mhmr_attention_f32: the LOW half of the smallest read-out stays normal as well

#: test 1: every tail length three times mod 64 (once mod 128), T <= 64, the 16 / 32 / 64 / 96 / 128 edges; the lengths around 256, one-
#: and two-query-block tails behind two and a half workgroups (272 / 273, 320 / 321); the production lengths 257 and 1025 (5 / 17 windows)
T_KEYS = tuple(range(1, 193)) + (255, 256, 257, 258, 272, 273, 320, 321, 1025)
_EDGES = (1, 16, 17, 32, 33, 64, 65, 96, 97, 128, 129, 192, 255, 256, 257, 258, 272, 273, 320, 321, 1025)
#: test 2: every residue mod 64 once (spread over T <= 64, 65 ... 128, 129 ... 192) plus the edges
T_PAD = tuple(sorted(set(r + 64 * (r % 3) for r in range(1, 65)) | set(_EDGES)))
T_PLAIN = (17, 64, 65, 200, 257, 577)                # test 3: ordinary V
T_F32 = tuple(range(1, 131)) + (257,)                # test 4


def swap23(t):
    """The key permutation of V^T (MHMR_EPI_VT): bits 2 and 3 of the key index swapped."""
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


def roundup(n, m):
    return (n + m - 1) // m * m


def windows(T):
    return (T + KB - 1) // KB


def qk_inputs(T, name):
    """q [T, H, 64] PRE-SCALED by ATTN_QSCALE (scores in the exp2 domain), k [T, H, 64] ~ N(0, 1), rounded to the operand type; seeded per
    (T, dtype, head)."""
    q, k = torch.empty(T, H, D), torch.empty(T, H, D)
    for h in range(H):
        g = torch.Generator().manual_seed(4 * T + 2 * h + (name == "bf16"))
        q[:, h] = torch.randn(T, D, generator=g) * ATTN_QSCALE
        k[:, h] = torch.randn(T, D, generator=g)
    return q.to(TDT[name]), k.to(TDT[name])


def v_inputs(T, name, B, seed=0):
    """Ordinary values: v [B, T, H, 64] ~ N(0, 1) in the operand type."""
    g = torch.Generator().manual_seed(7919 * T + 2 * seed + (name == "bf16"))
    return torch.randn(B, T, H, D, generator=g).to(TDT[name])


def window_v(T, Tp, dtype, e):
    """v [windows(T), Tp, H, 64]: image b reads out keys 64 b ... 64 b + 63 (V[b, 64 b + d, :, d] = 2^e for the real keys, zero elsewhere)."""
    nw = windows(T)
    v = torch.zeros(nw, Tp, H, D, dtype=dtype)
    j = torch.arange(T)
    v[j // KB, j, :, j % KB] = 2.0 ** e
    return v


def vt_layout(v):
    """v [B, Tp, H, 64] -> the kernels' V^T operand [B, H, 64, Tp], key-permuted."""
    vt = torch.zeros(v.shape[0], v.shape[2], v.shape[3], v.shape[1], dtype=v.dtype, device=v.device)
    vt[..., swap23(torch.arange(v.shape[1], device=v.device))] = v.permute(0, 2, 3, 1)
    return vt


def expected_readout(w, T, e):
    """w [H, T, T] -> what a read-out launch stores in rows < T: [windows(T), T, H * 64] = 2^e w[h, q, 64 b + d], exact zeros where key
    64 b + d does not exist."""
    nw = windows(T)
    full = torch.zeros(H, T, nw * KB, dtype=w.dtype)
    full[:, :, :T] = w * 2.0 ** e
    return full.view(H, T, nw, KB).permute(2, 1, 0, 3).reshape(nw, T, H * KB)


# ------------------------------------------------------------------------------------------------------ 16-bit forms
def weights64(q, k):
    """fp64 softmax_2(q k^T) on the rounded operands: [H, T, T]."""
    qd, kd = q.double().permute(1, 0, 2), k.double().permute(1, 0, 2)
    return torch.softmax(qd @ kd.transpose(-1, -2) * math.log(2.0), dim=-1)


def attention64(q, k, v):
    """fp64 attention of v [B, T, H, 64]: [B, T, H * 64]."""
    out = weights64(q, k)[None] @ v.double().permute(0, 2, 1, 3)
    return out.permute(0, 2, 1, 3).reshape(v.shape[0], v.shape[1], -1)


def _p16(q, k):
    """The yardstick's probabilities and row sums: p [H, T, T] in the operand type, l [H, T] fp32."""
    qf, kf = q.float().permute(1, 0, 2), k.float().permute(1, 0, 2)
    s = qf @ kf.transpose(-1, -2)                                            # fp32 scores of the rounded operands
    level = s[:, :, :KB].max(dim=-1, keepdim=True).values                   # row maximum of key tile 0, then fixed
    p = torch.exp2(s - level).to(q.dtype)                                   # ONE rounding to nearest per probability
    return p, p.float().sum(dim=-1)


def yardstick16(q, k, v):
    """The 16-bit computation on v [B, T, H, 64]: fp32 sums of the ROUNDED p, one division, the output rounded to op16 -> [B, T, H * 64]."""
    p, l = _p16(q, k)
    out = (p.float()[None] @ v.float().permute(0, 2, 1, 3)) / l[None, :, :, None]
    return out.to(q.dtype).permute(0, 2, 1, 3).reshape(v.shape[0], v.shape[1], -1)


def yardstick16_readout(q, k, e):
    """What the yardstick stores for the read-out of EVERY key, [H, T, T] in the operand type (a one-hot V picks one product per sum)."""
    p, l = _p16(q, k)
    return ((p.float() * 2.0 ** e) / l[:, :, None]).to(q.dtype)


def worst_rel(got, ref):
    """Worst relative error over the elements with a non-zero reference."""
    nz = ref != 0
    return float(((got.double() - ref).abs()[nz] / ref[nz]).max()) if bool(nz.any()) else 0.0


@functools.lru_cache(maxsize=None)
def key_case(T, name):
    """One (T, dtype) of the read-out tests, computed once and shared: q, k, the fp64 weights w [H, T, T] and Y = the yardstick's own worst
    per-key relative error."""
    q, k = qk_inputs(T, name)
    w = weights64(q, k)
    Y = worst_rel(yardstick16_readout(q, k, E16), w * 2.0 ** E16)
    return dict(q=q, k=k, w=w, Y=Y)


# ------------------------------------------------------------------------------------------------------ mhmr_attention_f32
def qkv_inputs32(T, seed=0):
    """fp32 q, k [T, H, 64] ~ N(0, 1), UN-scaled (the kernel multiplies by 1 / 8 itself)."""
    q, k = torch.empty(T, H, D), torch.empty(T, H, D)
    for h in range(H):
        g = torch.Generator().manual_seed(100003 + 4 * T + 2 * h + seed)
        q[:, h] = torch.randn(T, D, generator=g)
        k[:, h] = torch.randn(T, D, generator=g)
    return q, k


def weights64_f32(q, k):
    qd, kd = q.double().permute(1, 0, 2), k.double().permute(1, 0, 2)
    return torch.softmax(qd @ kd.transpose(-1, -2) / 8.0, dim=-1)


def pair_sum(x, dtype):
    """x fp32 -> hi + lo in fp64, hi = op16(x), lo = op16(x - hi): the value an op16 PAIR holds."""
    hi = x.to(dtype)
    lo = (x - hi.float()).to(dtype)
    return hi.double() + lo.double()


def yardstick32_readout(q, k, e, dtype):
    """Plain fp32 torch softmax(q k^T / 8) against the one-hot V of every key, stored as an op16 pair: [H, T, T] fp64."""
    qf, kf = q.permute(1, 0, 2), k.permute(1, 0, 2)
    w = torch.softmax(qf @ kf.transpose(-1, -2) / 8.0, dim=-1)
    return pair_sum(w * 2.0 ** e, dtype)


@functools.lru_cache(maxsize=None)
def key_case32(T, name):
    q, k = qkv_inputs32(T)
    w = weights64_f32(q, k)
    Y = worst_rel(yardstick32_readout(q, k, E32, TDT[name]), w * 2.0 ** E32)
    return dict(q=q, k=k, w=w, Y=Y)
