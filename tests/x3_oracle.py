"""Host statements for the operand pairs of the "f16x3" precision mode: what a correct [hi | lo] pair may miss, fp64
statements of the GELU and the LayerNorm that produce pairs, fp32 restatements of both in the kernels' operation order (the yardsticks), a
numpy restatement of the double-rounded pair the f16 build of `gelu_pair_kernel` used to store, and the gate of the three-product linear.
No GPU use; reads nothing outside tests/.  The cases (shapes, seeds, inputs) of tests/test_gpu_x3_pairs.py live here, so that
tests/test_x3_pairs_host.py proves on the CPU, on the very same inputs, that the GPU test's gate catches that defect."""
import functools

import numpy as np
import torch

TORCH16 = {"f16": torch.float16, "bf16": torch.bfloat16}
SIG_BITS = {"f16": 11, "bf16": 8}                     # significant bits of the 16-bit operand formats (the hidden one included)

GELU_CASES = [(1367, 1536), (513, 4096)]              # (M, N): M N >= 2^21; 1367 * 1536 / 4 = 256 * 2050 + 128: the last workgroup is half full
LN_CASES = [(2733, 384), (1365, 768), (1025, 1024)]   # (rows, C): rows = 1 mod 4 (three idle waves in the last workgroup), rows C >= 2^20
GELU_SPECIALS = [0.0, -0.0, 1e-6, -1e-6, 2.0 ** -14, -2.0 ** -14, 6.0, -6.0, 10.0, -10.0, -20.0]
GELU_SPECIAL_ROW, LN_CONST_ROW, LN_CONST = 5, 7, 1.5


def pair_bound(y, dtype):
    """Bound on |float(hi) + float(lo) - y| for a correct pair hi = op16(y), lo = op16(y - hi) of an fp32 value y:
    2^-22 |y| + 2^-25 (f16), 2^-16 |y| (bf16).

    * hi is within half a 16-bit unit of y: |y - hi| <= 2^-p |y| with p = 11 (f16) / 8 (bf16) significant bits.  (hi may also be the one
      rounding of the exact fused result that y is the fp32 rounding of: that moves it by at most 2^-24 |y| more, 2^-35 |y| after the
      next step -- below everything here.)
    * y - hi is exact in fp32: both are multiples of y's fp32 unit and the difference is below 2^-p |y|, i.e. it needs 24 - p bits.
    * lo rounds that difference ONCE to p bits: |(y - hi) - lo| <= 2^-p |y - hi| <= 2^-2p |y|.
    * f16 only: lo is subnormal (|lo| < 2^-14) whenever |y| < 2^-3, and then its rounding is absolute, half a subnormal step = 2^-25
      (which also covers a subnormal hi: |y| < 2^-14 leaves |y - hi| <= 2^-25 and lo in {0, +-2^-24}).  bf16 has fp32's exponent range."""
    y = np.abs(np.asarray(y, dtype=np.float64))
    return 2.0 ** -22 * y + 2.0 ** -25 if dtype == "f16" else 2.0 ** -16 * y


def half_ulp16(y, dtype):
    """Half a unit in the last place of the 16-bit format at |y| (fp64 in, fp64 out): the most op16(y) may differ from y."""
    y = np.abs(np.asarray(y, dtype=np.float64))
    _, e = np.frexp(y)                                                         # y = m 2^e, m in [0.5, 1): the leading bit is 2^(e-1)
    h = np.ldexp(1.0, e - 1 - SIG_BITS[dtype])
    return np.maximum(h, 2.0 ** -25) if dtype == "f16" else h


def ulp32(y):
    _, e = np.frexp(np.abs(np.asarray(y, dtype=np.float64)))
    return np.ldexp(1.0, e - 24)


def op16(y32, dtype):
    """fp32 torch tensor -> the 16-bit format, round to nearest even, ONE rounding."""
    assert y32.dtype == torch.float32
    return y32.to(TORCH16[dtype])


def consistent_pair(y32, dtype):
    """The pair as the header states it: hi = op16(y), lo = op16(y - hi), both from the SAME fp32 y.  Returns hi + lo in fp64 and hi in fp64."""
    hi = op16(y32, dtype)
    lo = op16(y32 - hi.float(), dtype)
    return (hi.double() + lo.double()).numpy(), hi.double().numpy()


# ------------------------------------------------------------------------------------------------ GELU
def gelu64(x):
    """Exact-erf GELU in fp64: x Phi(x) = 0.5 x (1 + erf(x / sqrt 2))."""
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def gelu32_factors(x):
    """The two fp32 factors of the kernel's product, in its order: a = 0.5 x, b = 1 + erf(x * 0.70710678f)."""
    assert x.dtype == torch.float32
    return 0.5 * x, 1.0 + torch.erf(x * torch.tensor(0.70710678118654752440, dtype=torch.float32))


def gelu32(x):
    a, b = gelu32_factors(x)
    return a * b


def gelu_scale(x):
    """Size of one fp32 rounding of the GELU at x: b = 1 + erf is O(1) with an absolute error of a few 2^-24, so y = a b errs by ~|x| 2^-24
    wherever x is -- also where y itself is tiny (x << 0, b cancels)."""
    return x.double().abs().numpy()


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm64(x, w, b, eps=1e-6):
    x = x.double()
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w.double() + b.double()


def layernorm32(x, w, b, eps=1e-6):
    """The kernel's order in fp32: mean = sum * (1/C); centred second pass; rstd = rsqrt(q * (1/C) + eps); ((x - mean) rstd) w + b."""
    assert x.dtype == torch.float32
    C = x.shape[1]
    inv = torch.tensor(1.0 / C, dtype=torch.float32)
    mean = x.sum(dim=1, keepdim=True) * inv
    d = x - mean
    rstd = torch.rsqrt((d * d).sum(dim=1, keepdim=True) * inv + torch.tensor(eps, dtype=torch.float32))
    return d * rstd * w + b


def layernorm_scale(x, w, b, eps=1e-6):
    """(|x| + |mean|) rstd |w| + |b|: the UN-centred magnitude, because x - mean cancels where x ~ mean and the error of the mean stays."""
    x = x.double()
    mean = x.mean(dim=1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(dim=1, keepdim=True) + eps)
    return ((x.abs() + mean.abs()) * rstd * w.double().abs() + b.double().abs()).numpy()


# ------------------------------------------------------------------------------------------------ the gate
def yardstick(y32, y64, scale):
    """c = max |fp32 restatement - fp64| / scale over the elements with scale > 0 (scale = 0 demands the pair bound alone)."""
    err = np.abs(np.asarray(y32, dtype=np.float64) - y64)
    ok = scale > 0
    assert np.all(err[~ok] == 0.0)
    return float((err[ok] / scale[ok]).max())


def gate(c, scale, y64, dtype):
    """Element-wise: 4 c scale + pair_bound(y64) -- the 4x rule on the arithmetic, the derived bound on the format."""
    return 4.0 * c * scale + pair_bound(y64, dtype)


def worst_ratio(err, g):
    """max err / gate (an element with gate 0 must have err 0: ratio 0, else inf)."""
    err, g = np.asarray(err, dtype=np.float64), np.asarray(g, dtype=np.float64)
    r = np.where(g > 0, err / np.where(g > 0, g, 1.0), np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isfinite(err), r, np.inf)                    # a NaN left in the output fails
    i = int(np.argmax(r))
    return float(r.flat[i]), i


# ------------------------------------------------------------------------------------------------ the defect, restated
def emulate_double_rounded_pair(a, b):
    """numpy restatement of what the f16 build of `gelu_pair_kernel` stored before the fix, for y = a * b (fp32 arrays):
        hi (stored) = v_cvt_pk_f16_f32(v_mul_f32(a, b))            = RN16(RN32(a b))
        lo          = v_fma_mixlo_f16(a, b, -hi'), hi' = v_fma_mixlo_f16(a, b, 0) = RN16(a b)   (each ONE rounding of the exact value)
    The product of two fp32 values is exact in fp64, and so is a b - hi' (it spans bits 2^(e-47) ... 2^(e-11)).  numpy converts
    float64 -> float16 with one rounding (torch goes through float32).  Returns (hi, lo) as float16 arrays."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    p = a.astype(np.float64) * b.astype(np.float64)
    hi = p.astype(np.float32).astype(np.float16)
    hi_fused = p.astype(np.float16)
    lo = (p - hi_fused.astype(np.float64)).astype(np.float16)
    return hi, lo


def count_tie_hazards(a, b):
    """Elements where RN32(a b) lies EXACTLY half way between two neighbouring f16 values while the exact product lies off the tie on the
    side round-to-even leaves: the only elements at which RN16(RN32(a b)) != RN16(a b)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    p = a.astype(np.float64) * b.astype(np.float64)
    y = p.astype(np.float32)
    even = y.astype(np.float16)                                                   # round to nearest EVEN
    with np.errstate(over="ignore"):
        other = np.nextafter(even, np.where(y.astype(np.float64) > even.astype(np.float64), np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
    tie = np.isfinite(other) & (0.5 * (even.astype(np.float64) + other.astype(np.float64)) == y.astype(np.float64)) & (even != other)
    off_even = np.abs(p - other.astype(np.float64)) < np.abs(p - even.astype(np.float64))
    return int(np.count_nonzero(tie & off_even))


# ------------------------------------------------------------------------------------------------ cases shared by the host and the GPU test
@functools.lru_cache(maxsize=None)
def gelu_case(M, N):
    """x = 2 randn, one row starting with the specials; fp64 statement, fp32 restatement, scale, yardstick.  Computed once; read only."""
    g = torch.Generator(device="cpu").manual_seed(1000 + N)
    x = 2.0 * torch.randn(M, N, generator=g)
    x[GELU_SPECIAL_ROW, :len(GELU_SPECIALS)] = torch.tensor(GELU_SPECIALS, dtype=torch.float32)
    y64, scale = gelu64(x).numpy(), gelu_scale(x)
    y32 = gelu32(x)
    return {"x": x, "y64": y64, "y32": y32, "scale": scale, "c": yardstick(y32.numpy(), y64, scale)}


@functools.lru_cache(maxsize=None)
def layernorm_case(rows, C):
    """x = 3 randn + 1.5, w = exp(0.5 randn) with one x30 channel, b = randn, one CONSTANT row (variance 0: y = b up to the error of the mean)."""
    g = torch.Generator(device="cpu").manual_seed(2000 + C)
    x = 3.0 * torch.randn(rows, C, generator=g) + 1.5
    w, b = torch.exp(0.5 * torch.randn(C, generator=g)), torch.randn(C, generator=g)
    w[5] *= 30.0
    x[LN_CONST_ROW] = LN_CONST
    y64, scale = layernorm64(x, w, b).numpy(), layernorm_scale(x, w, b)
    y32 = layernorm32(x, w, b)
    return {"x": x, "w": w, "b": b, "y64": y64, "y32": y32, "scale": scale, "c": yardstick(y32.numpy(), y64, scale)}


# ------------------------------------------------------------------------------------------------ the three-product linear
def split16(x32, dtype):
    hi = op16(x32, dtype)
    return hi, op16(x32 - hi.float(), dtype)


@functools.lru_cache(maxsize=None)
def linear_case(M, N, K, dtype="f16"):
    """A [M, K] = randn with a x40 hot column (as behind a x30 LayerNorm weight) and a 1e-4 column whose low half is subnormal in f16;
    W [N, K] = 0.03 randn (every low half subnormal in f16).  The pair operands, S = sum_k |a| |w| in fp64, and the two parts of the gate:

    operand part  3 * 2^-22 S + 2^-25 sum_k (|a_mk| + |w_nk|)  (f16; 3 * 2^-16 S in bf16):  with a = a_hi + a_lo + da, w = w_hi + w_lo + dw
        and |da| <= pair_bound(a), |dw| <= pair_bound(w):  a w - (a_hi w_hi + a_hi w_lo + a_lo w_hi) = a_lo w_lo + da w + a dw - ..., each of
        the three at most 2^-22 |a| |w|, plus 2^-25 |w| and 2^-25 |a| from the subnormal low halves.
    accumulation part  4 Y S:  Y = max |fp32 matmul of [A_hi | A_hi | A_lo] [W_hi | W_lo | W_hi]^T on the CPU - fp64 of the same products| / S,
        the 4x rule on a plain fp32 evaluation of the very sum the kernel forms."""
    g = torch.Generator(device="cpu").manual_seed(3000 + M + N + K)
    A = torch.randn(M, K, generator=g)
    A[:, 3] *= 40.0
    A[:, 9] *= 1e-4
    W = 0.03 * torch.randn(N, K, generator=g)
    bias = torch.randn(N, generator=g)
    a_hi, a_lo = split16(A, dtype)
    w_hi, w_lo = split16(W, dtype)
    A2, W3 = torch.cat([a_hi, a_lo], dim=1).contiguous(), torch.cat([w_hi, w_lo, w_hi], dim=1).contiguous()
    A3 = torch.cat([a_hi, a_hi, a_lo], dim=1)                # the activation columns the three k ranges read (the index wraps at K)
    exact = (A.double() @ W.double().T).numpy()
    S = (A.double().abs() @ W.double().abs().T).numpy()
    Y = float((np.abs((A3.float() @ W3.float().T).double().numpy() - (A3.double() @ W3.double().T).numpy()) / S).max())
    u2, sub = (2.0 ** -22, 2.0 ** -25) if dtype == "f16" else (2.0 ** -16, 0.0)
    operand = 3.0 * u2 * S + sub * (A.double().abs().sum(dim=1)[:, None] + W.double().abs().sum(dim=1)[None, :]).numpy()
    return {"A": A, "W": W, "bias": bias, "A2": A2, "W3": W3, "exact": exact, "S": S, "Y": Y, "operand": operand}


def linear_gate(case, roundings, gamma=None):
    """operand part + 4 Y S (both times |gamma| under the residual epilogue) + the epilogue's own fp32 roundings: `roundings` lists the fp64
    values of the intermediate results the epilogue rounds (acc + bias; gamma v; the output ...), each good to half an fp32 unit 2^-24 |r|."""
    g = case["operand"] + 4.0 * case["Y"] * case["S"]
    if gamma is not None:
        g = g * np.abs(gamma)[None, :]
    return g + 2.0 ** -24 * sum(np.abs(r) for r in roundings)
