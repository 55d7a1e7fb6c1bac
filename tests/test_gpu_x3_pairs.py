"""-m gpu: the operand pairs of the "f16x3" precision mode, ELEMENT BY ELEMENT (tests/x3_oracle.py holds the cases, the
fp64 statements, the yardsticks and the derivation of every bound; tests/test_x3_pairs_host.py shows on the CPU that the gates have power).
The mode's accuracy rests on every [hi | lo] pair recomposing to its fp32 value to 2^-22; a pair that is wrong at one element in 2^14 has a
relative L2 error of 5e-6 and passes every norm gate of tests/test_gpu_x3.py.  Here every element of `mhmr_gelu16_pair` and
`mhmr_layernorm16_pair` meets  4 c scale + pair_bound(y),  and every element of the three-product `mhmr_gemm16_ex` its own gate; unit
operands then pin which k range of the activation meets which k range of the weight."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multi_hmr_amd import _lib  # noqa: E402
import x3_oracle as xo  # noqa: E402

DT = {"f16": (_lib.DT_F16, torch.float16), "bf16": (_lib.DT_BF16, torch.bfloat16)}
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def check_pair(tag, out, rows, n, k, dtype):
    """out [>= rows, 2 n] = [hi | lo]: every element of hi + lo inside the gate, hi alone within half a 16-bit unit (plus the gate) of fp64."""
    o = out[:rows].cpu().double().numpy()
    hi, both = o[:, :n], o[:, :n] + o[:, n:]
    gate = xo.gate(k["c"], k["scale"], k["y64"], dtype)
    err = np.abs(both - k["y64"])
    r, i = xo.worst_ratio(err, gate)
    r_hi, i_hi = xo.worst_ratio(np.abs(hi - k["y64"]), xo.half_ulp16(k["y64"], dtype) + gate)
    over = int(np.count_nonzero(~(err <= gate)))
    print(f"\n[{tag} {dtype}] c = {k['c'] * 2 ** 24:.2f} * 2^-24; worst |hi + lo - y| / gate {r:.3f} at element {divmod(i, n)} "
          f"(y = {k['y64'].flat[i]:.6e}, got {both.flat[i]:.6e}), {over} elements over; worst hi {r_hi:.3f} at {divmod(i_hi, n)}")
    assert over == 0 and r <= 1.0, (tag, dtype, over, r)
    assert r_hi <= 1.0, (tag, dtype, r_hi)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("M,N", xo.GELU_CASES)
def test_gelu_pair_every_element(L, M, N, dtype):
    """x = 2 randn with a row of specials (+-0, +-1e-6, +-2^-14, +-6, +-10, -20); about a hundred elements per case whose fp32 result sits on
    an f16 tie (tests/test_x3_pairs_host.py counts them).  N = 1536: the last workgroup is half full; N = 4096 has M N / 4 = 1024 M, always
    whole workgroups.  One guard row behind the output."""
    k = xo.gelu_case(M, N)
    dt, tdt = DT[dtype]
    x = k["x"].to(dev())
    out = torch.full((M + 1, 2 * N), NAN, dtype=tdt, device=dev())
    _lib.check(L.mhmr_gelu16_pair(x.data_ptr(), out.data_ptr(), M, N, dt, stream()), "gelu pair")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[M:]).all())                                  # nothing behind the last row
    check_pair(f"gelu {M}x{N}", out, M, N, k, dtype)
    sp = out[xo.GELU_SPECIAL_ROW, :2].cpu().float()
    assert float(sp[0]) == 0.0 and float(sp[1]) == 0.0                        # gelu(+-0) = 0 exactly


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("rows,C", xo.LN_CASES)
def test_layernorm_pair_every_element(L, rows, C, dtype):
    """x = 3 randn + 1.5, w = exp(0.5 randn) with a x30 channel, b = randn, one constant row (y = b); rows = 1 mod 4: the last workgroup
    has one live wave, and the three rows behind it must stay unwritten."""
    k = xo.layernorm_case(rows, C)
    dt, tdt = DT[dtype]
    x, w, b = (k[n].to(dev()) for n in ("x", "w", "b"))
    out = torch.full((rows + 3, 2 * C), NAN, dtype=tdt, device=dev())
    _lib.check(L.mhmr_layernorm16_pair(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), rows, C, 1e-6, dt, stream()), "ln pair")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[rows:]).all())                               # nothing past row `rows`
    check_pair(f"layernorm {rows}x{C}", out, rows, C, k, dtype)


# (M, N, a_k): the 128x128 kernel (M or N no multiple of 256) at one k tile pair, four and twenty-four per range; the last two are whole
# 256x256 tiles and run on the 256x256 kernel.  (B, Np, Tp) of the patch epilogue: B Np rounded up to 128 rows = M, as vit_forward_x3 pads.
LINEAR_CASES = [(128, 128, 128), (384, 256, 256), (256, 384, 1536), (256, 256, 256), (512, 256, 1024)]
PATCH_ROWS = {(128, 128, 128): (3, 37, 128), (384, 256, 256): (3, 100, 128), (256, 384, 1536): (2, 100, 128), (256, 256, 256): (2, 100, 128),
              (512, 256, 1024): (3, 170, 256)}


def gemm_x3(L, A2, W3, M, N, K, bias, gamma, out, epi, pos=None, Np=0, Tp=128, Mvalid=None):
    _lib.check(L.mhmr_gemm16_ex(A2.data_ptr(), 2 * K, W3.data_ptr(), 3 * K, M, N, 3 * K, _lib.ptr(bias), _lib.ptr(gamma), out.data_ptr(), N, _lib.ptr(pos),
                                Np, Tp, N // 64, M if Mvalid is None else Mvalid, epi, _lib.DT_F16, 0, 0, K, stream()), "gemm x3")
    torch.cuda.synchronize()


def report(tag, got, ref64, gate, k):
    r, i = xo.worst_ratio(np.abs(got.cpu().double().numpy() - ref64), gate)
    print(f"\n[{tag}] Y = {k['Y'] * 2 ** 24:.2f} * 2^-24; worst |out - fp64| / gate {r:.3f} at {divmod(i, ref64.shape[1])}")
    return r


@pytest.mark.parametrize("epi", ["f32", "resid", "patch"])
@pytest.mark.parametrize("M,N,K", LINEAR_CASES)
def test_three_product_linear_every_element(L, M, N, K, epi):
    """[A_hi | A_lo] x [W_hi | W_lo | W_hi] against fp64 on the UNROUNDED operands: a x40 hot column, a 1e-4 column and weights whose low
    halves are subnormal.  Gate per element: the operand part (three discarded terms of 2^-22 |a| |w| and the subnormal steps), four times
    the accumulation error of a CPU fp32 matmul of the same products, and half an fp32 unit for each rounding of the epilogue."""
    k = xo.linear_case(M, N, K)
    A2, W3, bias = k["A2"].to(dev()), k["W3"].to(dev()), k["bias"].to(dev())
    v = k["exact"] + k["bias"].double().numpy()[None, :]
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    if epi == "f32":
        out = torch.full((M, N), NAN, device=dev())
        gemm_x3(L, A2, W3, M, N, K, bias, None, out, _lib.EPI_F32)
        r = report(f"linear f32 {M}x{N}x{K}", out, v, xo.linear_gate(k, [v]), k)
    elif epi == "resid":
        gamma, r0 = 0.5 + torch.rand(N, generator=g), torch.randn(M, N, generator=g)
        out = r0.to(dev())
        gemm_x3(L, A2, W3, M, N, K, bias, gamma.to(dev()), out, _lib.EPI_RESID)
        gv = gamma.double().numpy()[None, :] * v
        ref = r0.double().numpy() + gv
        r = report(f"linear resid {M}x{N}x{K}", out, ref, xo.linear_gate(k, [gv, gv, ref], gamma.double().numpy()), k)     # v, gamma v, r0 + gamma v
    else:
        B, Np, Tp = PATCH_ROWS[(M, N, K)]
        Mvalid = B * Np
        assert (Mvalid + 127) // 128 * 128 == M
        pos = torch.randn(1 + Np, N, generator=g)
        out = torch.full((B * Tp, N), NAN, device=dev())
        gemm_x3(L, A2, W3, M, N, K, bias, None, out, _lib.EPI_PATCH, pos.to(dev()), Np, Tp, Mvalid)
        got = out.view(B, Tp, N)
        assert bool(torch.isnan(got[:, Np:]).all())                          # the class slot and the padding rows stay untouched
        ref = v[:Mvalid] + np.tile(pos[1:].double().numpy(), (B, 1))                 # row m = b Np + n takes pos[1 + n]
        gate = (k["operand"] + 4.0 * k["Y"] * k["S"])[:Mvalid] + 2.0 ** -24 * (np.abs(v[:Mvalid]) + np.abs(ref))
        r = report(f"linear patch {M}x{N}x{K}", got[:, :Np].reshape(Mvalid, N), ref, gate, k)
    assert r <= 1.0, (epi, M, N, K, r)


@pytest.mark.parametrize("M,N,K", LINEAR_CASES)
def test_unit_operands_pin_the_k_ranges(L, M, N, K):
    """Three DIFFERENT weight ranges [W1 | W2 | W3] and one non-zero activation per row, at column j of the first or the last k tile
    (row m: j = 1, 63, K - 64, K - 1 in turn), no bias:
      A_hi = 0, A_lo = a e_j:  out = a W3[n, j] BIT FOR BIT (one product of two 11-bit values, exact in fp32): the low half meets the third
                               range and nothing else -- no A_lo W_lo term;
      A_lo = 0, A_hi = a e_j:  out = a (W1 + W2)[n, j] to one fp32 unit: the high half meets the first two ranges and not the third."""
    g = torch.Generator(device="cpu").manual_seed(7 * M + N + K)
    W = [(0.03 * torch.randn(N, K, generator=g)).half() for _ in range(3)]
    W[1] = (W[1].float() * 2.0 ** -11).half()                                # the size of a low half (subnormal f16 values among them)
    W3 = torch.cat(W, dim=1).contiguous().to(dev())
    a = ((1.0 + torch.rand(M, generator=g)) * torch.where(torch.rand(M, generator=g) < 0.5, -1.0, 1.0)).half()
    js = torch.tensor([1, 63, K - 64, K - 1])[torch.arange(M) % 4]
    rows = torch.arange(M)
    for half in (1, 0):
        A2 = torch.zeros(M, 2 * K, dtype=torch.float16)
        A2[rows, half * K + js] = a
        out = torch.full((M, N), NAN, device=dev())
        gemm_x3(L, A2.to(dev()), W3, M, N, K, None, None, out, _lib.EPI_F32)
        got = out.cpu()
        if half == 1:
            want = (a.double()[:, None] * W[2].double()[:, js].T)
            assert torch.equal(want.float().double(), want)                  # the product is an fp32 value
            bad = int((got.double() != want).sum())
            print(f"\n[unit operands {M}x{N}x{K}] A_lo e_j: {bad} elements differ from a W3[n, j]")
            assert bad == 0
        else:
            want = (a.double()[:, None] * (W[0].double() + W[1].double())[:, js].T).numpy()
            r, i = xo.worst_ratio(np.abs(got.double().numpy() - want), xo.ulp32(want))
            print(f"[unit operands {M}x{N}x{K}] A_hi e_j: worst |out - a (W1 + W2)[n, j]| = {r:.3f} fp32 units at {divmod(i, N)}")
            assert r <= 1.0
