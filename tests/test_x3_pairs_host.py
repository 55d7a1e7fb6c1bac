"""CPU: the element-wise gate of tests/test_gpu_x3_pairs.py has power (tests/x3_oracle.py).  A consistent pair passes
it at every element; the double-rounded pair the f16 build of `gelu_pair_kernel` used to store -- restated in numpy, on the very inputs of
each GPU case -- is flagged; and the gate is tight enough on those inputs that it cannot hide such an element."""
import numpy as np
import pytest
import torch

import x3_oracle as xo

DTYPES = ["f16", "bf16"]


def test_pair_bound_is_met_with_equality_nowhere_exceeded():
    """pair_bound against a dense sweep of fp32 values across f16's normal, subnormal and underflow ranges, and half_ulp16 for hi alone."""
    g = torch.Generator(device="cpu").manual_seed(1)
    y = torch.cat([torch.randn(1 << 18, generator=g) * s for s in (100.0, 1.0, 0.1, 2.0 ** -10, 2.0 ** -15, 2.0 ** -22)]
                  + [torch.tensor([0.0, -0.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -3, 1.0, 65504.0])])
    for dtype in DTYPES:
        both, hi = xo.consistent_pair(y, dtype)
        y64 = y.double().numpy()
        r, i = xo.worst_ratio(np.abs(both - y64), xo.pair_bound(y64, dtype))
        r_hi, _ = xo.worst_ratio(np.abs(hi - y64), xo.half_ulp16(y64, dtype))
        print(f"[pair_bound {dtype}] worst |hi + lo - y| / bound {r:.3f} at y = {float(y[i]):.6e}; hi alone / half ulp {r_hi:.3f}")
        assert r <= 1.0 and r_hi <= 1.0
        assert r > 0.25                      # the bound is not slack either (both roundings at the bottom of a binade: rare)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N", xo.GELU_CASES)
def test_gelu_consistent_pair_passes_and_the_gate_is_tight(M, N, dtype):
    k = xo.gelu_case(M, N)
    gate = xo.gate(k["c"], k["scale"], k["y64"], dtype)
    both, hi = xo.consistent_pair(k["y32"], dtype)
    r, i = xo.worst_ratio(np.abs(both - k["y64"]), gate)
    r_hi, _ = xo.worst_ratio(np.abs(hi - k["y64"]), xo.half_ulp16(k["y64"], dtype) + gate)
    share = float(np.mean(gate <= 2.0 ** -13 * np.abs(k["y64"])))
    print(f"[gelu {M}x{N} {dtype}] c = {k['c'] * 2 ** 24:.2f} * 2^-24, consistent pair {r:.3f} of its gate (x = {float(k['x'].flatten()[i]):.4f}), "
          f"hi {r_hi:.3f}, gate <= 2^-13 |y| at {100 * share:.1f} %")
    assert k["c"] < 4 * 2.0 ** -24                      # the restatement is an fp32 GELU: a few units
    assert r <= 1.0 and r_hi <= 1.0
    assert share >= 0.80                                # a quarter of the smallest error of the defect (2^-11 |y|): nothing to hide behind


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C", xo.LN_CASES)
def test_layernorm_consistent_pair_passes_and_the_gate_is_tight(rows, C, dtype):
    k = xo.layernorm_case(rows, C)
    gate = xo.gate(k["c"], k["scale"], k["y64"], dtype)
    both, hi = xo.consistent_pair(k["y32"], dtype)
    r, _ = xo.worst_ratio(np.abs(both - k["y64"]), gate)
    r_hi, _ = xo.worst_ratio(np.abs(hi - k["y64"]), xo.half_ulp16(k["y64"], dtype) + gate)
    share = float(np.mean(gate <= 2.0 ** -13 * np.abs(k["y64"])))
    print(f"[layernorm {rows}x{C} {dtype}] c = {k['c'] * 2 ** 24:.2f} * 2^-24, consistent pair {r:.3f} of its gate, hi {r_hi:.3f}, "
          f"gate <= 2^-13 |y| at {100 * share:.1f} %")
    assert k["c"] < 16 * 2.0 ** -24
    assert r <= 1.0 and r_hi <= 1.0
    assert share >= 0.80
    # the constant row: variance 0, y = b
    const = k["y64"][xo.LN_CONST_ROW]
    assert np.array_equal(const, k["b"].double().numpy())


@pytest.mark.parametrize("M,N", xo.GELU_CASES)
def test_the_double_rounded_gelu_pair_is_flagged(M, N):
    """The defect on the GPU case's own inputs: >= 32 tie hazards, and the emulated pair misses the gate at >= 32 elements by >= 2^-12 |y| each
    (one f16 unit is 2^-11 ... 2^-10 |y|), i.e. hundreds of times the gate -- while everywhere else it is a correct pair."""
    k = xo.gelu_case(M, N)
    a, b = xo.gelu32_factors(k["x"])
    hazards = xo.count_tie_hazards(a.numpy(), b.numpy())
    hi, lo = xo.emulate_double_rounded_pair(a.numpy(), b.numpy())
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - k["y64"])
    gate = xo.gate(k["c"], k["scale"], k["y64"], "f16")
    bad = err > gate
    big = bad & (err >= 2.0 ** -12 * np.abs(k["y64"]))
    r, _ = xo.worst_ratio(err, gate)
    print(f"[gelu {M}x{N}] tie hazards {hazards}, emulated pair over its gate at {int(bad.sum())} elements ({int(big.sum())} by >= 2^-12 |y|), "
          f"worst {r:.0f} x the gate, relative error of the flagged {float((err[big] / np.abs(k['y64'][big])).min()):.2e} ... "
          f"{float((err[big] / np.abs(k['y64'][big])).max()):.2e}; whole-array relative L2 {np.linalg.norm(err) / np.linalg.norm(k['y64']):.1e}")
    assert hazards >= 32
    assert int(big.sum()) >= 32
    assert int(bad.sum()) <= hazards                    # only hazards (those at x << 0, where y is tiny against 4 c |x|, stay inside)
    assert np.linalg.norm(err) / np.linalg.norm(k["y64"]) < 2e-5          # ... and invisible to a relative L2 gate of 2e-5
    # the stored hi is right (op16 of the fp32 value); it is lo that belongs to another hi
    assert np.array_equal(hi, xo.op16(a * b, "f16").numpy())


@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (256, 384, 1536)])
def test_linear_gate_admits_the_exact_three_products(M, N, K):
    """The fp64 sum of the three products of the pair operands lies inside the operand part alone (no accumulation allowance)."""
    k = xo.linear_case(M, N, K)
    A2, W3 = k["A2"].double(), k["W3"].double()
    three = (A2[:, :K] @ W3[:, :K].T + A2[:, :K] @ W3[:, K:2 * K].T + A2[:, K:] @ W3[:, 2 * K:].T).numpy()
    r, _ = xo.worst_ratio(np.abs(three - k["exact"]), k["operand"])
    one = (A2[:, :K] @ W3[:, :K].T).numpy()
    r1, _ = xo.worst_ratio(np.abs(one - k["exact"]), k["operand"] + 4.0 * k["Y"] * k["S"])
    print(f"[linear {M}x{N}x{K}] Y = {k['Y'] * 2 ** 24:.2f} * 2^-24; three exact products {r:.3f} of the operand part; hi x hi alone {r1:.0f} x the whole gate")
    assert r <= 1.0
    assert r1 > 10.0                        # a missing low-half product cannot pass, the accumulation allowance included
    assert k["Y"] < 2.0 ** -20
