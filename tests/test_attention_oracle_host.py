"""The inputs and the yardstick of tests/test_gpu_attention_keys.py are fair -- checked on the CPU, without a GPU.

The key-by-key attention test gates the kernels at 4x the error of a torch model of the 16-bit computation (tests/attn_oracle.py).  That
gate means something only if the model itself is as good as the number formats allow on the inputs the test uses, and if no read-out is so
small that the f16 subnormal step, not the kernel, sets its error."""
import pytest
import torch

import attn_oracle as ao


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_yardstick_against_fp64_on_every_length(name):
    """Worst per-key relative error of the yardstick <= 3 u + 2^-13 at every tested T: one rounding of p (u), the row sum as a weighted mean
    of such roundings (u), one output rounding (u); 2^-13 covers the fp32 scores, exp2 and sums.  Every read-out is a normal f16."""
    bound = 3 * ao.U[name] + 2.0 ** -13
    worst, worst_T, smallest = 0.0, 0, float("inf")
    for T in ao.T_KEYS:
        c = ao.key_case(T, name)
        if c["Y"] > worst:
            worst, worst_T = c["Y"], T
        smallest = min(smallest, float(c["w"].min()) * 2.0 ** ao.E16)
        assert abs(float(c["w"].sum(-1).min()) - 1) < 1e-12 and abs(float(c["w"].sum(-1).max()) - 1) < 1e-12
    print(f"[attention yardstick {name}] worst per-key relative error {worst:.3e} (T = {worst_T}; {worst / ao.U[name]:.2f} u), bound {bound:.3e}; "
          f"smallest read-out {smallest:.3e}")
    assert worst <= bound, (worst, worst_T)
    assert smallest >= ao.F16_MIN_NORMAL, smallest


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_one_key_is_exact(name):
    """T = 1: the only weight is 1, the yardstick stores 2^e exactly, so Y = 0 and the GPU test demands the exact bits."""
    c = ao.key_case(1, name)
    assert c["Y"] == 0.0
    assert torch.equal(ao.yardstick16_readout(c["q"], c["k"], ao.E16).double(), torch.full((ao.H, 1, 1), 2.0 ** ao.E16, dtype=torch.float64))
    c = ao.key_case32(1, name)
    assert c["Y"] == 0.0


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_yardstick_of_ordinary_values_matches_the_read_out(name):
    """yardstick16 on the one-hot window V is the read-out of the same keys (one code path for both kinds of test), and on random V it
    stays within the flat bounds of the older attention tests."""
    for T in (17, 65, 200):
        c = ao.key_case(T, name)
        v = ao.window_v(T, T, ao.TDT[name], ao.E16)
        got = ao.yardstick16(c["q"], c["k"], v)
        want = ao.expected_readout(ao.yardstick16_readout(c["q"], c["k"], ao.E16).double(), T, 0)
        assert torch.equal(got.double(), want)
        v = ao.v_inputs(T, name, 2)
        err = float((ao.yardstick16(c["q"], c["k"], v).double() - ao.attention64(c["q"], c["k"], v)).abs().max())
        assert err < (4e-3 if name == "f16" else 3e-2), err


def test_window_layout():
    """Every real key is read out exactly once, by image key // 64 at column key % 64; V^T is key-permuted inside 16-key groups."""
    for T, Tp in ((1, 64), (65, 128), (130, 192)):
        v = ao.window_v(T, Tp, torch.float32, 3)
        assert v.shape == (ao.windows(T), Tp, ao.H, 64)
        assert int((v != 0).sum()) == T * ao.H and float(v.max()) == 8.0
        for key in (0, T - 1):
            assert float(v[key // 64, key, 1, key % 64]) == 8.0
        assert float(v[:, T:].abs().max()) == 0.0 if Tp > T else True
        vt = ao.vt_layout(v)
        key = T - 1
        assert float(vt[key // 64, 0, key % 64, int(ao.swap23(torch.tensor(key)))]) == 8.0
    t = torch.arange(64)
    assert sorted(ao.swap23(t).tolist()) == t.tolist() and int(ao.swap23(torch.tensor(4))) == 8


@pytest.mark.parametrize("name", ["f16", "bf16"])
def test_fp32_yardstick(name):
    """mhmr_attention_f32's yardstick: fp32 softmax + the op16 pair.  Within 2^-16 + the pair's own step (2^-22 f16, 2^-16 bf16) of fp64
    -- a weight's relative error is the ABSOLUTE error of its fp32 score, 64 products of magnitude ~1 summed in fp32, divided by 8 --, and the
    LOW half of the smallest read-out is still a normal f16."""
    pair = 2.0 ** -22 if name == "f16" else 2.0 ** -16
    worst, smallest = 0.0, float("inf")
    for T in ao.T_F32:
        c = ao.key_case32(T, name)
        worst = max(worst, c["Y"])
        smallest = min(smallest, float(c["w"].min()) * 2.0 ** ao.E32)
    print(f"[attention_f32 yardstick {name}] worst per-key relative error {worst:.3e}; smallest read-out {smallest:.3e}")
    assert worst <= 2.0 ** -16 + pair, worst
    assert smallest * 2.0 ** -11 >= ao.F16_MIN_NORMAL, smallest
