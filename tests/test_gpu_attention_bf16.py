"""-m gpu: the attention tape and backward with bf16 operands on their own (csrc/attention_bf16.hip).

References (tests/attention_bf16_oracle.py): ``r64`` the contract's closed form with its roundings in fp64, ``y32`` the same closed form in
fp32 on the CPU (the yardstick) and ``u64`` the unrounded fp64 closed form.

Small cases (B = 2, H = 2).  The exact properties -- zeros in the rows >= T, equal bits from two calls, image 0 of B = 2 equal to B = 1, no
bit moved by other finite values in the rows >= T of qkv, dO and out32, intact sentinels -- and a value gate: per tensor the relative L2
distance to ``r64`` is at most 1/4 of the relative L2 distance between ``r64`` and ``u64``, the cost of the mode.  The project's ratio gate
against the yardstick cannot be used at these sizes: an fp32 evaluation differs from ``r64`` by a handful of bf16 rounding-boundary crossings
in P and dS, and between two legitimate fp32 orders that ratio swung from 0.03 to 31.  ``y32`` must pass the same gate.

Pooled cases (H = 16, B = 8 ... 32).  With enough (image, head) pairs the crossings are a stable statistic and the project's gate applies
unchanged: ``bo.gate(..., factor=4.0)``, kernel against ``y32``, both measured to ``r64``, per tensor."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_bf16_oracle as ao  # noqa: E402
import backbone_bwd_oracle as bo  # noqa: E402
from multi_hmr_amd import _lib, backbone_train as bt  # noqa: E402

SENT, TAIL = 7.25, 64
SMALL_B, SMALL_H = 2, 2
#: (T, Tp, lddo - C)
SMALL_CASES = [(T, bo.roundup(T, 64), 0) for T in (2, 16, 17, 33, 64, 65, 129, 257)] + [(65, 192, 0), (33, 64, 8)]
POOLED_CASES = [(257, 8, 16), (129, 16, 16), (65, 32, 16)]
NAMES = ("dQ", "dK", "dV")


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def rn(g, *shape):
    return torch.empty(*shape).normal_(0, 1, generator=g)


def guarded(*shape):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + TAIL,), SENT, dtype=torch.float32, device=dev())
    return buf, buf[:n].view(*shape)


@functools.lru_cache(maxsize=None)
def _case(T, Tp, B, H, seed=0):
    """CPU operands (padding rows hold finite values of their own) and the three references, computed once and left unchanged."""
    Cd = 64 * H
    g = torch.Generator().manual_seed(5100 + 7 * T + Tp + 1000 * seed)
    qkv = rn(g, B * Tp, 3 * Cd)
    qkv[:, :Cd] *= 2.0                                         # logits of standard deviation ~2: the softmax is not flat
    dO = rn(g, B * Tp, Cd)
    r64 = ao.attention_closed_form(qkv, dO, B, T, Tp, H, torch.float64)
    y32 = ao.attention_closed_form(qkv, dO, B, T, Tp, H, torch.float32)
    u64 = ao.attention_closed_form(qkv, dO, B, T, Tp, H, torch.float64, rounding=False)
    return dict(qkv=qkv, dO=dO, r64=r64, y32=y32, u64=u64)


def _run(L, qkv, dO, B, T, Tp, H, extra=0, refill=None):
    """tape + backward into sentinel-guarded buffers -> (out32, lse, dqkv).  ``extra``: dO has the pitch C + extra.  ``refill``: a generator
    seed; the rows >= T of qkv, dO and out32 are overwritten with other finite values before the backward runs (the tape ran on the refilled
    qkv as well, and must give the same out32)."""
    Cd = 64 * H
    qkv = qkv.to(dev()).contiguous()
    dOp = torch.full((B * Tp, Cd + extra), 9.5, dtype=torch.float32, device=dev())
    dOp[:, :Cd] = dO.to(dev())
    ob, out32 = guarded(B * Tp, Cd)
    lb, lse = guarded(B, H, Tp)
    gb, dqkv = guarded(B * Tp, 3 * Cd)
    nbytes = int(L.mhmr_attention_bf16_workspace_bytes(B, Tp, Cd, H))
    assert nbytes >= 14 * B * Tp * Cd + 4 * B * H * Tp
    wb = torch.full((nbytes // 4 + TAIL,), SENT, dtype=torch.float32, device=dev())
    pad = (torch.arange(B * Tp) % Tp >= T).to(dev())
    if refill is not None:
        g = torch.Generator().manual_seed(refill)
        qkv = qkv.clone()
        qkv[pad] = (rn(g, B * Tp, 3 * Cd) * 3.0 + 1.0).to(dev())[pad]
    _lib.check(L.mhmr_attention_bf16_tape(qkv.data_ptr(), out32.data_ptr(), lse.data_ptr(), B, T, Tp, Cd, H, wb.data_ptr(), nbytes, stream()), "tape")
    tape_out = out32.clone()
    if refill is not None:
        dOp[pad, :Cd] = (rn(g, B * Tp, Cd) * 5.0 - 2.0).to(dev())[pad]
        out32[pad] = (rn(g, B * Tp, Cd) * 4.0).to(dev())[pad]
    wb[:nbytes // 4] = SENT                                    # the backward converts on its own: nothing of the tape's workspace is needed
    _lib.check(L.mhmr_attention_bf16_backward(qkv.data_ptr(), out32.data_ptr(), lse.data_ptr(), dOp.data_ptr(), Cd + extra, dqkv.data_ptr(), B, T,
                                              Tp, Cd, H, wb.data_ptr(), nbytes, stream()), "backward")
    torch.cuda.synchronize()
    assert all(bool((b[-TAIL:] == SENT).all()) for b in (ob, lb, gb, wb)), "a write behind an output or the workspace"
    return tape_out.cpu(), lse.cpu(), dqkv.cpu()


def _tensors(out, dqkv, Cd):
    return dict(out32=out, dQ=dqkv[:, :Cd], dK=dqkv[:, Cd:2 * Cd], dV=dqkv[:, 2 * Cd:], dqkv=dqkv)


@pytest.mark.parametrize("T,Tp,extra", SMALL_CASES)
def test_small_cases_exact_properties_and_the_value_gate(L, T, Tp, extra):
    B, H, Cd = SMALL_B, SMALL_H, 64 * SMALL_H
    c = _case(T, Tp, B, H)
    out32, lse, dqkv = _run(L, c["qkv"], c["dO"], B, T, Tp, H, extra)
    real = torch.arange(B * Tp) % Tp < T
    assert bool(torch.isfinite(out32).all()) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(dqkv).all())
    assert bool((out32[~real] == 0).all()) and bool((lse[:, :, T:] == 0).all()) and bool((dqkv[~real] == 0).all()), "rows >= T are not exact zeros"
    # two calls; image 0 alone; other finite values in the rows >= T
    again = _run(L, c["qkv"], c["dO"], B, T, Tp, H, extra)
    assert all(torch.equal(a, b) for a, b in zip(again, (out32, lse, dqkv))), "two calls differ"
    one = _run(L, c["qkv"][:Tp], c["dO"][:Tp], 1, T, Tp, H, extra)
    assert torch.equal(one[0], out32[:Tp]) and torch.equal(one[1], lse[:1]) and torch.equal(one[2], dqkv[:Tp]), "image 0 of B = 2 differs from B = 1"
    if Tp > T:
        other = _run(L, c["qkv"], c["dO"], B, T, Tp, H, extra, refill=77 + T)
        assert all(torch.equal(a, b) for a, b in zip(other, (out32, lse, dqkv))), "the padding rows reached a real row"
    # the wrappers
    wo, wl = bt.attention_bf16_tape(c["qkv"].to(dev()), B, T, Tp, H)
    wd = bt.attention_bf16_backward(c["qkv"].to(dev()), wo, wl, c["dO"].to(dev()), B, T, Tp, H)
    assert torch.equal(wo.cpu(), out32) and torch.equal(wl.cpu(), lse) and torch.equal(wd.cpu(), dqkv), "the wrappers differ"
    # lse (logits of |value| < 32, where fp32 numbers are 3.8e-6 apart, and a handful of roundings: 1e-5 absolute)
    r_out, r_lse, r_d = c["r64"]
    lmx = float((lse.double() - r_lse).abs().max())
    print(f"[attention bf16 T {T} Tp {Tp}] lse max abs error {lmx:.3e}, largest |lse| {float(r_lse.abs().max()):.2f}")
    assert float(r_lse.abs().max()) < 32 and lmx < 1e-5
    # the value gate: a quarter of the cost of the mode, per tensor; the fp32 restatement passes it too
    got, r64, y32, u64 = _tensors(out32, dqkv, Cd), _tensors(r_out, r_d, Cd), _tensors(c["y32"][0], c["y32"][2], Cd), _tensors(c["u64"][0], c["u64"][2], Cd)
    bad = []
    for n in ("out32",) + NAMES:
        cost, k, y = bo.measure(r64[n], u64[n])[0], bo.measure(got[n], r64[n])[0], bo.measure(y32[n], r64[n])[0]
        ok = k <= 0.25 * cost and y <= 0.25 * cost
        print(f"[attention bf16 T {T} Tp {Tp}] {n}: rel L2 to r64: kernel {k:.3e}, fp32 restatement {y:.3e}; cost of the mode {cost:.3e}"
              f"{'' if ok else '  <-- FAILS'}")
        if not ok:
            bad.append(n)
    assert not bad, bad


@pytest.mark.parametrize("T,B,H", POOLED_CASES)
def test_pooled_cases_against_the_fp32_yardstick(L, T, B, H):
    Tp, Cd = bo.roundup(T, 64), 64 * H
    c = _case(T, Tp, B, H)
    out32, lse, dqkv = _run(L, c["qkv"], c["dO"], B, T, Tp, H)
    assert float((lse.double() - c["r64"][1]).abs().max()) < 1e-5
    got, r64, y32 = _tensors(out32, dqkv, Cd), _tensors(c["r64"][0], c["r64"][2], Cd), _tensors(c["y32"][0], c["y32"][2], Cd)
    for n in ("out32",) + NAMES + ("dqkv",):
        (kl2, kmx), (yl2, ymx) = bo.measure(got[n], r64[n]), bo.measure(y32[n], r64[n])
        print(f"[attention bf16 pooled T {T} B {B} H {H}] {n}: kernel / yardstick ratio: rel L2 {kl2 / yl2:.2f}, max {kmx / ymx:.2f}")
    bo.gate(f"attention bf16 pooled T {T} B {B} H {H}", [(n, got[n], y32[n], r64[n]) for n in ("out32",) + NAMES + ("dqkv",)], factor=4.0)
