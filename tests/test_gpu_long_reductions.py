"""-m gpu: the fp32 training kernels at the backbone's reduction lengths.  The person head's linears and the
attention tape / backward accumulate in fp32 MFMA chains whose error grows with the summed index; the block backward runs them with
M = B Tp token rows (4 160 ... 133 120), K and N up to 4096 and T up to 4097.  Here only the summed index is long, every other dimension
is tiny, and each kernel is compared with fp64 on the CPU.

Measure and gate (tests/backbone_bwd_oracle.py): per tensor the relative L2 error against fp64 and the maximum error relative to the
tensor's largest fp64 magnitude; the yardstick is fp32 CPU torch of the same expression, and the kernels may be at most 4x worse in
either measure.  Every test prints both columns before it asserts."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import backbone_bwd_oracle as bo  # noqa: E402
import test_gpu_backbone_backward as tb  # noqa: E402
from multi_hmr_amd import _lib  # noqa: E402
from test_gpu_backbone_backward import SENT, TAIL, dev, guarded, intact, rn, stream  # noqa: E402

ACTS = {"none": _lib.ACT_NONE, "gelu": _lib.ACT_GELU}


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def pitched(t, ld):
    """A device copy of the CPU matrix t [rows, width] inside a buffer of pitch ``ld`` whose other columns hold the sentinel -> the view."""
    buf = torch.full((t.shape[0], ld), SENT, dtype=torch.float32, device=dev())
    buf[:, :t.shape[1]] = t.to(dev())
    return buf[:, :t.shape[1]]


# ------------------------------------------------------------------------------------------------------ (1) weight side: the chain over M rows
WGT_N, WGT_K = 40, 96             # a ragged last 16-tile of n; three of the four waves of the one workgroup along k
WGT_M = (640, 4160, 33280, 133120)  # the block test's B Tp; one, 8 and 32 images of 896^2


@functools.lru_cache(maxsize=None)
def _weight_case(M, act):
    g = torch.Generator().manual_seed(7000 + M + len(act))
    dY, Z = rn(g, M, WGT_N), rn(g, M, WGT_N)
    X = rn(g, M, WGT_K) + 0.5                                  # activations behind a GELU or a LayerNorm bias have a mean
    r64 = bo.linear_backward(dY, Z, X, None, None, act, torch.float64)
    y32 = bo.linear_backward(dY, Z, X, None, None, act, torch.float32)
    return dict(dY=dY, Z=Z, X=X, r64=r64, y32=y32)


def _weight_run(L, c, M, act, pad=0):
    """dW, db of the case with every pitch ``pad`` larger than the width; dW's buffer is sentinel-filled, pad columns included."""
    N, K = WGT_N, WGT_K
    dY, Z, X = (pitched(c[k], c[k].shape[1] + pad) for k in ("dY", "Z", "X"))
    wb = torch.full((N * (K + pad) + TAIL,), SENT, dtype=torch.float32, device=dev())
    bb, db = guarded(N)
    _lib.check(L.mhmr_linear_f32_backward_weight(dY.data_ptr(), N + pad, Z.data_ptr(), N + pad, X.data_ptr(), K + pad, wb.data_ptr(), K + pad,
                                                 db.data_ptr(), M, N, K, ACTS[act], stream()), "mhmr_linear_f32_backward_weight")
    torch.cuda.synchronize()
    full = wb[:N * (K + pad)].view(N, K + pad)
    assert intact(wb, bb) and bool((full[:, K:] == SENT).all()), "a write outside dW or db"
    return full[:, :K], db


@pytest.mark.parametrize("act", ["none", "gelu"])
@pytest.mark.parametrize("M", WGT_M)
def test_weight_side_over_token_rows(L, M, act):
    c = _weight_case(M, act)
    dW, db = _weight_run(L, c, M, act)
    assert bool(torch.isfinite(dW).all()) and bool(torch.isfinite(db).all())
    bo.gate(f"weight side M {M} N {WGT_N} K {WGT_K} {act}", [("dW", dW, c["y32"]["dW"], c["r64"]["dW"]), ("db", db, c["y32"]["db"], c["r64"]["db"])])


@pytest.mark.parametrize("act", ["none", "gelu"])
def test_weight_side_with_pitches_wider_than_the_rows(L, act):
    """lddy, ldz, ldx and lddw 8 larger than the widths: the same bits as the contiguous call, nothing written between the rows of dW."""
    M = 4160
    c = _weight_case(M, act)
    dW, db = _weight_run(L, c, M, act, pad=8)
    flat, fb = _weight_run(L, c, M, act)
    assert torch.equal(dW, flat) and torch.equal(db, fb), "the pitches changed the result"
    bo.gate(f"weight side M {M} pitches + 8 {act}", [("dW", dW, c["y32"]["dW"], c["r64"]["dW"]), ("db", db, c["y32"]["db"], c["r64"]["db"])])


# ------------------------------------------------------------------------------------------------------ (2) forward, both forms: the chain over K
def selects_splitk(M, N, K):
    """The dispatch rule of mhmr_launch_linear_f32 (csrc/hph.hip), restated: K >= 256 goes to linear_f32_splitk_kernel (K / 4 per wave)
    while ceil(N / 128) * ceil(M / 16) < 1024 tiles; otherwise linear_f32_kernel runs one chain over all of K.  Whoever moves that threshold
    moves the shapes below with it, so that both forms stay under test at every K."""
    return K >= 256 and ((N + 127) // 128) * ((M + 15) // 16) < 1024


#: (M, N, the form the rule selects): exactly 1024 tiles; ragged in both directions; a few tiles
FWD_SHAPES = [(4096, 512, "plain"), (4100, 520, "plain"), (64, 96, "splitk")]


@functools.lru_cache(maxsize=None)
def _forward_case(M, N, K):
    g = torch.Generator().manual_seed(8000 + M + N + K)
    X, W = rn(g, M, K) + 0.5, rn(g, N, K, std=K ** -0.5)
    bias, R = rn(g, N, std=0.1), rn(g, M, N)
    return dict(X=X, W=W, bias=bias, R=R, r64=bo.linear_forward(X, W, bias, R, torch.float64), y32=bo.linear_forward(X, W, bias, R, torch.float32))


@pytest.mark.parametrize("K", [256, 1024, 4096])
@pytest.mark.parametrize("M,N,form", FWD_SHAPES)
def test_forward_linear_in_both_forms(L, M, N, form, K):
    assert selects_splitk(M, N, K) == (form == "splitk"), "the shape no longer selects the form this case is about"
    c = _forward_case(M, N, K)
    X, W, bias, R = (c[k].to(dev()).contiguous() for k in ("X", "W", "bias", "R"))
    yb, Y = guarded(M, N)
    _lib.check(L.mhmr_linear_f32(X.data_ptr(), K, None, W.data_ptr(), K, bias.data_ptr(), R.data_ptr(), N, Y.data_ptr(), N, M, N, K, _lib.ACT_NONE,
                                 stream()), "mhmr_linear_f32")
    torch.cuda.synchronize()
    assert intact(yb) and bool(torch.isfinite(Y).all())
    bo.gate(f"forward {form} M {M} N {N} K {K}", [("Y", Y, c["y32"], c["r64"])])


# ------------------------------------------------------------------------------------------------------ (3) input side: four chains over N / 4
INP_M, INP_K = 130, 64


@functools.lru_cache(maxsize=None)
def _input_case(N, act):
    g = torch.Generator().manual_seed(9000 + N + len(act))
    dY, Z = rn(g, INP_M, N), rn(g, INP_M, N)
    W, dR = rn(g, N, INP_K, std=INP_K ** -0.5), rn(g, INP_M, INP_K)
    r64 = bo.linear_backward(dY, Z, None, W, dR, act, torch.float64)
    y32 = bo.linear_backward(dY, Z, None, W, dR, act, torch.float32)
    return dict(dY=dY, Z=Z, W=W, dR=dR, r64=r64["dX"], y32=y32["dX"])


@pytest.mark.parametrize("act", ["none", "gelu"])
@pytest.mark.parametrize("N", [1024, 3072, 4096])
def test_input_side_over_wide_layers(L, N, act):
    M, K = INP_M, INP_K
    c = _input_case(N, act)
    dY, Z, W, dR = (c[k].to(dev()).contiguous() for k in ("dY", "Z", "W", "dR"))
    xb, dX = guarded(M, K)
    _lib.check(L.mhmr_linear_f32_backward_input(dY.data_ptr(), N, None, Z.data_ptr(), N, W.data_ptr(), K, dR.data_ptr(), K, dX.data_ptr(), K, M, N, K,
                                                ACTS[act], stream()), "mhmr_linear_f32_backward_input")
    torch.cuda.synchronize()
    assert intact(xb) and bool(torch.isfinite(dX).all())
    bo.gate(f"input side M {M} N {N} K {K} {act}", [("dX", dX, c["y32"], c["r64"])])


# ------------------------------------------------------------------------------------------------------ (4) attention: the chains over T keys / queries
ATT_LONG = [(1025, 1088), (2305, 2368), (4097, 4160)]          # the token counts of 448^2, 672^2 and 896^2


@functools.lru_cache(maxsize=None)
def _attention_case(T, Tp):
    """As test_gpu_backbone_backward._attention_case with B = H = 1.  The fp64 closed form holds a few T x T matrices: computed once per case,
    only the results are kept."""
    Cd = 64
    g = torch.Generator().manual_seed(5000 + 7 * T + Tp)
    qkv = rn(g, Tp, 3 * Cd)
    qkv[:, :Cd] *= 2.0
    dO = rn(g, Tp, Cd)
    r64 = bo.attention_backward_closed_form(qkv, dO, 1, T, Tp, 1, torch.float64)
    y32 = bo.attention_backward_autograd(qkv, dO, 1, T, Tp, 1, torch.float32)
    o64, lse64 = bo.attention_forward(qkv, 1, T, Tp, 1, torch.float64)
    o32, _ = bo.attention_forward(qkv, 1, T, Tp, 1, torch.float32)
    return dict(qkv=qkv, dO=dO, r64=r64, y32=y32, o64=o64, o32=o32, lse64=lse64)


@pytest.mark.parametrize("T,Tp", ATT_LONG)
def test_attention_at_the_backbone_token_counts(L, T, Tp):
    Cd = 64
    c = _attention_case(T, Tp)
    out32, lse, dqkv = tb._attention_run(L, c["qkv"], c["dO"], 1, T, Tp, 1)          # asserts the sentinels behind every output
    real = torch.arange(Tp) < T
    o, l, d = out32.cpu(), lse.cpu(), dqkv.cpu()
    assert bool((o[~real] == 0).all()) and bool((l.reshape(1, 1, Tp)[:, :, T:] == 0).all())
    lmx = float((l.double() - c["lse64"]).abs().max())
    print(f"[attention T {T} Tp {Tp}] tape: lse max abs error {lmx:.3e}, largest |lse| {float(c['lse64'].abs().max()):.2f}")
    assert bool(torch.isfinite(d).all()) and bool((d[~real] == 0).all()), "rows >= T of dqkv are not exact zeros"
    rows = [("tape out32", o, c["o32"], c["o64"]), ("dqkv", d, c["y32"], c["r64"])]
    rows += [(n, d[:, i * Cd:(i + 1) * Cd], c["y32"][:, i * Cd:(i + 1) * Cd], c["r64"][:, i * Cd:(i + 1) * Cd]) for i, n in enumerate(("dQ", "dK", "dV"))]
    bo.gate(f"attention T {T} Tp {Tp}", rows)
    assert float(c["lse64"].abs().max()) < 32 and lmx < 1e-5
