"""-m gpu: the bf16-operand linears (csrc/linear_bf16.hip) against the fp64 product of the ROUNDED operands.

A product of two bf16 numbers is exact in fp32, so the only error of the kernels against that reference is the order of their fp32
accumulation.  Measure and gate are section 28's (tests/backbone_bwd_oracle.py): relative L2 and maximum error over the largest fp64
magnitude, at most 4x the same two measures of fp32 CPU torch on the same rounded operands.  A wrong rounding mode (truncation) or a
rounded accumulator would show as ~2^-9, a thousand times over the gate.  Every test prints both columns before it asserts."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import backbone_bwd_oracle as bo  # noqa: E402
from linear_bf16_oracle import round_bf16  # noqa: E402
from multi_hmr_amd import _lib, backbone_train as bt  # noqa: E402

SENT = 7.25                       # sentinel behind every output, in the padding columns of a wide output and behind the workspace
FILL = -3.5                       # what the padding columns of a wide INPUT hold: finite, and never an operand
TAIL = 64


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


def wide(t, pad):
    """The device copy of a CPU matrix with `pad` extra columns per row (FILL) -> (the [rows, ld] buffer, ld)."""
    rows, cols = t.shape
    buf = torch.full((rows, cols + pad), FILL, dtype=torch.float32, device=dev())
    buf[:, :cols] = t.to(dev())
    return buf, cols + pad


class Out:
    """An fp32 output [rows, cols] with leading dimension cols + pad: SENT in the padding columns and in TAIL elements behind it."""

    def __init__(self, rows, cols, pad=0):
        self.rows, self.cols, self.ld = rows, cols, cols + pad
        self.buf = torch.full((rows * self.ld + TAIL,), SENT, dtype=torch.float32, device=dev())

    def ptr(self):
        return self.buf.data_ptr()

    def value(self):
        m = self.buf[:self.rows * self.ld].view(self.rows, self.ld)
        assert bool((self.buf[-TAIL:] == SENT).all()), "a write behind an output"
        assert bool((m[:, self.cols:] == SENT).all()), "a write into the padding columns of an output"
        v = m[:, :self.cols].clone()
        assert bool(torch.isfinite(v).all())
        return v


class Workspace:
    def __init__(self, L, M, N, K):
        self.nbytes = int(L.mhmr_linear_bf16_workspace_bytes(M, N, K))
        assert self.nbytes > 0 and self.nbytes % 4 == 0
        self.buf = torch.full((self.nbytes // 4 + TAIL,), SENT, dtype=torch.float32, device=dev())

    def intact(self):
        return bool((self.buf[-TAIL:] == SENT).all())


def run_forward(L, X, W, bias, pad=0):
    (M, K), N = X.shape, W.shape[0]
    Xd, ldx = wide(X, pad)
    Wd, ldw = wide(W, pad)
    bd = None if bias is None else bias.to(dev())
    Y, ws = Out(M, N, pad), Workspace(L, M, N, K)
    _lib.check(L.mhmr_linear_bf16(Xd.data_ptr(), ldx, Wd.data_ptr(), ldw, _lib.ptr(bd), Y.ptr(), Y.ld, M, N, K, ws.buf.data_ptr(), ws.nbytes, stream()),
               "mhmr_linear_bf16")
    torch.cuda.synchronize()
    assert ws.intact(), "a write behind the workspace"
    return Y.value()


def run_input(L, dY, W, dR, pad=0):
    (M, N), K = dY.shape, W.shape[1]
    Gd, ldg = wide(dY, pad)
    Wd, ldw = wide(W, pad)
    Rd, ldr = wide(dR, pad) if dR is not None else (None, 0)
    dX, ws = Out(M, K, pad), Workspace(L, M, N, K)
    _lib.check(L.mhmr_linear_bf16_backward_input(Gd.data_ptr(), ldg, Wd.data_ptr(), ldw, _lib.ptr(Rd), ldr, dX.ptr(), dX.ld, M, N, K,
                                                 ws.buf.data_ptr(), ws.nbytes, stream()), "mhmr_linear_bf16_backward_input")
    torch.cuda.synchronize()
    assert ws.intact(), "a write behind the workspace"
    return dX.value()


def run_weight(L, dY, X, pad=0, want_dw=True, want_db=True):
    (M, N), K = dY.shape, X.shape[1]
    Gd, ldg = wide(dY, pad)
    Xd, ldx = wide(X, pad)
    dW, db, ws = Out(N, K, pad), Out(1, N), Workspace(L, M, N, K)
    _lib.check(L.mhmr_linear_bf16_backward_weight(Gd.data_ptr(), ldg, Xd.data_ptr(), ldx, dW.ptr() if want_dw else None, dW.ld,
                                                  db.ptr() if want_db else None, M, N, K, ws.buf.data_ptr(), ws.nbytes, stream()),
               "mhmr_linear_bf16_backward_weight")
    torch.cuda.synchronize()
    assert ws.intact(), "a write behind the workspace"
    if not want_dw:
        assert bool((dW.buf == SENT).all()), "dW was NULL and something was written"
    if not want_db:
        assert bool((db.buf == SENT).all()), "db was NULL and something was written"
    return (dW.value() if want_dw else None), (db.value()[0] if want_db else None)


# (M, N, K, extra columns of every leading dimension)
SHAPES = [(64, 64, 64, 0), (64, 192, 64, 0), (192, 64, 256, 0), (128, 320, 64, 0), (320, 1536, 384, 0), (320, 384, 1536, 0), (320, 1536, 384, 8)]
NK = [(64, 64), (192, 64), (64, 256), (320, 64), (1536, 384), (384, 1536)]


@functools.lru_cache(maxsize=None)
def _operands(M, N, K):
    """CPU operands and the references of the three products at one shape: computed once, left unchanged."""
    g = torch.Generator().manual_seed(9000 + M + 3 * N + 7 * K)
    X, W, dY = rn(g, M, K) + 0.5, rn(g, N, K), rn(g, M, N)
    bias, dR = rn(g, N), rn(g, M, K)
    Xr, Wr, Gr = round_bf16(X), round_bf16(W), round_bf16(dY)
    assert not torch.equal(Xr, X) and float((Xr - X).abs().max()) <= 2.0 ** -8 * float(X.abs().max())
    c = dict(X=X, W=W, dY=dY, bias=bias, dR=dR)
    c["y64"], c["y32"] = Xr.double() @ Wr.double().T, Xr @ Wr.T
    c["dx64"], c["dx32"] = Gr.double() @ Wr.double(), Gr @ Wr
    c["dw64"], c["dw32"] = Gr.double().T @ Xr.double(), Gr.T @ Xr
    c["db64"], c["dbabs"] = dY.double().sum(0), dY.double().abs().sum(0)
    return c


def check_db(tag, db, c):
    """db is an fp64 sum rounded once: half an fp32 ulp of the result, plus the fp64 sum's own error (1e-13 of the sum of magnitudes)."""
    err = (db.cpu().double() - c["db64"]).abs()
    bound = 2.0 ** -24 * c["db64"].abs() + 1e-13 * c["dbabs"]
    print(f"[{tag}] db: largest error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), tag


@pytest.mark.parametrize("extra", [False, True], ids=["plain", "bias_dR"])
@pytest.mark.parametrize("M,N,K,pad", SHAPES)
def test_forward_and_input_side(L, M, N, K, pad, extra):
    c = _operands(M, N, K)
    bias, dR = (c["bias"], c["dR"]) if extra else (None, None)
    tag = f"bf16 linear M {M} N {N} K {K} ld+{pad}{' +bias/dR' if extra else ''}"
    Y, dX = run_forward(L, c["X"], c["W"], bias, pad), run_input(L, c["dY"], c["W"], dR, pad)
    # two calls give the same bits; the wrappers are the raw entries
    assert torch.equal(run_forward(L, c["X"], c["W"], bias, pad), Y) and torch.equal(run_input(L, c["dY"], c["W"], dR, pad), dX), "two calls differ"
    to = lambda t: None if t is None else t.to(dev())
    assert torch.equal(bt.linear_bf16(to(c["X"]), to(c["W"]), to(bias)), Y), "linear_bf16 differs from the raw entry"
    assert torch.equal(bt.linear_bf16_backward_input(to(c["dY"]), to(c["W"]), to(dR)), dX), "linear_bf16_backward_input differs from the raw entry"
    y64, y32 = (c["y64"] + bias.double(), c["y32"] + bias) if extra else (c["y64"], c["y32"])
    x64, x32 = (c["dx64"] + dR.double(), c["dx32"] + dR) if extra else (c["dx64"], c["dx32"])
    bo.gate(tag, [("Y", Y, y32, y64), ("dX", dX, x32, x64)])


@pytest.mark.parametrize("M", [64, 320, 640])
@pytest.mark.parametrize("N,K", NK)
def test_weight_side(L, M, N, K):
    c = _operands(M, N, K)
    tag = f"bf16 weight side M {M} N {N} K {K}"
    dW, db = run_weight(L, c["dY"], c["X"])
    dW2, db2 = run_weight(L, c["dY"], c["X"])
    assert torch.equal(dW2, dW) and torch.equal(db2, db), "two calls differ"
    # either output alone: the same bits, and nothing written through the NULL pointer
    only_w, _ = run_weight(L, c["dY"], c["X"], want_db=False)
    _, only_b = run_weight(L, c["dY"], c["X"], want_dw=False)
    assert torch.equal(only_w, dW) and torch.equal(only_b, db)
    w_dw, w_db = bt.linear_bf16_backward_weight(c["dY"].to(dev()), c["X"].to(dev()))
    assert torch.equal(w_dw, dW) and torch.equal(w_db, db), "linear_bf16_backward_weight differs from the raw entry"
    check_db(tag, db, c)
    bo.gate(tag, [("dW", dW, c["dw32"], c["dw64"])])


def test_weight_side_wide_leading_dimensions(L):
    M, N, K, pad = 320, 1536, 384, 8
    c = _operands(M, N, K)
    dW, db = run_weight(L, c["dY"], c["X"], pad)
    plain, plain_db = run_weight(L, c["dY"], c["X"])
    assert torch.equal(dW, plain) and torch.equal(db, plain_db), "the leading dimensions changed the result"


# the long sum: only M is long (one block's B * Tp at ViT-L 896^2: 4 160 per image, x 8, x 32)
@pytest.mark.parametrize("M,N,K", [(4160, 64, 64), (33280, 64, 64), (133120, 64, 64), (4160, 128, 64)])
def test_weight_side_long_sum(L, M, N, K):
    c = _operands(M, N, K)
    tag = f"bf16 weight side, long sum M {M} N {N} K {K}"
    dW, db = run_weight(L, c["dY"], c["X"])
    dW2, db2 = run_weight(L, c["dY"], c["X"])
    assert torch.equal(dW2, dW) and torch.equal(db2, db), "two calls differ"
    check_db(tag, db, c)
    bo.gate(tag, [("dW", dW, c["dw32"], c["dw64"])])


@pytest.mark.parametrize("M", [64, 640, 4096, 4160])
def test_rows_of_zeros_in_dy_contribute_nothing(L, M):
    """dW and db with 64 rows of exact zeros appended to dY (and any finite rows appended to X) are the bits of the call without them:
    a padding row of the block, whose cotangent is masked to zero, reaches no parameter gradient.  4096 -> 4160 adds a slice."""
    N, K = 128, 64
    c = _operands(M, N, K)
    dW, db = run_weight(L, c["dY"], c["X"])
    g = torch.Generator().manual_seed(M)
    dY0 = torch.cat([c["dY"], torch.zeros(64, N)])
    X0 = torch.cat([c["X"], rn(g, 64, K) * 5.0 + 2.0])
    dW0, db0 = run_weight(L, dY0, X0)
    assert torch.equal(dW0, dW) and torch.equal(db0, db)
