"""Oracle of the mixed-precision backbone backward: bf16 rounding as torch does it, one linear whose operands are
rounded in both directions, and oracle/dinov2_ref's own Block with its four nn.Linear modules computing through that linear.

``rounded_block_backward`` is tests/backbone_bwd_oracle.py's ``block_backward`` with the rounding switched on: everything that is not a
linear (LayerNorm, attention, GELU, LayerScale, the residuals, the bias gradients) is dinov2_ref's arithmetic under torch autograd in the
dtype it is given (fp64: the reference, fp32: the yardstick)."""
import copy
import types

import torch

import backbone_bwd_oracle as bo


def round_bf16(t, dtype=None):
    """Round to nearest even to bf16 as ``torch.Tensor.bfloat16()`` does from fp32, widened to ``dtype`` (default: t's own)."""
    return t.float().bfloat16().to(t.dtype if dtype is None else dtype)


class RoundedLinear(torch.autograd.Function):
    """Y = r(X) r(W)^T + b;  dX = r(dY) r(W),  dW = r(dY)^T r(X),  db = the column sums of the UNROUNDED dY -- computed in the dtype of
    the inputs.  ``rounding`` False: r is the identity (a plain linear)."""

    @staticmethod
    def forward(ctx, X, W, b, rounding):
        r = round_bf16 if rounding else (lambda t: t)
        Xr, Wr = r(X), r(W)
        ctx.save_for_backward(Xr, Wr)
        ctx.rounding = rounding
        return torch.nn.functional.linear(Xr, Wr, b)

    @staticmethod
    def backward(ctx, dY):
        Xr, Wr = ctx.saved_tensors
        dYr = round_bf16(dY) if ctx.rounding else dY
        dX = dYr @ Wr
        dW = dYr.reshape(-1, dYr.shape[-1]).T @ Xr.reshape(-1, Xr.shape[-1])
        db = dY.reshape(-1, dY.shape[-1]).sum(0)
        return dX, dW, db, None


def with_rounded_linears(module, rounding=True):
    """A deep copy of ``module`` whose nn.Linear submodules compute through ``RoundedLinear``; every other submodule is untouched."""
    m = copy.deepcopy(module)
    for lin in [s for s in m.modules() if isinstance(s, torch.nn.Linear)]:
        lin.forward = types.MethodType(lambda self, x: RoundedLinear.apply(x, self.weight, self.bias, rounding), lin)
    return m


def rounded_block_backward(blk, x_in, g_out, B, T, Tp, dtype=torch.float64, rounding=True):
    """``backbone_bwd_oracle.block_backward`` of ``blk`` with bf16-operand linears (same arguments, same dict)."""
    return bo.block_backward(with_rounded_linears(blk, rounding), x_in, g_out, B, T, Tp, dtype)      # (block_backward copies and casts)
