"""Training the detection head on a frozen backbone: ``Model.forward(..., is_training=True, train_detection=True)``
attaches ``out["scores"]`` to autograd with respect to the four parameters of ``mlp_classif``; ``backward`` is ``mhmr_detect_backward``.

The backward reads what the forward left in the model's per-batch workspace (the hidden layer ``hid_cls``, the context operand) and the
packed second-layer weight, so -- exactly as for ``train_heads`` -- it must run BEFORE the next forward of the same batch size and before
``repack_heads()``: both move a generation counter, and a backward that finds it moved raises.  There is no CPU path."""
from __future__ import annotations

import torch

from . import _lib

DETECTION_PARAMETERS = ("mlp_classif.0.weight", "mlp_classif.0.bias", "mlp_classif.2.weight", "mlp_classif.2.bias")


def detect_backward(hid16, ctx16, w2, b2, g_scores, rows, C_, clamped, dt_id, stream):
    """``mhmr_detect_backward`` on device tensors: hid16 [>= rows, ldh], ctx16 [>= rows, ldx] (16-bit), w2 [C], b2 [1], g_scores [rows] fp32 ->
    (g_w1 [C, C], g_b1 [C], g_w2 [C], g_b2 [1]).  Allocates the outputs and the workspace."""
    L, dev = _lib.lib(), hid16.device
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    g_w1, g_b1, g_w2, g_b2 = f(C_, C_), f(C_), f(C_), f(1)
    nbytes = int(L.mhmr_detect_backward_workspace_bytes(rows, C_))
    if nbytes < 0:
        _lib.check(nbytes, "mhmr_detect_backward_workspace_bytes")
    wsb = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _lib.check(L.mhmr_detect_backward(hid16.data_ptr(), hid16.stride(0), ctx16.data_ptr(), ctx16.stride(0), w2.data_ptr(), b2.data_ptr(),
                                      g_scores.data_ptr(), rows, C_, int(clamped), dt_id, g_w1.data_ptr(), g_b1.data_ptr(), g_w2.data_ptr(),
                                      g_b2.data_ptr(), wsb.data_ptr(), nbytes, stream), "mhmr_detect_backward")
    return g_w1, g_b1, g_w2, g_b2


class _DetectFunction(torch.autograd.Function):
    """(mlp_classif parameters) -> scores [B, G, G, 1]: the values are the ones the forward has already computed."""

    @staticmethod
    def forward(ctx, model, st, *params):
        ctx.model, ctx.st = model, st
        return st["scores"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_scores):
        model, st = ctx.model, ctx.st
        need = ctx.needs_input_grad[2:]
        dev, P, ws = st["dev"], st["P"], st["ws"]
        if ws.get("generation") != st["generation"] or P.get("heads_generation") != st["heads_generation"] or model._packed is not P:
            raise _lib.MhmrError("Model: backward must run before the next forward of the same batch size and before repack_heads() / "
                                 "repack(): the workspace (context operand, features) or the packed head weights this forward used have "
                                 "been overwritten since")
        g_scores = g_scores.to(torch.float32).contiguous()
        with model._lock, torch.cuda.device(dev):
            g_w1, g_b1, g_w2, g_b2 = detect_backward(ws["hid_cls"], ws["ctx16"], P["cls2_w"], P["cls2_b"], g_scores, st["rows"], P["C"], True,
                                                     P["dt_id"], torch.cuda.current_stream(dev).cuda_stream)
        grads = (g_w1, g_b1, g_w2.view(1, -1), g_b2)
        return (None, None) + tuple(g if k else None for g, k in zip(grads, need))


def attach(model, st):
    """-> scores attached to autograd with respect to the ``mlp_classif`` parameters that require grad (a detached value otherwise)."""
    params = dict(model.named_parameters())
    with torch.enable_grad():
        return _DetectFunction.apply(model, st, *[params[n] for n in DETECTION_PARAMETERS])


__all__ = ["DETECTION_PARAMETERS", "detect_backward", "attach"]
