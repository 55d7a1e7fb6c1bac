"""Training the detection head on a frozen backbone: ``Model.forward(..., is_training=True, train_detection=True)``
attaches ``out["scores"]`` to autograd with respect to the four parameters of ``mlp_classif``; ``backward`` is ``mhmr_detect_backward``.

The backward reads what the forward left in the model's per-batch workspace (the hidden layer ``hid_cls``, the context operand) and the
packed second-layer weight, so -- exactly as for ``train_heads`` -- it must run BEFORE the next forward of the same batch size and before
``repack_heads()``: both move a generation counter, and a backward that finds it moved raises.  There is no CPU path.

``Model.forward_features`` passes the caller's feature tensor as one more input of the node: its gradient is the
detector's share of the feature cotangent, ``mhmr_detect_feature_grad``."""
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
    nbytes = _lib.workspace_bytes("mhmr_detect_backward_workspace_bytes", rows, C_)
    wsb = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _lib.check(L.mhmr_detect_backward(hid16.data_ptr(), hid16.stride(0), ctx16.data_ptr(), ctx16.stride(0), w2.data_ptr(), b2.data_ptr(),
                                      g_scores.data_ptr(), rows, C_, int(clamped), dt_id, g_w1.data_ptr(), g_b1.data_ptr(), g_w2.data_ptr(),
                                      g_b2.data_ptr(), wsb.data_ptr(), nbytes, stream), "mhmr_detect_backward")
    return g_w1, g_b1, g_w2, g_b2


def detect_feature_grad(hid16, w16, w2, b2, g_scores, rows, C_, clamped, dt_id, stream, g_feat=None):
    """``mhmr_detect_feature_grad`` on device tensors: hid16 [>= rows, ldh], w16 [C, ldw] (16-bit), w2 [C], b2 [1], g_scores [rows] fp32 ->
    (g_feat [rows, C] or the given [rows, ldg] buffer, dl [rows]: the workspace, as the product used it).  Allocates both."""
    L, dev = _lib.lib(), hid16.device
    if g_feat is None:
        g_feat = torch.empty(rows, C_, dtype=torch.float32, device=dev)
    nbytes = _lib.workspace_bytes("mhmr_detect_feature_grad_workspace_bytes", rows)
    wsb = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
    _lib.check(L.mhmr_detect_feature_grad(hid16.data_ptr(), hid16.stride(0), w16.data_ptr(), w16.stride(0), w2.data_ptr(), b2.data_ptr(),
                                          g_scores.data_ptr(), rows, C_, int(clamped), dt_id, g_feat.data_ptr(), g_feat.stride(0) if rows else C_,
                                          wsb.data_ptr(), nbytes, stream), "mhmr_detect_feature_grad")
    return g_feat, wsb[:rows]


class _DetectFunction(torch.autograd.Function):
    """(features or None, mlp_classif parameters) -> scores [B, G, G, 1]: the values are the ones the forward has already computed."""

    @staticmethod
    def forward(ctx, model, st, features, *params):
        ctx.model, ctx.st = model, st
        ctx.feat_shape = None if features is None else tuple(features.shape)
        return st["scores"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_scores):
        model, st = ctx.model, ctx.st
        need, need_feat = ctx.needs_input_grad[3:], ctx.needs_input_grad[2]
        dev, P, ws = st["dev"], st["P"], st["ws"]
        model._require_current(st["taken"])
        g_scores = g_scores.to(torch.float32).contiguous()
        g_feat, grads = None, (None,) * 4
        with model._lock, torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if any(need):
                g_w1, g_b1, g_w2, g_b2 = detect_backward(ws["hid_cls"], ws["ctx16"], P["cls2_w"], P["cls2_b"], g_scores, st["rows"], P["C"], True,
                                                         P["dt_id"], stream)
                grads = (g_w1, g_b1, g_w2.view(1, -1), g_b2)
            if need_feat:
                g_feat, _ = detect_feature_grad(ws["hid_cls"], P["cls0_w"], P["cls2_w"], P["cls2_b"], g_scores, st["rows"], P["C"], True,
                                                P["dt_id"], stream)
                g_feat = g_feat.view(ctx.feat_shape)
        return (None, None, g_feat) + tuple(g if k else None for g, k in zip(grads, need))


def attach(model, st, features=None, with_params=True):
    """-> scores attached to autograd with respect to the ``mlp_classif`` parameters that require grad (``with_params``: train_detection)
    and to ``features`` (the tensor ``Model.forward_features`` was given, when it requires grad); a detached value otherwise."""
    params = dict(model.named_parameters())
    with torch.enable_grad():
        return _DetectFunction.apply(model, st, features, *[params[n] if with_params else params[n].detach() for n in DETECTION_PARAMETERS])


__all__ = ["DETECTION_PARAMETERS", "detect_backward", "detect_feature_grad", "attach"]
