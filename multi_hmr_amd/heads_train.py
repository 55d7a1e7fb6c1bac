"""Training the heads on a frozen backbone: ``Model.forward(..., is_training=True, return_readout=True,
train_heads=True)`` attaches ``out["readout"]`` and ``out["offset"]`` to autograd with respect to the parameters of ``x_attention_head``
and ``mlp_offset``; ``backward`` is ``mhmr_hph_backward``.

The backward reads what the forward left in the model's per-batch workspace (the context operand with the detected cells' rows, the
features) and in the packed head weights, so it must run BEFORE the next forward of the same batch size and before ``repack_heads()``:
both move a generation counter, and a backward that finds it moved raises.  There is no CPU path.

``Model.forward_features`` passes the caller's feature tensor as one more input of the node: its gradient is the
heads' share of the feature cotangent, ``mhmr_hph_backward_desc.g_feat`` -- the dense term of every context row plus ``g_zc`` and
``g_token`` at the persons' rows."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

LAYER_KEYS = ("0.norm.weight", "0.norm.bias", "0.fn.to_qkv.weight", "0.fn.to_out.0.weight", "0.fn.to_out.0.bias", "1.norm.weight", "1.norm.bias",
              "1.fn.to_kv.weight", "1.fn.to_q.weight", "1.fn.to_out.0.weight", "1.fn.to_out.0.bias", "2.norm.weight", "2.norm.bias",
              "2.fn.net.0.weight", "2.fn.net.0.bias", "2.fn.net.3.weight", "2.fn.net.3.bias")        # in _lib.HphLayerGrads.FIELDS order
DEC_PARTS = ("decpose", "decshape", "deccam", "decexpression")
HEAD = "x_attention_head."


def head_parameter_names(depth: int) -> list:
    """``named_parameters`` keys of every parameter of ``mlp_offset`` and ``x_attention_head``, in the order ``heads_parameters`` returns."""
    names = ["mlp_offset.0.weight", "mlp_offset.0.bias", "mlp_offset.2.weight", "mlp_offset.2.bias"]
    names += [HEAD + n for n in ("cross_queries_x", "cross_queries_y", "cross_values_x", "cross_values_y", "transformer.to_token_embedding.weight",
                                 "transformer.to_token_embedding.bias", "transformer.pos_embedding")]
    for l in range(depth):
        names += [f"{HEAD}transformer.transformer.layers.{l}.{k}" for k in LAYER_KEYS]
    names += [f"{HEAD}{m}.{wb}" for m in DEC_PARTS for wb in ("weight", "bias")]
    return names


def packed_to_parameter_grads(g: dict, layer_grads: list, Cc: int, nb: int, dim: int) -> dict:
    """Gradients in the packed layout of ``mhmr_hph_backward`` -> ``{parameter name: gradient in the parameter's shape}``.
    ``g``: the twelve buffers of ``_lib.HphBackwardDesc.GRADS``; ``layer_grads``: per layer the seventeen of ``HphLayerGrads.FIELDS``.
    Slices drop the zero padding (``tok_w`` columns, ``to_kv`` columns); ``dec_w`` / ``dec_b`` split into the four read-out linears (the
    ``init_*`` folded into ``dec_b`` are buffers); ``tok_b`` is the gradient of the bias AND of ``pos_embedding[0, 0]``, which the pack
    adds into it."""
    out = {"mlp_offset.0.weight": g["g_off1_w"], "mlp_offset.0.bias": g["g_off1_b"], "mlp_offset.2.weight": g["g_off2_w"],
           "mlp_offset.2.bias": g["g_off2_b"], HEAD + "cross_queries_x": g["g_cq_x"], HEAD + "cross_queries_y": g["g_cq_y"],
           HEAD + "cross_values_x": g["g_cv_x"], HEAD + "cross_values_y": g["g_cv_y"],
           HEAD + "transformer.to_token_embedding.weight": g["g_tok_w"][:, : Cc + 318 + nb + 3].contiguous(),
           HEAD + "transformer.to_token_embedding.bias": g["g_tok_b"], HEAD + "transformer.pos_embedding": g["g_tok_b"].reshape(1, 1, dim).clone()}
    for l, row in enumerate(layer_grads):
        for key, field in zip(LAYER_KEYS, _lib.HphLayerGrads.FIELDS):
            t = row[field]
            out[f"{HEAD}transformer.transformer.layers.{l}.{key}"] = t[:, :Cc].contiguous() if field == "to_kv" else t
    a = 0
    for m, n in zip(DEC_PARTS, (318, nb, 3, 10)):
        out[f"{HEAD}{m}.weight"], out[f"{HEAD}{m}.bias"] = g["g_dec_w"][a:a + n].contiguous(), g["g_dec_b"][a:a + n].contiguous()
        a += n
    return out


def layer_grad_shapes(inner: int, dim: int, mlp: int, Kc: int) -> dict:
    """Shapes of the packed per-layer gradient buffers, by field of ``HphLayerGrads``."""
    return {"ln_sa_w": (dim,), "ln_sa_b": (dim,), "to_qkv": (3 * inner, dim), "sa_out_w": (dim, inner), "sa_out_b": (dim,), "ln_ca_w": (dim,),
            "ln_ca_b": (dim,), "to_kv": (2 * inner, Kc), "to_q": (inner, dim), "ca_out_w": (dim, inner), "ca_out_b": (dim,), "ln_ff_w": (dim,),
            "ln_ff_b": (dim,), "ff1_w": (mlp, dim), "ff1_b": (mlp,), "ff2_w": (dim, mlp), "ff2_b": (dim,)}


class _HeadsFunction(torch.autograd.Function):
    """(features or None, head parameters) -> (readout, offset): the values are the ones the forward has already computed."""

    @staticmethod
    def forward(ctx, model, st, features, *params):
        ctx.model, ctx.st = model, st
        ctx.shapes = [tuple(p.shape) for p in params]
        ctx.feat_shape = None if features is None else tuple(features.shape)
        return st["readout"], st["offset"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_readout, g_offset):
        model, st = ctx.model, ctx.st
        need, need_feat = ctx.needs_input_grad[3:], ctx.needs_input_grad[2]
        dev, Pn, P = st["dev"], st["Pn"], st["P"]
        if Pn == 0:      # no person: no contribution, the gradients are zeros (None for the features: autograd's zero)
            return (None, None, None) + tuple(torch.zeros(s, device=dev) if n else None for s, n in zip(ctx.shapes, need))
        model._require_current(st["taken"])
        h = P["hph"]
        L, stream = _lib.lib(), torch.cuda.current_stream(dev).cuda_stream
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        C_, Cc, Kc, G, dim, nb, Ktok, Ndec, inner = P["C"], P["Cc"], P["Kc"], P["G"], h["dim"], h["nb"], h["Ktok"], h["Ndec"], h["inner"]
        shapes = {"g_off1_w": (C_, C_), "g_off1_b": (C_,), "g_off2_w": (2, C_), "g_off2_b": (2,), "g_tok_w": (dim, Ktok), "g_tok_b": (dim,),
                  "g_dec_w": (Ndec, dim), "g_dec_b": (Ndec,), "g_cq_x": (G, Cc), "g_cq_y": (G, Cc), "g_cv_x": (G, Cc), "g_cv_y": (G, Cc)}
        g = {n: f(*s) for n, s in shapes.items()}
        lshapes = layer_grad_shapes(inner, dim, h["mlp"], Kc)
        lgrads, lbufs = (_lib.HphLayerGrads * max(h["depth"], 1))(), []
        for l in range(h["depth"]):
            row = {n: f(*lshapes[n]) for n in _lib.HphLayerGrads.FIELDS}
            for n, t in row.items():
                setattr(lgrads[l], n, t.data_ptr())
            lbufs.append(row)
        g_zc, g_token = f(Pn, C_), f(Pn, Ktok)
        g_feat = f(st["B"] * P["N"], C_) if need_feat else None
        fwd = st["desc"]
        nbytes = _lib.workspace_bytes("mhmr_hph_backward_workspace_bytes", C.byref(fwd), st["B"], Pn)
        wsb = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        g_readout, g_offset = g_readout.to(torch.float32).contiguous(), g_offset.to(torch.float32).contiguous()
        d = _lib.HphBackwardDesc()
        d.fwd = C.pointer(fwd)
        d.ctx16, d.det_y, d.det_x = st["ws"]["ctx16"].data_ptr(), st["det"][1].data_ptr(), st["det"][2].data_ptr()
        d.gstart, d.chunks = st["gstart"].data_ptr(), st["chunks"].data_ptr()
        d.ngroups, d.nmax, d.nchunks, d.P, d.B = st["ngc"], Pn, st["ncc"], Pn, st["B"]
        d.g_readout, d.ldg, d.g_offset = g_readout.data_ptr(), int(g_readout.shape[1]), g_offset.data_ptr()
        for n, t in g.items():
            setattr(d, n, t.data_ptr())
        d.layer_grads = C.cast(lgrads, C.POINTER(_lib.HphLayerGrads))
        d.g_zc, d.g_token, d.workspace, d.workspace_bytes = g_zc.data_ptr(), g_token.data_ptr(), wsb.data_ptr(), nbytes
        d.g_feat, d.ld_feat = _lib.f32p(g_feat), C_
        with model._lock, torch.cuda.device(dev):
            _lib.check(L.mhmr_hph_backward(C.byref(d), stream), "mhmr_hph_backward")
        # the cotangents of the gathered features (rows of the persons), for a backbone backward
        model.heads_feature_grads = {"g_zc": g_zc, "g_token": g_token[:, :Cc]}
        named = packed_to_parameter_grads(g, lbufs, Cc, nb, dim)
        return (None, None, g_feat.view(ctx.feat_shape) if need_feat else None) + tuple(named[n] if k else None for n, k in zip(st["names"], need))


def attach(model, st, features=None, with_params=True):
    """-> (readout, offset) attached to autograd with respect to the head parameters that require grad (``with_params``: train_heads) and
    to ``features`` (the tensor ``Model.forward_features`` was given, when it requires grad); detached values otherwise."""
    names = head_parameter_names(st["P"]["hph"]["depth"])
    params = dict(model.named_parameters())
    st["names"] = names
    with torch.enable_grad():
        return _HeadsFunction.apply(model, st, features, *[params[n] if with_params else params[n].detach() for n in names])


__all__ = ["head_parameter_names", "packed_to_parameter_grads", "layer_grad_shapes", "attach"]
