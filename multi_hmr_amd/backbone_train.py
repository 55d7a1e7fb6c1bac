"""Training the last backbone blocks: the backward of a ViT block and of the self-attention over all tokens of an
image, in fp32 at the fp32 master weights, evaluated at the residual stream the inference forward produced.

The functions here run the block and tail backward of csrc/vit_bwd.hip and the exact attention pair of csrc/attention_f32.hip on device
tensors and allocate their outputs and workspaces.  There is no CPU path.  ``precision="bf16"`` gives the linears
of a block bf16 operands with fp32 accumulation (csrc/linear_bf16.hip), in the recomputed tape and in both backward products; attention,
LayerNorm and the column sums stay exact, and ``"f32"`` is the default.  ``attention="bf16"`` is the independent
switch of the attention tape and backward: bf16 operands, fp32 accumulation, fp32 logits (csrc/attention_bf16.hip;
``attention_bf16_tape`` / ``attention_bf16_backward`` run the pair on its own).  Token rows follow the forward's layout: ``Tp`` rows per
image, patch rows first, the class token at row ``N = T - 1``, padding behind it."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

#: descriptor field (``_lib.VitBlockBackwardDesc.PARAMS``) -> parameter name inside ``backbone.encoder.blocks.<l>``
BLOCK_FIELDS = dict(ln1_w="norm1.weight", ln1_b="norm1.bias", qkv_w="attn.qkv.weight", qkv_b="attn.qkv.bias", proj_w="attn.proj.weight",
                    proj_b="attn.proj.bias", ls1="ls1.gamma", ln2_w="norm2.weight", ln2_b="norm2.bias", fc1_w="mlp.fc1.weight",
                    fc1_b="mlp.fc1.bias", fc2_w="mlp.fc2.weight", fc2_b="mlp.fc2.bias", ls2="ls2.gamma")
ENCODER = "backbone.encoder."


def backbone_parameter_names(depth: int, n: int = 1) -> list:
    """``named_parameters`` keys of the final norm and of the last ``n`` blocks of a ``depth``-block encoder, in the order
    ``Model.backbone_parameters`` returns: norm.weight, norm.bias, then blocks ``depth - n .. depth - 1`` field by field."""
    if not 1 <= n <= depth:
        raise ValueError(f"n must be in [1, {depth}]")
    names = [ENCODER + "norm.weight", ENCODER + "norm.bias"]
    for l in range(depth - n, depth):
        names += [f"{ENCODER}blocks.{l}.{BLOCK_FIELDS[f]}" for f in _lib.VitBlockBackwardDesc.PARAMS]
    return names


#: the four parameters of the token embedding, in the order ``Model.embedding_parameters`` returns and ``embed_backward`` answers
EMBED_FIELDS = dict(g_patch_w="patch_embed.proj.weight", g_patch_b="patch_embed.proj.bias", g_pos="pos_embed", g_cls="cls_token")


def embedding_parameter_names() -> list:
    """``named_parameters`` keys of the token embedding: patch convolution weight and bias, position table, class token.  They receive a
    gradient only when every block is trained (``train_backbone_(depth)``): DESIGN.md section 29."""
    return [ENCODER + n for n in EMBED_FIELDS.values()]


def _f32(t):
    if not t.is_cuda:
        raise _lib.MhmrError("multi_hmr_amd.backbone_train runs only on an MI355X (HIP) tensor; there is no CPU fallback")
    return t.detach().to(torch.float32).contiguous()


def _call(entry, args, dev, stream=None, ws=None):
    """``entry(*args, [workspace, workspace_bytes,] stream)`` on ``stream`` (default: the current stream of ``dev``), checked under the
    entry's name.  ``ws`` = (the entry's workspace-size entry, *its arguments): a uint8 workspace of that size is allocated on ``dev``."""
    if ws is not None:
        nbytes = _lib.workspace_bytes(*ws)
        wsb = torch.empty(nbytes, dtype=torch.uint8, device=dev)      # alive until the call is enqueued
        args += (wsb.data_ptr(), nbytes)
    stream = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
    _lib.check(getattr(_lib.lib(), entry)(*args, stream), entry)


def _attention_ws(kind, B, Tp, Cd, H):
    """``_call``'s ``ws`` of the attention backward of ``kind`` ("f32" or "bf16"; the bf16 tape takes the same workspace)."""
    return ("mhmr_attention_bf16_workspace_bytes", B, Tp, Cd, H) if kind == "bf16" else ("mhmr_attention_f32_backward_workspace_bytes", B, Tp, H)


def _attention_tape(kind, qkv, B, T, Tp, H, stream):
    qkv = _f32(qkv)
    dev, Cd = qkv.device, qkv.shape[1] // 3
    out32 = torch.empty(B * Tp, Cd, dtype=torch.float32, device=dev)
    lse = torch.empty(B, H, Tp, dtype=torch.float32, device=dev)
    _call(f"mhmr_attention_{kind}_tape", (qkv.data_ptr(), out32.data_ptr(), lse.data_ptr(), B, T, Tp, Cd, H), dev, stream,
          _attention_ws(kind, B, Tp, Cd, H) if kind == "bf16" else None)
    return out32, lse


def _attention_backward(kind, qkv, out32, lse, dO, B, T, Tp, H, stream, dqkv):
    qkv, out32, lse = _f32(qkv), _f32(out32), _f32(lse)
    dev, Cd = qkv.device, qkv.shape[1] // 3
    if dO.dtype != torch.float32 or dO.stride(-1) != 1:
        dO = _f32(dO)
    if dqkv is None:
        dqkv = torch.empty(B * Tp, 3 * Cd, dtype=torch.float32, device=dev)
    _call(f"mhmr_attention_{kind}_backward", (qkv.data_ptr(), out32.data_ptr(), lse.data_ptr(), dO.data_ptr(), dO.stride(0), dqkv.data_ptr(), B,
                                              T, Tp, Cd, H), dev, stream, _attention_ws(kind, B, Tp, Cd, H))
    return dqkv


def attention_tape(qkv, B, T, Tp, H, stream=None):
    """``mhmr_attention_f32_tape``: qkv [B*Tp, 3C] fp32 -> (out32 [B*Tp, C], lse [B, H, Tp])."""
    return _attention_tape("f32", qkv, B, T, Tp, H, stream)


def attention_backward(qkv, out32, lse, dO, B, T, Tp, H, stream=None, dqkv=None):
    """``mhmr_attention_f32_backward``: -> dqkv [B*Tp, 3C] with respect to the un-scaled Q, K and V."""
    return _attention_backward("f32", qkv, out32, lse, dO, B, T, Tp, H, stream, dqkv)


def attention_bf16_tape(qkv, B, T, Tp, H, stream=None):
    """``mhmr_attention_bf16_tape``: qkv [B*Tp, 3C] fp32 -> (out32 [B*Tp, C], lse [B, H, Tp]) with bf16 operands."""
    return _attention_tape("bf16", qkv, B, T, Tp, H, stream)


def attention_bf16_backward(qkv, out32, lse, dO, B, T, Tp, H, stream=None, dqkv=None):
    """``mhmr_attention_bf16_backward``: -> dqkv [B*Tp, 3C] with respect to the un-scaled Q, K and V; ``out32`` and ``lse`` are the tape's."""
    return _attention_backward("bf16", qkv, out32, lse, dO, B, T, Tp, H, stream, dqkv)


def block_tensors(block, device=None) -> dict:
    """{descriptor field: fp32 contiguous tensor} of a block module with DINOv2's parameter names (the nn.Parameters themselves when they
    already are fp32, contiguous and on the device)."""
    named = dict(block.named_parameters())
    out = {}
    for f, n in BLOCK_FIELDS.items():
        t = named[n].detach()
        out[f] = t.to(device=device if device is not None else t.device, dtype=torch.float32).contiguous()
    return out


def fill_block_desc(d, params: dict, grads: dict, B, T, Tp, Cd, H):
    """Set the shape, the fourteen master tensors and the fourteen gradient buffers of a ``_lib.VitBlockBackwardDesc``."""
    d.B, d.T, d.Tp, d.C, d.H = B, T, Tp, Cd, H
    for f in _lib.VitBlockBackwardDesc.PARAMS:
        setattr(d, f, params[f].data_ptr())
        setattr(d, "g_" + f, grads[f].data_ptr())
    return d


def linear_bf16(X, W, bias=None, stream=None):
    """``mhmr_linear_bf16``: Y [M, N] = r(X [M, K]) r(W [N, K])^T + bias, bf16 operands (round to nearest even), fp32 accumulation."""
    X, W = _f32(X), _f32(W)
    bias = None if bias is None else _f32(bias)
    (M, K), N = X.shape, W.shape[0]
    Y = torch.empty(M, N, dtype=torch.float32, device=X.device)
    _call("mhmr_linear_bf16", (X.data_ptr(), K, W.data_ptr(), K, _lib.ptr(bias), Y.data_ptr(), N, M, N, K), X.device, stream,
          ("mhmr_linear_bf16_workspace_bytes", M, N, K))
    return Y


def linear_bf16_backward_input(dY, W, dR=None, stream=None):
    """``mhmr_linear_bf16_backward_input``: dX [M, K] = r(dY [M, N]) r(W [N, K]) (+ dR, added in fp32)."""
    dY, W = _f32(dY), _f32(W)
    dR = None if dR is None else _f32(dR)
    (M, N), K = dY.shape, W.shape[1]
    dX = torch.empty(M, K, dtype=torch.float32, device=dY.device)
    _call("mhmr_linear_bf16_backward_input", (dY.data_ptr(), N, W.data_ptr(), K, _lib.ptr(dR), K, dX.data_ptr(), K, M, N, K), dY.device, stream,
          ("mhmr_linear_bf16_workspace_bytes", M, N, K))
    return dX


def linear_bf16_backward_weight(dY, X, stream=None):
    """``mhmr_linear_bf16_backward_weight``: (dW [N, K] = r(dY [M, N])^T r(X [M, K]), db [N] = the fp64 column sums of the unrounded dY)."""
    dY, X = _f32(dY), _f32(X)
    (M, N), K = dY.shape, X.shape[1]
    dW = torch.empty(N, K, dtype=torch.float32, device=dY.device)
    db = torch.empty(N, dtype=torch.float32, device=dY.device)
    _call("mhmr_linear_bf16_backward_weight", (dY.data_ptr(), N, X.data_ptr(), K, dW.data_ptr(), K, db.data_ptr(), M, N, K), dY.device, stream,
          ("mhmr_linear_bf16_workspace_bytes", M, N, K))
    return dW, db


def block_backward(params: dict, x_in, g_out, B, T, Tp, H, stream=None, precision="f32", attention="f32"):
    """``mhmr_vit_block_backward`` on device tensors: ``params`` = {descriptor field: fp32 tensor} (``block_tensors``), x_in and g_out
    [B*Tp, C] -> (g_in [B*Tp, C], {field: gradient of the parameter's shape}).  ``precision``: "f32" (the exact linears) or "bf16"
    (bf16 operands, fp32 accumulation).  ``attention``: the same two names for the attention tape and backward
    (DESIGN.md section 31)."""
    prec, att = _lib.bwd_precision(precision), _lib.attn_precision(attention)
    x_in, g_out = _f32(x_in), _f32(g_out)
    dev, Cd = x_in.device, x_in.shape[1]
    grads = {f: torch.empty_like(params[f]) for f in _lib.VitBlockBackwardDesc.PARAMS}
    g_in = torch.empty_like(x_in)
    nbytes = _lib.workspace_bytes("mhmr_vit_block_backward_workspace_bytes_pa", B, Tp, Cd, prec, att)
    wsb = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d = fill_block_desc(_lib.VitBlockBackwardDesc(), params, grads, B, T, Tp, Cd, H)
    d.linear_precision = prec
    d.x_in, d.g_out, d.g_in, d.workspace, d.workspace_bytes = x_in.data_ptr(), g_out.data_ptr(), g_in.data_ptr(), wsb.data_ptr(), nbytes
    _call("mhmr_vit_block_backward_a", (C.byref(d), att), dev, stream)
    return g_in, grads


def tail_backward(norm_w, norm_b, blocks: list, tap, resid, g_feat, B, N, Tp, H, stream=None, precision="f32", attention="f32"):
    """``mhmr_vit_tail_backward`` on device tensors: final norm + the blocks of ``blocks`` ([{descriptor field: fp32 tensor}], first block
    first) at the tapped streams ``tap [n, B*Tp, C]``; ``resid [B*Tp, C]`` the stream the final norm read; ``g_feat [B*N, C]``
    -> (g_stream [B*Tp, C], g_norm_w, g_norm_b, [{field: gradient}] per block).  ``precision``, ``attention``: as in ``block_backward``, for every block."""
    prec, att = _lib.bwd_precision(precision), _lib.attn_precision(attention)
    n, dev, Cd = len(blocks), resid.device, resid.shape[-1]
    g_feat = _f32(g_feat).reshape(B * N, Cd)
    assert tap.dtype == resid.dtype == torch.float32 and tap.is_contiguous() and resid.is_contiguous() and tap.numel() == n * B * Tp * Cd
    grads = [{f: torch.empty_like(b[f]) for f in _lib.VitBlockBackwardDesc.PARAMS} for b in blocks]
    descs = (_lib.VitBlockBackwardDesc * n)()
    for i in range(n):
        fill_block_desc(descs[i], blocks[i], grads[i], B, N + 1, Tp, Cd, H)
    g_norm_w, g_norm_b = torch.empty_like(norm_w), torch.empty_like(norm_b)
    g_stream = torch.empty(B * Tp, Cd, dtype=torch.float32, device=dev)
    nbytes = _lib.workspace_bytes("mhmr_vit_tail_backward_workspace_bytes_pa", B, Tp, Cd, prec, att)
    wsb = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d = _lib.VitTailBackwardDesc()
    d.linear_precision = prec
    d.B, d.N, d.T, d.Tp, d.C, d.H, d.n = B, N, N + 1, Tp, Cd, H, n
    d.norm_w, d.norm_b, d.blocks = norm_w.data_ptr(), norm_b.data_ptr(), C.cast(descs, C.POINTER(_lib.VitBlockBackwardDesc))
    d.tap, d.resid, d.g_feat = tap.data_ptr(), resid.data_ptr(), g_feat.data_ptr()
    d.g_norm_w, d.g_norm_b, d.g_stream, d.workspace, d.workspace_bytes = g_norm_w.data_ptr(), g_norm_b.data_ptr(), g_stream.data_ptr(), wsb.data_ptr(), nbytes
    _call("mhmr_vit_tail_backward_a", (C.byref(d), att), dev, stream)
    return g_stream, g_norm_w, g_norm_b, grads


def embed_backward(x, g_stream, B, G, M, Tp, stream=None):
    """``mhmr_vit_embed_backward`` on device tensors: ``x [B, 3, 14 G, 14 G]`` the forward's input, ``g_stream [B*Tp, C]`` the cotangent of the
    stream entering block 0 (``tail_backward`` over every block), ``M`` the edge of the stored position table
    -> {g_patch_w [C, 588], g_patch_b [C], g_pos [1 + M*M, C], g_cls [C]}."""
    import numpy as np
    from . import packing
    x, g_stream = _f32(x), _f32(g_stream)
    dev, Cd = g_stream.device, g_stream.shape[1]
    assert tuple(x.shape) == (B, 3, 14 * G, 14 * G) and g_stream.shape[0] == B * Tp
    interp = torch.from_numpy(np.ascontiguousarray(packing.pos_embed_matrix(M, G))).to(dev)
    out = dict(g_patch_w=torch.empty(Cd, 588, dtype=torch.float32, device=dev), g_patch_b=torch.empty(Cd, dtype=torch.float32, device=dev),
               g_pos=torch.empty(1 + M * M, Cd, dtype=torch.float32, device=dev), g_cls=torch.empty(Cd, dtype=torch.float32, device=dev))
    nbytes = _lib.workspace_bytes("mhmr_vit_embed_backward_workspace_bytes", B, G, M, Cd)
    wsb = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d = _lib.VitEmbedBackwardDesc()
    d.B, d.S, d.G, d.M, d.Tp, d.C = B, 14 * G, G, M, Tp, Cd
    d.x, d.g_stream, d.interp, d.workspace, d.workspace_bytes = x.data_ptr(), g_stream.data_ptr(), interp.data_ptr(), wsb.data_ptr(), nbytes
    for f, t in out.items():
        setattr(d, f, t.data_ptr())
    _call("mhmr_vit_embed_backward", (C.byref(d),), dev, stream)
    return out


def model_tail_backward(model, P, ws, B, g_feat, n, x=None):
    """The tail backward of ``model`` on the workspace of its last ``train_backbone`` forward of batch size B: the fp32 master weights
    are the ``nn.Parameter``s themselves; one call per image block of the workspace (``Model._nsplit``), the parameter gradients of the
    blocks added in block order.  -> {parameter name: gradient} for ``backbone_parameter_names(depth, n)``.
    ``x`` (the forward's fp32 input, ``n == depth`` only): every image block's ``g_stream`` also goes through ``embed_backward`` with that
    block's images, and the dict gains the gradients of ``embedding_parameter_names()`` (shaped [C, 588], [C], [1 + M*M, C], [C])."""
    enc = model.backbone.encoder
    depth, N, Cd, H = len(enc.blocks), P["N"], P["C"], P["H"]
    if ws.get("tap_blocks") != n:
        raise _lib.MhmrError(f"Model: this workspace taps {ws.get('tap_blocks')} blocks, the backward needs {n}")
    dev = ws["feat32"].device
    norm_w, norm_b = _f32(enc.norm.weight), _f32(enc.norm.bias)
    blocks = [block_tensors(enc.blocks[l], dev) for l in range(depth - n, depth)]
    g_feat = _f32(g_feat).reshape(B * N, Cd)
    if x is not None and n != depth:
        raise _lib.MhmrError(f"Model: the embedding gradient needs every block's backward ({depth}), this one runs {n}")
    names = backbone_parameter_names(depth, n) + (embedding_parameter_names() if x is not None else [])
    M = int(round((enc.pos_embed.shape[1] - 1) ** 0.5))
    total = None
    for part in ws["parts"]:
        Bh, i0, bufs = part["B"], part["img0"], part["bufs"]
        g_stream, gw, gb, grads = tail_backward(norm_w, norm_b, blocks, bufs["tap"], bufs["resid"], g_feat[i0 * N:(i0 + Bh) * N], Bh, N, ws["Tp"], H,
                                                precision=model._backbone_precision, attention=model._backbone_attention)
        flat = [gw, gb] + [g[f] for g in grads for f in _lib.VitBlockBackwardDesc.PARAMS]
        if x is not None:
            ge = embed_backward(x[i0:i0 + Bh], g_stream, Bh, P["G"], M, ws["Tp"])
            flat += [ge[f] for f in EMBED_FIELDS]
        total = flat if total is None else [a + b for a, b in zip(total, flat)]
    return dict(zip(names, total))


class _TailFunction(torch.autograd.Function):
    """(the parameters of backbone_parameter_names, then -- when the embedding is trained -- of embedding_parameter_names) -> features
    [B, N, C]: the values are the ones the forward has already computed."""

    @staticmethod
    def forward(ctx, model, st, *params):
        ctx.model, ctx.st = model, st
        return st["features"]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_feat):
        model, st = ctx.model, ctx.st
        P, ws = st["P"], st["ws"]
        model._require_current(st["taken"])
        need = ctx.needs_input_grad[2:]
        embed = any(need[len(st["named"]) - len(EMBED_FIELDS):]) if st["x"] is not None else False
        with model._lock, torch.cuda.device(st["dev"]):
            grads = model_tail_backward(model, P, ws, st["B"], g_feat, st["n"], st["x"] if embed else None)
        need = [want and k in grads for (k, _), want in zip(st["named"], need)]
        return (None, None) + tuple(grads[k].view_as(p) if want else None for (k, p), want in zip(st["named"], need))


def embeddings_on(model) -> bool:
    """Some embedding parameter of ``model`` requires grad.  ``ValueError`` when ``train_backbone_``'s n then is not the depth: the gradient
    reaches the embedding only through every block."""
    if not any(p.requires_grad for p in model.embedding_parameters()):
        return False
    depth = len(model.backbone.encoder.blocks)
    if model._backbone_n != depth:
        raise ValueError(f"embedding parameters require grad, but train_backbone_({model._backbone_n}) stops the backward in front of block "
                         f"{depth - model._backbone_n}: call train_backbone_({depth}) (or train_embeddings_(False))")
    return True


def attach(model, P, ws, B, x=None):
    """-> the features of the forward that has just run on ``ws`` (a clone, [B, N, C]) attached to autograd with respect to
    ``model.backbone_parameters(n)``: the node that hands the feature cotangent to ``mhmr_vit_tail_backward``.  ``x``: the forward's
    contiguous fp32 input when the embedding is trained (``embeddings_on``) -- the node then also takes ``model.embedding_parameters()`` and
    keeps a reference to ``x``, which the caller must not write into before ``backward()``."""
    n = model._backbone_n
    params = dict(model.named_parameters())
    names = backbone_parameter_names(len(model.backbone.encoder.blocks), n) + (embedding_parameter_names() if x is not None else [])
    named = [(k, params[k]) for k in names]
    st = dict(P=P, ws=ws, B=B, n=n, dev=ws["feat32"].device, taken=model._take(P, ws, "backbone_generation"), x=x,
              named=named, features=ws["feat32"].view(B, P["N"], P["C"]).clone())
    with torch.enable_grad():
        return _TailFunction.apply(model, st, *[p for _, p in named])


__all__ = ["BLOCK_FIELDS", "EMBED_FIELDS", "backbone_parameter_names", "embedding_parameter_names", "attention_tape", "attention_backward",
           "attention_bf16_tape", "attention_bf16_backward", "block_tensors", "linear_bf16", "linear_bf16_backward_input",
           "linear_bf16_backward_weight", "block_backward", "tail_backward", "embed_backward", "model_tail_backward", "embeddings_on", "attach"]
