"""Oracle of the token-embedding backward: ``DinoVisionTransformer.prepare_tokens`` restated in a chosen dtype --
``F.conv2d`` for the patches and ``F.interpolate(..., mode="bicubic", scale_factor=(s, s))`` for the position table, both applied IN that
dtype (oracle.dinov2_ref.interpolate_pos_embed casts to fp32 inside, which would leave 1e-7 in an fp64 reference) -- and its gradients by
torch autograd.

Tokens come in the reference's order, [B, 1 + N, C] with the class token first; the stream cotangent comes in the library's,
[B*Tp, C] with the N patch rows of an image first, its class row at N and padding behind it (never read here)."""
import math

import torch
import torch.nn.functional as F

PATCH = 14
NAMES = ("g_patch_w", "g_patch_b", "g_pos", "g_cls")


def interpolate(pos_embed, G, offset=0.1):
    """pos_embed [1, 1 + M*M, C] -> [1, 1 + G*G, C] in pos_embed's own dtype; for G == M the table is returned untouched."""
    n = pos_embed.shape[1] - 1
    M = int(round(math.sqrt(n)))
    assert M * M == n
    if G == M:
        return pos_embed
    C = pos_embed.shape[-1]
    s = float(G + offset) / M
    patch = F.interpolate(pos_embed[:, 1:].reshape(1, M, M, C).permute(0, 3, 1, 2), mode="bicubic", antialias=False, scale_factor=(s, s))
    assert patch.shape[-2:] == (G, G) and patch.dtype == pos_embed.dtype
    return torch.cat((pos_embed[:, :1], patch.permute(0, 2, 3, 1).reshape(1, G * G, C)), dim=1)


def prepare_tokens(x, patch_w, patch_b, cls_token, pos_embed):
    """x [B, 3, S, S], patch_w [C, 3, 14, 14], patch_b [C], cls_token [1, 1, C], pos_embed [1, 1 + M*M, C], all of one dtype
    -> tokens [B, 1 + N, C], class token first."""
    B, _, H, W = x.shape
    assert H == W and H % PATCH == 0
    t = F.conv2d(x, patch_w, patch_b, stride=PATCH).flatten(2).transpose(1, 2)
    t = torch.cat((cls_token.expand(B, -1, -1), t), dim=1)
    return t + interpolate(pos_embed, H // PATCH)


def make_params(C, M, seed):
    """fp32 parameters of an embedding of width C with an M x M position table (the gradients do not depend on their values: the function
    is linear in them)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.empty(*s).normal_(0, 1, generator=g)
    return dict(patch_w=rn(C, 3, PATCH, PATCH) * (3 * PATCH * PATCH) ** -0.5, patch_b=0.1 * rn(C), cls_token=0.02 * rn(1, 1, C),
                pos_embed=0.02 * rn(1, 1 + M * M, C))


def stream_to_tokens(g_stream, B, N, Tp):
    """The cotangent of the tokens, class first, from g_stream [B*Tp, C]: rows > N of an image are dropped."""
    g = g_stream.reshape(B, Tp, -1)
    return torch.cat((g[:, N:N + 1], g[:, :N]), dim=1)


def embed_backward(x, params, g_stream, B, G, Tp, dtype=torch.float64):
    """Autograd of ``prepare_tokens`` in ``dtype`` against g_stream [B*Tp, C] -> {g_patch_w [C, 588], g_patch_b [C], g_pos [1 + M*M, C],
    g_cls [C]} in ``dtype``."""
    p = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in params.items()}
    tok = prepare_tokens(x.to(dtype), p["patch_w"], p["patch_b"], p["cls_token"], p["pos_embed"])
    (tok * stream_to_tokens(g_stream.to(dtype), B, G * G, Tp)).sum().backward()
    C = tok.shape[-1]
    return dict(g_patch_w=p["patch_w"].grad.reshape(C, 3 * PATCH * PATCH), g_patch_b=p["patch_b"].grad, g_pos=p["pos_embed"].grad[0],
                g_cls=p["cls_token"].grad.reshape(C))
