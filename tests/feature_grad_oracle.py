"""TEST INFRASTRUCTURE: the cotangent of the features restated in torch on the CPU, parametrised by dtype and
differentiated by autograd -- the reference of ``Model.forward_features``'s ``features.grad``.

The heads' share is ``hph_bwd_oracle.head_forward`` with the features as the ONE leaf: ``zc`` and ``zq`` are gathered from it, the context
is built from it (rounded to the 16-bit operand type straight-through, the value tables added at the detected cells).  The detector's
share restates DESIGN.md section 22 (``detect_bwd_oracle.scores``): the device's stored hidden layer is taken as given in value and
mask, the first-layer weight and the context are rounded to the 16-bit type, the context straight-through.  The two parts are returned
separately and summed."""
from __future__ import annotations

import torch

import detect_bwd_oracle as do
import hph_bwd_oracle as ho


def product(left, w16, dtype):
    """out[m][c] = sum_n left[m][n] w16[n][c] in ``dtype`` (the 16-bit weight is an exact number)."""
    return left.to(dtype) @ w16.to(dtype)


def detector_term(hid16, w16, w2, b2, gs, clamped, dtype):
    """d sum(gs * scores) / d X [rows, C] of the detection head with the hidden layer taken as given: W1 = w16 [C, C] (16-bit values)."""
    rows, C_ = hid16.shape
    X = torch.zeros(rows, C_, dtype=dtype, requires_grad=True)          # the mask and the values come from hid16: X's value is not read
    s = do.scores(X, w16.to(dtype), torch.zeros(C_, dtype=dtype), w2.to(dtype), b2.to(dtype), hidden=hid16.to(dtype), clamped=clamped)
    (g,) = torch.autograd.grad((s * gs.to(dtype)).sum(), X)
    return g


def feature_grads(sd_all, feat, K, idx, cot_readout, cot_offset, cot_scores, hid16, depth, heads, G, precision, dtype):
    """{"heads", "detector", "total"}: gradients [B, N, C] of sum(cot_readout * readout) + sum(cot_offset * offset) (heads) and of
    sum(cot_scores * scores) (detector) with respect to the features, in ``dtype``.  A cotangent of None leaves its part out (zeros).
    ``hid16`` [B N, C]: the device's stored hidden layer of mlp_classif."""
    tdt = ho.TDT[precision]
    B, N, C_ = feat.shape
    out = {}
    Pn = int(idx[0].shape[0])
    if Pn > 0 and (cot_readout is not None or cot_offset is not None):
        sd = ho.head_operands(sd_all, precision, dtype)
        f = feat.to(dtype).clone().requires_grad_()
        rows = idx[1] * G + idx[2]
        z_K = ho.embedd_camera(K.to(dtype), G).reshape(B, N, -1)
        zc = f[idx[0], rows]
        zq = torch.cat([f[idx[0], rows], z_K[idx[0], rows]], 1)
        readout, offset = ho.head_forward(sd, zc, zq, f, K, idx, depth, heads, G, precision)
        s = readout.new_zeros(())
        if cot_readout is not None:
            s = s + (readout * cot_readout.to(dtype)).sum()
        if cot_offset is not None:
            s = s + (offset * cot_offset.to(dtype)).sum()
        (out["heads"],) = torch.autograd.grad(s, f)
    else:
        out["heads"] = torch.zeros(B, N, C_, dtype=dtype)
    if cot_scores is not None:
        f = feat.to(dtype).clone().requires_grad_()
        X = ho._round_st(f.reshape(B * N, C_), tdt)
        W1 = sd_all["mlp_classif.0.weight"].to(tdt).to(dtype)
        s = do.scores(X, W1, sd_all["mlp_classif.0.bias"].to(dtype), sd_all["mlp_classif.2.weight"].reshape(-1).to(dtype),
                      sd_all["mlp_classif.2.bias"].to(dtype), hidden=hid16.to(dtype), clamped=True)
        (out["detector"],) = torch.autograd.grad((s * cot_scores.reshape(-1).to(dtype)).sum(), f)
    else:
        out["detector"] = torch.zeros(B, N, C_, dtype=dtype)
    out["total"] = out["heads"] + out["detector"]
    return out
