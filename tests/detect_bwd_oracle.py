"""TEST INFRASTRUCTURE: the two layers of the detection head mlp_classif restated in torch on the CPU, parametrised by dtype and
differentiated by autograd -- the reference of csrc/detect_bwd.hip.

The kernels differentiate the forward as its kernels evaluate it: the stored hidden layer hid16, the context operand ctx16 and the
ReLU mask hid16 > 0 are TAKEN AS GIVEN.  So the first layer enters the graph as ``hid16 + (Z mask - (Z mask).detach())`` with
``Z = X W1^T + b1``: its value is hid16, its derivative is that of ``Z mask``, and autograd yields exactly
    dl = gs p (1 - p) [clamp mask],  db2 = sum dl,  dw2 = dl^T hid16,  db1 = w2 * (dl^T mask),  dW1 = (w2 * (dl mask))^T X.
``hidden=None`` is the true function instead (hid = relu(Z), no rounding): what a finite difference can follow."""
from __future__ import annotations

import torch

from hph_bwd_oracle import TDT, four_x  # noqa: F401  (four_x: the 4x rule, shared with the decoder's tests)

CLAMP_LO, CLAMP_HI = 1e-4, 1.0 - 1e-4


def scores(X, W1, b1, w2, b2, hidden=None, clamped=True):
    """scores [M] of the two layers.  X [M, C]; W1 [C, C]; b1 [C]; w2 [C]; b2 [1] or 0-d; ``hidden``: the stored hidden layer [M, C]
    taken as given (with its own mask), or None for relu(Z)."""
    Z = X @ W1.T + b1
    if hidden is None:
        hid = torch.relu(Z)
    else:
        Zm = Z * (hidden > 0).to(Z.dtype)
        hid = hidden + (Zm - Zm.detach())
    p = torch.sigmoid(hid @ w2 + b2.reshape(()))
    return torch.clamp(p, CLAMP_LO, CLAMP_HI) if clamped else p


def grads(X, hidden, W1, b1, w2, b2, gs, clamped, dtype):
    """(dW1 [C, C], db1 [C], dw2 [C], db2 [1]) of sum(gs * scores) in ``dtype``, hidden taken as given."""
    leaves = [t.detach().to(dtype).clone().requires_grad_() for t in (W1, b1, w2, b2.reshape(1))]
    s = scores(X.to(dtype), *leaves, hidden=hidden.to(dtype), clamped=clamped)
    return torch.autograd.grad((s * gs.to(dtype)).sum(), leaves)


def logits64(hidden, w2, b2):
    """The fp64 logits and probabilities of the given hidden layer (the input conditions of the tests are stated on these)."""
    s = hidden.double() @ w2.double() + b2.double().reshape(())
    return s, torch.sigmoid(s)


def clamp_margin(p):
    """Relative distance of each p from the nearer clamp bound, measured from the saturation that bound guards: |p / 1e-4 - 1| below,
    |(1 - p) / 1e-4 - 1| above.  (Measured on p itself, every row beyond the upper bound would count as 'at the bound'.)"""
    return torch.minimum((p / CLAMP_LO - 1).abs(), ((1 - p) / (1 - CLAMP_HI) - 1).abs())
