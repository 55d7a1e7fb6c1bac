"""-m "not gpu": the host side of the detection-head backward (csrc/detect_bwd.hip, multi_hmr_amd/detect_train.py)
-- header / binding agree, the entry validates before any launch (so every case runs without a GPU), the workspace bound that keeps the
hidden layer's [rows, C] cotangent out of memory, the Python switches on a CPU model, and the oracle of tests/detect_bwd_oracle.py pinned
in fp64 against central finite differences."""
import os
import re

import pytest
import torch

import detect_bwd_oracle as do
from multi_hmr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE = -1, -2
ENTRIES = {"mhmr_detect_backward_workspace_bytes", "mhmr_detect_backward"}
PTR = 64          # non-null, never dereferenced: validation comes before any launch
ARGS = ("hid16", "ldh", "ctx16", "ldx", "w2", "b2", "gs", "rows", "C", "clamped", "dtype", "g_w1", "g_b1", "g_w2", "g_b2", "ws", "nbytes", "stream")


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_entries_are_declared_bound_and_additive(L):
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    assert ENTRIES <= declared and ENTRIES <= set(_lib._SIGS)
    assert declared == set(_lib.EXPORTS)
    assert all(hasattr(L, n) for n in ENTRIES)
    assert "#define MHMR_VERSION 106" in header and _lib.VERSION == 106 and L.mhmr_version() == 106      # additive entries: the version stays
    assert "detect_bwd.hip" in _lib.SOURCES
    assert len(_lib._SIGS["mhmr_detect_backward"][0]) == len(ARGS)


def test_validation_precedes_every_launch(L):
    base = dict(hid16=PTR, ldh=384, ctx16=PTR, ldx=512, w2=PTR, b2=PTR, gs=PTR, rows=515, C=384, clamped=1, dtype=_lib.DT_F16, g_w1=PTR, g_b1=PTR,
                g_w2=PTR, g_b2=PTR, ws=PTR, nbytes=1 << 40, stream=None)
    call = lambda **o: L.mhmr_detect_backward(*[{**base, **o}[k] for k in ARGS])
    assert call(rows=-1) == BAD_ARG and L.mhmr_detect_backward_workspace_bytes(-1, 384) == BAD_ARG
    for bad in ("hid16", "ctx16", "w2", "b2", "gs", "g_w1", "g_b1", "g_w2", "g_b2", "ws"):
        assert call(**{bad: None}) == BAD_ARG, bad
    need = L.mhmr_detect_backward_workspace_bytes(515, 384)
    assert need > 0 and call(nbytes=need - 1) == BAD_ARG
    for bad in (dict(C=0), dict(C=-128), dict(C=192), dict(C=200), dict(ldh=383), dict(ldx=383), dict(dtype=2), dict(dtype=-1), dict(ldh=385),
                dict(C=16384 + 128, ldh=1 << 20, ldx=1 << 20), dict(rows=512 * 65535 + 1)):
        assert call(**bad) == BAD_SHAPE, bad
    for c in (0, 192, -128):
        assert L.mhmr_detect_backward_workspace_bytes(515, c) == BAD_SHAPE
    # outputs are written for rows == 0 as well, so they are required there too (the inputs are not)
    for bad in ("g_w1", "g_b1", "g_w2", "g_b2"):
        assert call(rows=0, **{bad: None}) == BAD_ARG, bad


@pytest.mark.parametrize("rows,C_", [(0, 128), (1, 128), (515, 384), (8300, 1024), (131072, 1024)])
def test_workspace_never_holds_a_rows_by_C_array(L, rows, C_):
    """At most 16 C C 4 (the slice partials of dW1) + 4 rows (dl) + O(slices C): 16 C bytes for each of the ceil(rows / 512) first-stage
    slices of the column sums (+ 8 for db2, + three 256-byte alignments).  Nothing grows like rows x C x 4."""
    got = L.mhmr_detect_backward_workspace_bytes(rows, C_)
    slices = -(-rows // 512)
    bound = 16 * C_ * C_ * 4 + 4 * rows + (16 * C_ + 8) * slices + 3 * 256
    print(f"rows {rows} C {C_}: workspace {got} bytes, bound {bound}, a [rows, C] fp32 array {rows * C_ * 4}")
    assert 0 <= got <= bound
    assert got >= min(16, slices) * C_ * C_ * 4 + 4 * rows
    if rows == 131072:
        assert got < rows * C_ * 4 // 7                     # 71 MB against the 512 MB of a materialised cotangent


def test_model_switches_on_a_cpu_model():
    """detection_parameters() is mlp_classif, off by default; heads_parameters() keeps its contents; train_detection outside training mode
    is a ValueError before anything touches a device."""
    import synthetic
    from multi_hmr_amd import Model
    from multi_hmr_amd.heads_train import head_parameter_names
    m = Model(backbone="dinov2_vits14", img_size=224, smplx_data=synthetic.make_smplx_data(seed=0), mean_params=synthetic.make_mean_params(seed=0),
              backbone_depth=1)
    det = m.detection_parameters()
    names = {k for k, p in m.named_parameters() if any(p is q for q in det)}
    assert names == {"mlp_classif.0.weight", "mlp_classif.0.bias", "mlp_classif.2.weight", "mlp_classif.2.bias"} and len(det) == 4
    assert not any(p.requires_grad for p in m.parameters())
    assert m.train_detection_(True) is m
    assert {k for k, p in m.named_parameters() if p.requires_grad} == names
    assert not any(p.requires_grad for p in m.heads_parameters())
    assert not names & set(head_parameter_names(m.xat_depth))
    m.train_detection_(False)
    assert not any(p.requires_grad for p in m.parameters())
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 224, 224), train_detection=True)
    with pytest.raises(_lib.MhmrError):                   # a CPU tensor: no fallback
        m(torch.zeros(1, 3, 224, 224), idx=None, K=torch.eye(3)[None], is_training=True, train_detection=True)


# ------------------------------------------------------------------------------------------------------ the oracle itself
def _seeded_case(rows=37, C_=128, seed=60):
    """fp64 operands whose pre-activations are SEEDED: Z0 is drawn first (|Z0| in [0.01, 1], random signs) and X solved from
    X W1^T + b1 = Z0, so no Z lies near the ReLU kink; rows 0-2 / 3-5 are pushed beyond the upper / lower clamp bound."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.empty(*s, dtype=torch.float64).normal_(0, 1, generator=g)
    W1 = torch.eye(C_, dtype=torch.float64) + 0.3 * rn(C_, C_) / C_ ** 0.5
    b1, w2, b2 = 0.1 * rn(C_), rn(C_) / C_ ** 0.5, 0.2 * rn(1)
    mag = 0.01 + 0.99 * torch.rand(rows, C_, generator=g, dtype=torch.float64)
    Z0 = mag * torch.where(torch.rand(rows, C_, generator=g) < 0.5, -1.0, 1.0).double()
    for r in range(6):                                    # aligned with +-w2: logits of about +-12
        sign = 1.0 if r < 3 else -1.0
        pos = (sign * w2) > 0
        k = (12.0 + 0.3 * r) / float((w2[pos] ** 2).sum())
        Z0[r] = torch.where(pos, torch.clamp(k * sign * w2, min=0.01), -mag[r])
    X = torch.linalg.solve(W1, (Z0 - b1).T).T
    gs = rn(rows)
    return X, W1, b1, w2, b2, gs


def test_oracle_against_finite_differences():
    """Central differences of the TRUE function (hid = relu(Z)) along four seeded directions of (W1, b1, w2, b2) against the oracle's
    straight-through gradients at hidden = relu(Z); gate 1e-6 relative.  The two input conditions are asserted first."""
    X, W1, b1, w2, b2, gs = _seeded_case()
    Z = X @ W1.T + b1
    hidden = torch.relu(Z)
    s, p = do.logits64(hidden, w2, b2)
    print(f"min |Z| {float(Z.abs().min()):.3e}; clamp margin {float(do.clamp_margin(p).min()):.3e}; rows beyond the clamp: "
          f"{int((p > do.CLAMP_HI).sum())} above, {int((p < do.CLAMP_LO).sum())} below")
    assert float(Z.abs().min()) > 1e-3, "no pre-activation within 1e-3 of the ReLU kink"
    assert float(do.clamp_margin(p).min()) > 1e-2, "no p within 1 % of a clamp bound"
    assert int((p > do.CLAMP_HI).sum()) == 3 and int((p < do.CLAMP_LO).sum()) == 3
    leaves = [W1, b1, w2, b2]
    for clamped in (True, False):
        an_grads = do.grads(X, hidden, W1, b1, w2, b2, gs, clamped, torch.float64)
        f = lambda lv: (do.scores(X, *lv, hidden=None, clamped=clamped) * gs).sum()
        g = torch.Generator().manual_seed(61)
        for n in range(4):
            dirs = [torch.empty(t.shape, dtype=torch.float64).normal_(0, 1, generator=g) * float(t.abs().mean() + 1e-3) for t in leaves]
            h = 1e-6
            with torch.no_grad():
                fd = float(f([t + h * d for t, d in zip(leaves, dirs)]) - f([t - h * d for t, d in zip(leaves, dirs)])) / (2 * h)
            an = float(sum((gr * d).sum() for gr, d in zip(an_grads, dirs)))
            rel = abs(fd - an) / abs(an)
            print(f"[clamped {clamped}] direction {n}: finite difference {fd:.9e}, autograd {an:.9e}, relative {rel:.2e}")
            assert rel < 1e-6, (clamped, n, rel)
    # the clamp is part of the derivative: the six rows beyond it carry gradient only in the unclamped form
    gc = do.grads(X, hidden, W1, b1, w2, b2, gs, True, torch.float64)
    gu = do.grads(X, hidden, W1, b1, w2, b2, gs, False, torch.float64)
    assert not torch.equal(gc[3], gu[3])
