"""-m "not gpu": the host side of the heads-from-stored-features path (csrc/feature_grad.hip, the g_feat fields of the two backward
descriptors, mhmr_detect_feature_grad) -- header / binding agree, every new entry returns its documented code before
any launch (so every case runs without a GPU), an empty problem returns 0, and the feature oracle's detector term is the product it
claims to be."""
import ctypes as C
import os
import re

import pytest
import torch

import feature_grad_oracle as fo
from multi_hmr_amd import Model, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE = -1, -2
ENTRIES = {"mhmr_rows_times_weight", "mhmr_detect_feature_grad_workspace_bytes", "mhmr_detect_feature_grad", "mhmr_features_to_context"}
PTR = 64          # non-null, never dereferenced: validation comes before any launch


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _call(fn, names, defaults):
    return lambda **o: fn(*[{**defaults, **o}[k] for k in names])


def test_entries_are_declared_bound_and_additive(L):
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    assert ENTRIES <= declared and ENTRIES <= set(_lib._SIGS) and declared == set(_lib.EXPORTS)
    assert "#define MHMR_VERSION 106" in header and L.mhmr_version() == 106      # additive entries and appended fields: the version stays
    assert "feature_grad.hip" in _lib.SOURCES
    assert all(hasattr(L, n) for n in ENTRIES)
    # the appended descriptor fields come last, and a fresh descriptor has them NULL / 0
    assert [f[0] for f in _lib.XattnBackwardDesc._fields_][-3:] == ["g_feat", "ld_feat", "feat_cols"]
    assert [f[0] for f in _lib.HphBackwardDesc._fields_][-2:] == ["g_feat", "ld_feat"]
    assert not _lib.XattnBackwardDesc().g_feat and not _lib.HphBackwardDesc().g_feat
    assert not _lib.f32p(None)


def test_rows_times_weight_validation(L):
    names = ("left", "ldl", "w16", "ldw", "out", "ldo", "rows", "n", "C", "accumulate", "dtype", "stream")
    call = _call(L.mhmr_rows_times_weight, names, dict(left=PTR, ldl=512, w16=PTR, ldw=1024, out=PTR, ldo=1024, rows=203, n=512, C=1024,
                                                       accumulate=0, dtype=_lib.DT_F16, stream=None))
    assert call(rows=-1) == BAD_ARG
    assert call(rows=0) == 0 and call(rows=0, left=None, w16=None, out=None) == 0          # an empty problem
    for bad in (dict(n=0), dict(n=-16), dict(n=520), dict(C=0), dict(C=1000), dict(C=64), dict(ldl=511), dict(ldw=1023), dict(ldo=1023),
                dict(dtype=2), dict(dtype=-1),
                dict(rows=64 * 0xFFFFFF // 8 + 1),                       # 8 column tiles: one row tile more than 2^24 - 1 workgroups
                dict(rows=2 ** 31 - 1)):
        assert call(**bad) == BAD_SHAPE, bad
    for bad in (dict(left=None), dict(w16=None), dict(out=None)):
        assert call(**bad) == BAD_ARG, bad


def test_detect_feature_grad_validation(L):
    names = ("hid16", "ldh", "w16", "ldw", "w2", "b2", "gs", "rows", "C", "clamped", "dtype", "g_feat", "ldg", "ws", "nbytes", "stream")
    call = _call(L.mhmr_detect_feature_grad, names, dict(hid16=PTR, ldh=384, w16=PTR, ldw=384, w2=PTR, b2=PTR, gs=PTR, rows=515, C=384, clamped=1,
                                                         dtype=_lib.DT_BF16, g_feat=PTR, ldg=384, ws=PTR, nbytes=1 << 30, stream=None))
    need = L.mhmr_detect_feature_grad_workspace_bytes(515)
    assert need >= 4 * 515 and L.mhmr_detect_feature_grad_workspace_bytes(0) == 0 and L.mhmr_detect_feature_grad_workspace_bytes(-1) == BAD_ARG
    sizes = [L.mhmr_detect_feature_grad_workspace_bytes(r) for r in (0, 1, 5, 203, 515, 131072)]
    assert sizes == sorted(sizes)
    assert call(rows=-1) == BAD_ARG
    assert call(rows=0) == 0 and call(rows=0, hid16=None, g_feat=None, ws=None, nbytes=0) == 0
    for bad in (dict(C=0), dict(C=-128), dict(C=100), dict(C=16384 + 128), dict(ldh=383), dict(ldh=385), dict(ldw=383), dict(ldg=383), dict(dtype=2),
                dict(rows=512 * 65535 + 1, nbytes=1 << 40),                              # the launch limit of the row pass' sibling
                dict(rows=64 * (0xFFFFFF // 64) + 64, C=8192, ldh=8192, ldw=8192, ldg=8192, nbytes=1 << 40)):      # 64 column tiles
        assert call(**bad) == BAD_SHAPE, bad
    for bad in (dict(hid16=None), dict(w16=None), dict(w2=None), dict(b2=None), dict(gs=None), dict(g_feat=None), dict(ws=None),
                dict(nbytes=need - 1)):
        assert call(**bad) == BAD_ARG, bad


def test_features_to_context_validation(L):
    names = ("features", "feat32", "ctx16", "ldctx", "rows", "C", "dtype", "stream")
    call = _call(L.mhmr_features_to_context, names, dict(features=1 << 20, feat32=1 << 30, ctx16=PTR, ldctx=512, rows=512, C=384,
                                                         dtype=_lib.DT_F16, stream=None))
    assert call(rows=-1) == BAD_ARG
    assert call(rows=0) == 0 and call(rows=0, features=None, feat32=None, ctx16=None) == 0
    for bad in (dict(C=0), dict(C=-4), dict(ldctx=383), dict(dtype=7), dict(rows=2 ** 22, C=1024, ldctx=1024), dict(rows=2 ** 31 - 1)):
        assert call(**bad) == BAD_SHAPE, bad
    for bad in (dict(features=None), dict(feat32=None), dict(ctx16=None),
                dict(feat32=(1 << 20) + 4), dict(feat32=(1 << 20) - 4), dict(feat32=(1 << 20) + 512 * 384 * 4 - 4)):      # a partial overlap
        assert call(**bad) == BAD_ARG, bad


def _stack_desc(**over):
    d = _lib.XattnBackwardDesc()
    d.depth, d.dim, d.heads, d.mlp, d.Kc, d.N, d.B, d.dtype = 2, 1024, 8, 1024, 512, 256, 2, _lib.DT_F16
    d.P, d.ngroups, d.nmax, d.nchunks, d.ctx_valid = 5, 2, 5, 3, 483
    keep = [(_lib.HphLayer * 2)(), (_lib.HphLayerGrads * 2)()]
    for arr in keep:
        for e in arr:
            for n, _ in e._fields_:
                setattr(e, n, PTR)
    d.layers, d.grads = C.cast(keep[0], C.POINTER(_lib.HphLayer)), C.cast(keep[1], C.POINTER(_lib.HphLayerGrads))
    for n in ("x0", "ctx16", "gstart", "chunks", "g_x_out", "g_x0"):
        setattr(d, n, PTR)
    d.workspace, d.workspace_bytes = PTR, 1024                    # too short: a call that passes every shape rule ends in BAD_ARG, unlaunched
    d.g_feat, d.ld_feat, d.feat_cols = C.cast(C.c_void_p(PTR), _lib._f32p), 384, 384
    for k, v in over.items():
        setattr(d, k, v)
    d._keep = keep
    return d


def test_the_descriptors_check_g_feat_before_any_launch(L):
    call = lambda **o: L.mhmr_xattn_layers_backward(C.byref(_stack_desc(**o)), None)
    assert call() == BAD_ARG                                       # (the short workspace: the feature fields themselves are fine)
    for bad in (dict(feat_cols=0), dict(feat_cols=100), dict(feat_cols=640), dict(ld_feat=383), dict(feat_cols=-128)):
        assert call(**bad) == BAD_SHAPE, bad
    assert call(g_feat=_lib.f32p(None), feat_cols=0, ld_feat=0) == BAD_ARG      # NULL: the fields beside it are not read
    # the whole head: C of the forward descriptor is the width
    f = _lib.HphDesc()
    f.dtype, f.C, f.G, f.N, f.Kc, f.dim, f.heads, f.mlp, f.depth, f.nb, f.Ktok, f.Ndec, f.patch, f.nearness = (
        _lib.DT_F16, 384, 16, 256, 512, 1024, 8, 1024, 2, 10, 816, 341, 14, 1)
    f.cam_dim = 99
    d = _lib.HphBackwardDesc()
    d.fwd = C.pointer(f)
    d.ngroups, d.nmax, d.nchunks, d.P, d.B, d.ldg, d.workspace_bytes = 2, 5, 3, 5, 2, 341, 0
    d.g_feat = C.cast(C.c_void_p(PTR), _lib._f32p)
    d.ld_feat = 383
    assert L.mhmr_hph_backward(C.byref(d), None) == BAD_SHAPE
    d.ld_feat = 384
    assert L.mhmr_hph_backward(C.byref(d), None) == BAD_ARG        # past the shape rules: the NULL pointers of this descriptor


def test_forward_features_rejects_its_arguments_without_a_device():
    """What needs no GPU: the keyword rules of ``forward`` and a CPU tensor."""
    import synthetic
    m = Model(backbone="dinov2_vits14", img_size=224, smplx_data=synthetic.make_smplx_data(seed=0), mean_params=synthetic.make_mean_params(seed=0),
              backbone_depth=1)
    f = torch.zeros(1, 256, 384)
    with pytest.raises(ValueError):
        m.forward_features(f, train_heads=True)
    with pytest.raises(ValueError):
        m.forward_features(f, is_training=True, train_heads=True)
    with pytest.raises(ValueError):
        m.forward_features(f, train_detection=True)
    with pytest.raises(_lib.MhmrError, match="no CPU fallback"):
        m.forward_features(f, K=torch.eye(3)[None])


def test_oracle_detector_term_is_the_product_of_the_hidden_cotangent():
    """fp64, by hand: dl = gs p (1 - p) inside the clamp, the hidden cotangent dl w2 under the mask, times the weight."""
    g = torch.Generator().manual_seed(2)
    rows, C_ = 9, 128
    hid = torch.relu(torch.empty(rows, C_).normal_(0, 1, generator=g)).half()
    w16 = (torch.empty(C_, C_).normal_(0, 1, generator=g) * C_ ** -0.5).half()
    w2, b2, gs = torch.empty(C_).normal_(0, 1, generator=g) * C_ ** -0.5, torch.tensor([0.1]), torch.empty(rows).normal_(0, 1, generator=g)
    hid[4] = (w2 > 0).half() * 8                                    # one row beyond the clamp
    p = torch.sigmoid(hid.double() @ w2.double() + b2.double())
    inside = (p >= 1e-4) & (p <= 1 - 1e-4)
    assert not bool(inside[4]) and int(inside.sum()) == rows - 1
    dl = torch.where(inside, gs.double() * p * (1 - p), torch.zeros((), dtype=torch.float64))
    want = fo.product(torch.where(hid > 0, dl[:, None] * w2.double()[None, :], torch.zeros((), dtype=torch.float64)), w16, torch.float64)
    got = fo.detector_term(hid, w16, w2, b2, gs, True, torch.float64)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
