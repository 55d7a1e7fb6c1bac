"""-m "not gpu": the host side of the backbone backward -- the entries of csrc/vit_bwd.hip and the attention pair
of csrc/attention_f32.hip are declared, exported and bound, their descriptors match the header, every entry validates its arguments
before any launch (so these calls run without a GPU),
the closed-form attention oracle equals fp64 autograd, and the Python surface names the right parameters."""
import ctypes as C
import os
import re

import pytest
import torch

import backbone_bwd_oracle as bo
from multi_hmr_amd import _lib, backbone_train as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"mhmr_attention_f32_tape", "mhmr_attention_f32_backward_workspace_bytes", "mhmr_attention_f32_backward",
           "mhmr_vit_block_backward_workspace_bytes", "mhmr_vit_block_backward", "mhmr_vit_tail_backward_workspace_bytes",
           "mhmr_vit_tail_backward"}
STRUCTS = {"mhmr_vit_block_backward_desc": _lib.VitBlockBackwardDesc, "mhmr_vit_tail_backward_desc": _lib.VitTailBackwardDesc,
           "mhmr_vit_desc": _lib.VitDesc}
PTR = 0x10000          # a non-NULL, 16-byte aligned address that is never dereferenced: validation comes before any launch
BAD_ARG, BAD_SHAPE = -1, -2


def _struct_fields(header, name):
    end = header.index("} " + name + ";")
    body = header[header.rindex("typedef struct {", 0, end):end]
    return re.findall(r"[\*\s,]([A-Za-z_0-9]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_entries_are_declared_bound_and_additive(L):
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    assert ENTRIES <= declared and ENTRIES <= set(_lib._SIGS)
    assert declared == set(_lib.EXPORTS)
    assert "#define MHMR_VERSION 106" in header and _lib.VERSION == 106 and L.mhmr_version() == 106      # additive: the version stays
    assert "vit_bwd.hip" in _lib.SOURCES
    for name, cls in STRUCTS.items():
        assert _struct_fields(header, name) == [f[0] for f in cls._fields_], name
    assert all(hasattr(L, n) for n in ENTRIES)
    # the tap is appended: zero (the default of a fresh descriptor) means off, and every older field keeps its offset
    assert [f[0] for f in _lib.VitDesc._fields_][-2:] == ["tap", "tap_first"]
    d = _lib.VitDesc()
    assert not d.tap and d.tap_first == 0
    assert tuple(_lib.VitBlockBackwardDesc.PARAMS) == bo.PARAMS == tuple(bt.BLOCK_FIELDS)


# ------------------------------------------------------------------------------------------------------ validation
def _tape(L, qkv=PTR, out=PTR, lse=PTR, B=2, T=17, Tp=64, Cd=128, H=2):
    return L.mhmr_attention_f32_tape(qkv, out, lse, B, T, Tp, Cd, H, None)


def _abwd(L, qkv=PTR, out=PTR, lse=PTR, dO=PTR, ldd=128, dqkv=PTR, B=2, T=17, Tp=64, Cd=128, H=2, ws=PTR, nbytes=None):
    nbytes = int(L.mhmr_attention_f32_backward_workspace_bytes(B, Tp, H)) if nbytes is None else nbytes
    return L.mhmr_attention_f32_backward(qkv, out, lse, dO, ldd, dqkv, B, T, Tp, Cd, H, ws, nbytes, None)


def test_attention_entries_validate_before_any_launch(L):
    for call in (_tape, _abwd):
        for kw in (dict(qkv=None), dict(out=None), dict(lse=None), dict(B=-1), dict(T=-1), dict(Tp=-64), dict(H=-2, Cd=-128)):
            assert call(L, **kw) == BAD_ARG, (call.__name__, kw)
        for kw in (dict(Cd=192), dict(H=3), dict(Tp=96), dict(Tp=80, T=70), dict(T=65), dict(B=0), dict(T=0), dict(B=65536), dict(qkv=PTR + 4)):
            assert call(L, **kw) == (BAD_ARG if "qkv" in kw else BAD_SHAPE), (call.__name__, kw)
    for kw in (dict(dO=None), dict(dqkv=None), dict(ws=None), dict(nbytes=0), dict(dO=PTR + 8),
               dict(nbytes=int(L.mhmr_attention_f32_backward_workspace_bytes(2, 64, 2)) - 1)):
        assert _abwd(L, **kw) == BAD_ARG, kw
    for kw in (dict(ldd=127), dict(ldd=130), dict(ldd=64)):
        assert _abwd(L, **kw) == BAD_SHAPE, kw
    wb = L.mhmr_attention_f32_backward_workspace_bytes
    assert wb(-1, 64, 2) == BAD_ARG and wb(1, -64, 2) == BAD_ARG and wb(1, 64, -1) == BAD_ARG
    assert wb(1, 65, 2) == BAD_SHAPE and wb(0, 64, 2) == BAD_SHAPE
    assert 0 < wb(1, 64, 2) < wb(2, 64, 2) < wb(4, 64, 2) and wb(2, 64, 2) >= 2 * 2 * 64 * 4      # grows with B; holds D [B, H, Tp]


def _block_desc(L, **over):
    d = _lib.VitBlockBackwardDesc()
    d.B, d.T, d.Tp, d.C, d.H = 2, 17, 64, 128, 2
    for n, t in d._fields_:
        if t is _lib._vp:
            setattr(d, n, PTR)
    d.g_in = PTR + 64
    for k, v in over.items():
        setattr(d, k, v)
    if "workspace_bytes" not in over:
        nb = int(L.mhmr_vit_block_backward_workspace_bytes(d.B, d.Tp, d.C))
        d.workspace_bytes = nb if nb > 0 else 1 << 40
    return d


def test_block_backward_validates_before_any_launch(L):
    call = lambda **over: L.mhmr_vit_block_backward(C.byref(_block_desc(L, **over)), None)
    assert L.mhmr_vit_block_backward(None, None) == BAD_ARG
    for n, t in _lib.VitBlockBackwardDesc._fields_:
        if t is _lib._vp:
            assert call(**{n: None}) == BAD_ARG, n                      # every pointer is read or written
    assert call(workspace_bytes=int(L.mhmr_vit_block_backward_workspace_bytes(2, 64, 128)) - 1) == BAD_ARG
    assert call(g_in=PTR) == BAD_ARG                                     # g_in may not alias g_out
    for over in (dict(B=-1), dict(T=-1), dict(Tp=-64), dict(C=-128, H=-2)):
        assert call(**over) == BAD_ARG, over
    for over in (dict(C=192), dict(H=3), dict(Tp=96), dict(T=65), dict(B=0), dict(T=0), dict(C=4096, H=64), dict(B=65535, Tp=64)):
        assert call(**over) == BAD_SHAPE, over
    wb = L.mhmr_vit_block_backward_workspace_bytes
    assert wb(-1, 64, 128) == BAD_ARG and wb(1, 65, 128) == BAD_SHAPE and wb(1, 64, 100) == BAD_SHAPE and wb(1, 64, 4096) == BAD_SHAPE
    assert 0 < wb(1, 64, 128) < wb(2, 64, 128) < wb(4, 64, 128)
    assert wb(2, 64, 128) >= 26 * 2 * 64 * 128 * 4                       # the tape and the cotangents: 26 C floats per row


def test_tail_backward_validates_before_any_launch(L):
    blocks = (_lib.VitBlockBackwardDesc * 2)()
    for b in blocks:
        for n, t in b._fields_:
            if t is _lib._vp:
                setattr(b, n, PTR)

    def call(null_block_field=None, **over):
        d = _lib.VitTailBackwardDesc()
        d.B, d.N, d.T, d.Tp, d.C, d.H, d.n = 2, 16, 17, 64, 128, 2, 2
        for n, t in d._fields_:
            if t is _lib._vp:
                setattr(d, n, PTR)
        d.blocks = C.cast(blocks, C.POINTER(_lib.VitBlockBackwardDesc))
        for k, v in over.items():
            setattr(d, k, v)
        if "workspace_bytes" not in over:
            nb = int(L.mhmr_vit_tail_backward_workspace_bytes(d.B, d.Tp, d.C))
            d.workspace_bytes = nb if nb > 0 else 1 << 40
        if null_block_field:
            setattr(blocks[1], null_block_field, None)
        rc = L.mhmr_vit_tail_backward(C.byref(d), None)
        if null_block_field:
            setattr(blocks[1], null_block_field, PTR)
        return rc
    assert L.mhmr_vit_tail_backward(None, None) == BAD_ARG
    for n, t in _lib.VitTailBackwardDesc._fields_:
        if t is _lib._vp:
            assert call(**{n: None}) == BAD_ARG, n
    assert call(blocks=None) == BAD_ARG
    for f in _lib.VitBlockBackwardDesc.PARAMS:
        assert call(null_block_field=f) == BAD_ARG and call(null_block_field="g_" + f) == BAD_ARG, f
    assert call(workspace_bytes=int(L.mhmr_vit_tail_backward_workspace_bytes(2, 64, 128)) - 1) == BAD_ARG
    for over in (dict(B=-1), dict(n=-1), dict(N=-1), dict(T=-1), dict(Tp=-64)):
        assert call(**over) == BAD_ARG, over
    for over in (dict(n=0), dict(N=15), dict(C=192), dict(H=3), dict(Tp=96), dict(T=65, N=64), dict(B=0)):
        assert call(**over) == BAD_SHAPE, over
    wb, bb = L.mhmr_vit_tail_backward_workspace_bytes, L.mhmr_vit_block_backward_workspace_bytes
    assert wb(-1, 64, 128) == BAD_ARG and wb(1, 65, 128) == BAD_SHAPE and wb(1, 64, 100) == BAD_SHAPE
    assert 0 < wb(1, 64, 128) < wb(2, 64, 128) < wb(4, 64, 128) and wb(2, 64, 128) > bb(2, 64, 128)


# ------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("T,Tp", [(2, 64), (17, 64), (65, 192)])
def test_closed_form_attention_backward_equals_fp64_autograd(T, Tp):
    B, H = 2, 2
    g = torch.Generator().manual_seed(T)
    qkv = torch.empty(B * Tp, 3 * 64 * H).normal_(0, 1, generator=g)
    dO = torch.empty(B * Tp, 64 * H).normal_(0, 1, generator=g)
    closed = bo.attention_backward_closed_form(qkv, dO, B, T, Tp, H)
    auto = bo.attention_backward_autograd(qkv, dO, B, T, Tp, H)
    assert closed.dtype == auto.dtype == torch.float64 and closed.shape == auto.shape == (B * Tp, 3 * 64 * H)
    assert float((closed - auto).abs().max()) < 1e-13 * float(auto.abs().max()) + 1e-15
    real = torch.arange(B * Tp) % Tp < T
    assert bool((closed[~real] == 0).all()) and bool((auto[~real] == 0).all()) and bool((closed[real] != 0).any())
    # the key-bias direction: a common shift of the keys changes nothing, so dK sums to zero over the keys of an image and head
    dk = closed[:, 64 * H:2 * 64 * H].reshape(B, Tp, H, 64).sum(1)
    assert float(dk.abs().max()) < 1e-12 * float(closed.abs().max())
    out, lse = bo.attention_forward(qkv, B, T, Tp, H)
    assert out.shape == (B * Tp, 64 * H) and lse.shape == (B, H, Tp) and bool((out[~real] == 0).all())


def test_block_oracle_is_the_reference_block():
    from oracle import dinov2_ref
    blk = bo.make_block(128, 2, seed=1)
    assert isinstance(blk, dinov2_ref.Block) and set(bo.block_params(blk)) == set(bo.PARAMS)
    assert len(list(blk.parameters())) == 14
    g = torch.Generator().manual_seed(0)
    x, go = torch.empty(2 * 64, 128).normal_(0, 1, generator=g), torch.empty(2 * 64, 128).normal_(0, 1, generator=g)
    r = bo.block_backward(blk, x, go, 2, 17, 64)
    assert all(r[k].shape == p.shape for k, p in bo.block_params(blk).items()) and r["g_in"].shape == (128, 128)
    assert bool((r["g_in"].reshape(2, 64, 128)[:, 17:] == 0).all()) and all(p.grad is None for p in blk.parameters())


# ------------------------------------------------------------------------------------------------------ the Python surface
def test_backbone_parameter_names_match_the_module(smplx_data, mean_params):
    from multi_hmr_amd import Model
    m = Model(backbone="dinov2_vits14", img_size=224, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=3)
    named = dict(m.named_parameters())
    for n in (1, 2, 3):
        names = bt.backbone_parameter_names(3, n)
        assert len(names) == len(set(names)) == 2 + 14 * n and all(k in named for k in names)
        assert names[:2] == ["backbone.encoder.norm.weight", "backbone.encoder.norm.bias"]
        blocks = {int(k.split(".")[3]) for k in names[2:]}
        assert blocks == set(range(3 - n, 3))
        assert [id(p) for p in m.backbone_parameters(n)] == [id(named[k]) for k in names]
    every = {k for k in named if k.startswith("backbone.encoder.blocks.") or k.startswith("backbone.encoder.norm.")}
    assert set(bt.backbone_parameter_names(3, 3)) == every
    for bad in (0, 4, -1):
        with pytest.raises(ValueError):
            bt.backbone_parameter_names(3, bad)
        with pytest.raises(ValueError):
            m.train_backbone_(bad)


def test_train_backbone_leaves_every_other_parameter_frozen(smplx_data, mean_params):
    from multi_hmr_amd import Model
    m = Model(backbone="dinov2_vits14", img_size=224, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=3)
    assert not any(p.requires_grad for p in m.parameters())
    assert m.train_backbone_(2) is m
    on = {k for k, p in m.named_parameters() if p.requires_grad}
    assert on == set(bt.backbone_parameter_names(3, 2))
    m.train_backbone_(2, False)
    assert not any(p.requires_grad for p in m.parameters())
    m.train_backbone_(1)
    assert {k for k, p in m.named_parameters() if p.requires_grad} == set(bt.backbone_parameter_names(3, 1))
    # the switches of forward: train_backbone needs training mode, as the other two do (checked before any GPU work)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 224, 224), K=torch.eye(3)[None], train_backbone=True)
