"""-m "not gpu": the host side of the token-embedding backward -- the entries of csrc/vit_embed_bwd.hip are declared,
exported and bound, the descriptor matches the header, every validation rule answers before any launch (so these calls run without a
GPU), the oracle's restatement is the reference's prepare_tokens, packing.pos_embed_matrix is the resampling and its transpose the fp64
adjoint, and the Python surface names and switches the right parameters."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import embed_bwd_oracle as eo
from multi_hmr_amd import _lib, backbone_train as bt, packing
from oracle import dinov2_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"mhmr_vit_embed_backward_workspace_bytes", "mhmr_vit_embed_backward"}
PTR = 0x10000          # a non-NULL, 16-byte aligned address that is never dereferenced: validation comes before any launch
BAD_ARG, BAD_SHAPE = -1, -2
TABLES = [(37, 16), (37, 64), (37, 48), (5, 3), (4, 9)]          # (M, G)


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _struct_fields(header, name):
    end = header.index("} " + name + ";")
    body = header[header.rindex("typedef struct {", 0, end):end]
    return re.findall(r"[\*\s,]([A-Za-z_0-9]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_entries_are_declared_bound_and_additive(L):
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    assert ENTRIES <= declared and ENTRIES <= set(_lib._SIGS)
    assert declared == set(_lib.EXPORTS)
    assert "#define MHMR_VERSION 106" in header and _lib.VERSION == 106 and L.mhmr_version() == 106      # additive: the version stays
    assert "vit_embed_bwd.hip" in _lib.SOURCES
    assert all(hasattr(L, n) for n in ENTRIES)
    fields = [f[0] for f in _lib.VitEmbedBackwardDesc._fields_]
    assert _struct_fields(header, "mhmr_vit_embed_backward_desc") == fields
    assert fields == ["B", "S", "G", "M", "Tp", "C", "x", "g_stream", "interp", "g_patch_w", "g_patch_b", "g_cls", "g_pos", "workspace",
                      "workspace_bytes"]
    # the descriptors of the block and of the tail keep their fields: the embedding has an entry of its own
    assert not any(n in [f[0] for f in cls._fields_] for cls in (_lib.VitBlockBackwardDesc, _lib.VitTailBackwardDesc)
                   for n in ("x", "interp", "g_patch_w", "g_pos", "g_cls"))


def _desc(L, **over):
    d = _lib.VitEmbedBackwardDesc()
    d.B, d.S, d.G, d.M, d.Tp, d.C = 2, 42, 3, 5, 64, 128
    for n, t in d._fields_:
        if t is _lib._vp:
            setattr(d, n, PTR)
    for k, v in over.items():
        setattr(d, k, v)
    if "workspace_bytes" not in over:
        nb = int(L.mhmr_vit_embed_backward_workspace_bytes(d.B, d.G, d.M, d.C))
        d.workspace_bytes = nb if nb > 0 else 1 << 40
    return d


def test_embed_backward_validates_before_any_launch(L):
    call = lambda **over: L.mhmr_vit_embed_backward(C.byref(_desc(L, **over)), None)
    assert L.mhmr_vit_embed_backward(None, None) == BAD_ARG
    for n, t in _lib.VitEmbedBackwardDesc._fields_:
        if t is _lib._vp:
            assert call(**{n: None}) == BAD_ARG, n                       # every pointer is read or written
    assert call(workspace_bytes=int(L.mhmr_vit_embed_backward_workspace_bytes(2, 3, 5, 128)) - 1) == BAD_ARG
    assert call(workspace_bytes=0) == BAD_ARG and call(workspace=PTR + 8) == BAD_ARG and call(interp=PTR + 4) == BAD_ARG
    for over in (dict(B=-1), dict(S=-42, G=-3), dict(G=-3), dict(S=-42), dict(M=-5), dict(Tp=-64), dict(C=-128)):
        assert call(**over) == BAD_ARG, over
    for over in (dict(S=41), dict(S=56), dict(G=4), dict(Tp=96), dict(Tp=0), dict(S=112, G=8, Tp=64), dict(C=96), dict(C=0), dict(C=2112),
                 dict(B=0), dict(M=0), dict(S=0, G=0), dict(M=4097), dict(S=14 * 1025, G=1025, Tp=1025 * 1025 + 63), dict(B=16384, Tp=64)):
        assert call(**over) == BAD_SHAPE, over
    wb = L.mhmr_vit_embed_backward_workspace_bytes
    assert wb(-1, 3, 5, 128) == BAD_ARG and wb(1, -3, 5, 128) == BAD_ARG and wb(1, 3, -5, 128) == BAD_ARG and wb(1, 3, 5, -128) == BAD_ARG
    for bad in ((0, 3, 5, 128), (1, 0, 5, 128), (1, 3, 0, 128), (1, 3, 5, 100), (1, 3, 5, 0), (1, 3, 5, 2112), (1, 1025, 5, 128), (1, 3, 4097, 128)):
        assert wb(*bad) == BAD_SHAPE, bad
    assert 0 < wb(1, 3, 5, 128) < wb(64, 3, 5, 128) < wb(4096, 3, 5, 128)                  # grows with B: the slices of the bias sums
    assert wb(1, 16, 37, 128) >= (16 * 16 + 16 * 37) * 128 * 8                             # the image sums and the half-resampled table, fp64


# ------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("M,G", [(5, 3), (4, 4), (4, 9)])
def test_restatement_is_the_reference_prepare_tokens(M, G):
    """fp32 restatement == DinoVisionTransformer.prepare_tokens: the same operations in the same dtype, so within a few fp32 roundings of
    the tokens' size (both sides round the convolution, the resampling and one addition)."""
    enc = dinov2_ref.DinoVisionTransformer(embed_dim=128, depth=1, num_heads=2, img_size=14 * M)
    p = eo.make_params(128, M, seed=10 * M + G)
    with torch.no_grad():
        enc.patch_embed.proj.weight.copy_(p["patch_w"])
        enc.patch_embed.proj.bias.copy_(p["patch_b"])
        enc.cls_token.copy_(p["cls_token"])
        enc.pos_embed.copy_(p["pos_embed"])
        x = torch.randn(2, 3, 14 * G, 14 * G, generator=torch.Generator().manual_seed(3)) + 0.5
        ref, got = enc.prepare_tokens(x), eo.prepare_tokens(x, **p)
    assert got.shape == ref.shape == (2, 1 + G * G, 128) and got.dtype == torch.float32
    assert float((got - ref).abs().max()) <= 4 * 2.0 ** -24 * float(ref.abs().max())
    # in fp64 the restatement stays fp64 all the way (the reference's resampling would cast to fp32)
    assert eo.prepare_tokens(x.double(), **{k: v.double() for k, v in p.items()}).dtype == torch.float64
    assert eo.interpolate(p["pos_embed"], M) is p["pos_embed"]


@pytest.mark.parametrize("M,G", TABLES)
def test_pos_embed_matrix_reproduces_the_host_interpolation(M, G):
    R = packing.pos_embed_matrix(M, G)
    assert R.shape == (G, M) and R.dtype == np.float64
    assert float(np.abs(R.sum(1) - 1.0).max()) < 1e-14                   # cubic convolution weights sum to one, clipped taps included
    pe = np.random.default_rng(M * 100 + G).normal(0, 0.02, (1, 1 + M * M, 8)).astype(np.float32)
    want = packing.interpolate_pos_embed(pe, G)
    got = np.einsum("ya,xb,abc->yxc", R, R, pe[0, 1:].astype(np.float64).reshape(M, M, 8)).reshape(G * G, 8).astype(np.float32)
    assert want.shape == (1 + G * G, 8) and np.array_equal(want[0], pe[0, 0])
    assert bool((np.abs(got.astype(np.float64) - want[1:].astype(np.float64)) <= np.spacing(np.abs(want[1:])).astype(np.float64)).all())
    # the fp64 torch resampling of the oracle is the same map
    ref = eo.interpolate(torch.from_numpy(pe).double(), G)[0, 1:].numpy()
    exact = np.einsum("ya,xb,abc->yxc", R, R, pe[0, 1:].astype(np.float64).reshape(M, M, 8)).reshape(G * G, 8)
    assert float(np.abs(exact - ref).max()) < 1e-13 * float(np.abs(ref).max())


def test_pos_embed_matrix_is_the_identity_on_the_stored_grid():
    for M in (1, 4, 16, 37):
        assert np.array_equal(packing.pos_embed_matrix(M, M), np.eye(M))
    # ... which the formula with the 0.1 offset is not: a neighbouring grid has no row of the identity
    assert not np.array_equal(packing.pos_embed_matrix(4, 5)[:4], np.eye(4))


@pytest.mark.parametrize("M,G", [(37, 16), (5, 3)])
def test_pos_embed_matrix_transposed_is_the_fp64_adjoint(M, G):
    """interp^T g interp == fp64 autograd of F.interpolate(bicubic, scale_factor): sums of at most 16 products in fp64 on both sides, so a
    bound of 1e-13 of the largest entry leaves three decades over the 1.1e-16 of one rounding."""
    Cd = 8
    g = torch.Generator().manual_seed(M + G)
    pe = torch.empty(1, 1 + M * M, Cd, dtype=torch.float64).normal_(0, 1, generator=g).requires_grad_()
    go = torch.empty(1, 1 + G * G, Cd, dtype=torch.float64).normal_(0, 1, generator=g)
    (eo.interpolate(pe, G) * go).sum().backward()
    R = torch.from_numpy(packing.pos_embed_matrix(M, G))
    adj = torch.einsum("ya,xb,yxc->abc", R, R, go[0, 1:].reshape(G, G, Cd)).reshape(M * M, Cd)
    assert torch.equal(pe.grad[0, 0], go[0, 0])
    assert float((adj - pe.grad[0, 1:]).abs().max()) < 1e-13 * float(pe.grad.abs().max())


# ------------------------------------------------------------------------------------------------------ the Python surface
def _model(smplx_data, mean_params):
    from multi_hmr_amd import Model
    return Model(backbone="dinov2_vits14", img_size=224, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=3)


def test_embedding_parameter_names_resolve_and_the_switch_flips_exactly_those(smplx_data, mean_params):
    m = _model(smplx_data, mean_params)
    named = dict(m.named_parameters())
    names = bt.embedding_parameter_names()
    assert names == ["backbone.encoder.patch_embed.proj.weight", "backbone.encoder.patch_embed.proj.bias", "backbone.encoder.pos_embed",
                     "backbone.encoder.cls_token"]
    assert all(k in named for k in names) and [id(p) for p in m.embedding_parameters()] == [id(named[k]) for k in names]
    assert not set(names) & set(bt.backbone_parameter_names(3, 3))
    assert named[names[0]].shape == (384, 3, 14, 14) and named[names[2]].shape == (1, 1 + 37 * 37, 384)
    assert tuple(bt.EMBED_FIELDS.values()) == tuple(k[len(bt.ENCODER):] for k in names) and set(bt.EMBED_FIELDS) == set(eo.NAMES)
    assert not any(p.requires_grad for p in m.parameters())
    assert m.train_embeddings_() is m
    assert {k for k, p in named.items() if p.requires_grad} == set(names)
    m.train_backbone_(3)
    assert {k for k, p in named.items() if p.requires_grad} == set(names) | set(bt.backbone_parameter_names(3, 3))
    m.train_embeddings_(False)
    assert {k for k, p in named.items() if p.requires_grad} == set(bt.backbone_parameter_names(3, 3))
    # with the backbone, every encoder parameter the reference's optimiser sees has a gradient here (the mask token is never used)
    every = {k for k in named if k.startswith("backbone.encoder.") and not k.endswith("mask_token")}
    assert every == set(names) | set(bt.backbone_parameter_names(3, 3))


def test_embeddings_without_every_block_raise_before_anything_else(smplx_data, mean_params):
    m = _model(smplx_data, mean_params).train_backbone_(2).train_embeddings_()
    x, K = torch.zeros(1, 3, 224, 224), torch.eye(3)[None]              # CPU tensors: the check comes before the device is looked at
    idx = tuple(torch.zeros(1, dtype=torch.long) for _ in range(4))
    with pytest.raises(ValueError, match=r"train_backbone_\(3\)"):
        m(x, idx=idx, K=K, is_training=True, train_backbone=True)
    with pytest.raises(ValueError, match=r"train_backbone_\(3\)"):
        m.backbone_features(x, train_backbone=True)
    # with every block switched on the same call gets as far as the device check; without train_backbone the switch is not looked at
    m.train_backbone_(3)
    with pytest.raises(_lib.MhmrError, match="MI355X"):
        m(x, idx=idx, K=K, is_training=True, train_backbone=True)
    m.train_backbone_(2)
    with pytest.raises(_lib.MhmrError, match="MI355X"):
        m(x, idx=idx, K=K, is_training=True)
