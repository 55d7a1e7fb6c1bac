"""-m "not gpu": the host side of the decoder backward (csrc/hph_bwd.hip, multi_hmr_amd/heads_train.py) -- header /
binding / version agree, every new entry validates before any launch (so every case runs without a GPU), the workspace sizes are
monotone, the packed-gradient -> parameter mapping on CPU tensors, and the oracle of tests/hph_bwd_oracle.py pinned in fp64 against
central finite differences."""
import ctypes as C
import os
import re

import pytest
import torch

import hph_bwd_oracle as ho
from multi_hmr_amd import _lib, heads_train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE = -1, -2
ENTRIES = {"mhmr_linear_f32_backward_input", "mhmr_linear_f32_backward_weight", "mhmr_layernorm_f32_backward_workspace_bytes",
           "mhmr_layernorm_f32_backward", "mhmr_hph_self_attn_backward", "mhmr_hph_cross_attn_backward", "mhmr_grad_ctx_gemm_workspace_bytes",
           "mhmr_grad_ctx_gemm", "mhmr_xattn_layers_backward_workspace_bytes", "mhmr_xattn_layers_backward", "mhmr_hph_backward_workspace_bytes",
           "mhmr_hph_backward"}
STRUCTS = {"mhmr_hph_layer_grads": _lib.HphLayerGrads, "mhmr_xattn_backward_desc": _lib.XattnBackwardDesc,
           "mhmr_hph_backward_desc": _lib.HphBackwardDesc}
PTR = 64          # non-null, never dereferenced: validation comes before any launch


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
    assert "#define MHMR_VERSION 106" in header and _lib.VERSION == 106 and L.mhmr_version() == 106      # additive entries: the version stays
    assert "hph_bwd.hip" in _lib.SOURCES
    for name, cls in STRUCTS.items():
        assert _struct_fields(header, name) == [f[0] for f in cls._fields_], name
    assert all(hasattr(L, n) for n in ENTRIES)
    assert _lib.HphLayerGrads.FIELDS == tuple(n.replace("to_kv16", "to_kv") for n, _ in _lib.HphLayer._fields_)


# ------------------------------------------------------------------------------------------------------ validation
def test_linear_backward_validation(L):
    inp = lambda **o: L.mhmr_linear_f32_backward_input(*[{**dict(dY=PTR, lddy=32, row_idx=None, Z=PTR, ldz=32, W=PTR, ldw=64, dR=None, lddr=0,
                                                                 dX=PTR, lddx=64, M=5, N=32, K=64, act=_lib.ACT_GELU, stream=None), **o}[k]
                                                         for k in ("dY", "lddy", "row_idx", "Z", "ldz", "W", "ldw", "dR", "lddr", "dX", "lddx", "M", "N", "K",
                                                                   "act", "stream")])
    assert inp(M=-1) == BAD_ARG
    assert inp(M=0) == 0
    for bad in (dict(N=0), dict(K=0), dict(act=3), dict(act=-1), dict(lddy=31), dict(ldw=63), dict(lddx=63), dict(dR=PTR, lddr=63), dict(ldz=31),
                dict(M=16 * 65535 + 1)):
        assert inp(**bad) == BAD_SHAPE, bad
    for bad in (dict(dY=None), dict(W=None), dict(dX=None), dict(Z=None)):
        assert inp(**bad) == BAD_ARG, bad
    wgt = lambda **o: L.mhmr_linear_f32_backward_weight(*[{**dict(dY=PTR, lddy=32, Z=PTR, ldz=32, X=PTR, ldx=64, dW=PTR, lddw=64, db=PTR, M=5, N=32,
                                                                  K=64, act=_lib.ACT_RELU, stream=None), **o}[k]
                                                          for k in ("dY", "lddy", "Z", "ldz", "X", "ldx", "dW", "lddw", "db", "M", "N", "K", "act", "stream")])
    assert wgt(M=-1) == BAD_ARG
    for bad in (dict(N=0), dict(K=0), dict(act=7), dict(lddy=31), dict(ldx=63), dict(lddw=63), dict(ldz=31),
                dict(N=16 * 65535 + 1, lddy=16 * 65535 + 1, ldz=16 * 65535 + 1)):
        assert wgt(**bad) == BAD_SHAPE, bad
    for bad in (dict(dW=None, db=None), dict(dY=None), dict(X=None), dict(Z=None)):
        assert wgt(**bad) == BAD_ARG, bad


def test_linear_forward_refuses_more_row_tiles_than_a_grid_holds(L):
    """mhmr_linear_f32's row tiles of 16 are gridDim.y of both of its forms: a launch limit, refused before the launch like its backward
    siblings' (every case here returns before any launch, so the pointers are never read)."""
    call = lambda **o: L.mhmr_linear_f32(*[{**dict(X=PTR, ldx=64, row_idx=None, W=PTR, ldw=64, bias=None, R=None, ldr=0, Y=PTR, ldy=32, M=5, N=32,
                                                   K=64, act=_lib.ACT_NONE, stream=None), **o}[k]
                                           for k in ("X", "ldx", "row_idx", "W", "ldw", "bias", "R", "ldr", "Y", "ldy", "M", "N", "K", "act", "stream")])
    for K in (64, 256, 4096):                          # the plain form and the split-k form
        assert call(M=16 * 65535 + 1, K=K, ldx=K, ldw=K) == BAD_SHAPE, K
        assert call(M=0x7fffffff, K=K, ldx=K, ldw=K) == BAD_SHAPE, K
    for bad in (dict(M=0), dict(N=0), dict(K=0), dict(K=40), dict(ldx=66), dict(ldw=66)):
        assert call(**bad) == BAD_SHAPE, bad


def test_layernorm_backward_validation(L):
    call = lambda **o: L.mhmr_layernorm_f32_backward(*[{**dict(x=PTR, w=PTR, dy=PTR, dR=None, dx=PTR, dw=PTR, db=PTR, rows=5, C=128, eps=1e-5,
                                                               ws=PTR, nbytes=1 << 20, stream=None), **o}[k]
                                                       for k in ("x", "w", "dy", "dR", "dx", "dw", "db", "rows", "C", "eps", "ws", "nbytes", "stream")])
    assert call(rows=-1) == BAD_ARG and call(rows=0) == 0
    for c in (0, 96, 2112):
        assert call(C=c) == BAD_SHAPE and L.mhmr_layernorm_f32_backward_workspace_bytes(5, c) == BAD_SHAPE
    need = L.mhmr_layernorm_f32_backward_workspace_bytes(5, 128)
    for bad in (dict(x=None), dict(w=None), dict(dy=None), dict(dx=None), dict(dw=None), dict(db=None), dict(ws=None), dict(nbytes=need - 1)):
        assert call(**bad) == BAD_ARG, bad
    assert L.mhmr_layernorm_f32_backward_workspace_bytes(-1, 128) == BAD_ARG
    # the first-stage slices of 32 rows are gridDim.y: a launch limit, refused before the dx kernel is enqueued
    assert call(rows=32 * 65535 + 1, nbytes=1 << 40) == BAD_SHAPE and L.mhmr_layernorm_f32_backward_workspace_bytes(32 * 65535 + 1, 128) == BAD_SHAPE
    assert L.mhmr_layernorm_f32_backward_workspace_bytes(32 * 65535, 128) > 0


def test_attention_backward_validation(L):
    sa = lambda **o: L.mhmr_hph_self_attn_backward(*[{**dict(qkv=PTR, dO=PTR, gstart=PTR, dqkv=PTR, lse=PTR, ngroups=2, nmax=9, heads=8, stream=None),
                                                      **o}[k] for k in ("qkv", "dO", "gstart", "dqkv", "lse", "ngroups", "nmax", "heads", "stream")])
    assert sa(ngroups=-1) == BAD_ARG and sa(nmax=-1) == BAD_ARG
    assert sa(ngroups=0) == 0 and sa(nmax=0) == 0
    for bad in (dict(heads=0), dict(heads=65536), dict(nmax=64 * 65535 + 1)):
        assert sa(**bad) == BAD_SHAPE, bad
    for bad in ("qkv", "dO", "gstart", "dqkv", "lse"):
        assert sa(**{bad: None}) == BAD_ARG, bad
    ca = lambda **o: L.mhmr_hph_cross_attn_backward(*[{**dict(q=PTR, kv=PTR, dO=PTR, chunks=PTR, nchunks=3, dq=PTR, dkv=PTR, lse=PTR, heads=8, N=256,
                                                              B=2, stream=None), **o}[k]
                                                      for k in ("q", "kv", "dO", "chunks", "nchunks", "dq", "dkv", "lse", "heads", "N", "B", "stream")])
    assert ca(nchunks=-1) == BAD_ARG
    for bad in (dict(heads=0), dict(heads=65536), dict(N=0), dict(B=0), dict(B=65536), dict(B=65535, N=1 << 16)):
        assert ca(**bad) == BAD_SHAPE, bad
    for bad in (dict(kv=None), dict(dq=None, dkv=None), dict(q=None), dict(dO=None), dict(chunks=None), dict(lse=None)):
        assert ca(**bad) == BAD_ARG, bad


def test_context_gemm_validation(L):
    call = lambda **o: L.mhmr_grad_ctx_gemm(*[{**dict(G=PTR, ldg=128, op16=PTR, ld16=512, dW=PTR, rows=1000, Nn=128, Kc=512, cvalid=483,
                                                      dtype=_lib.DT_F16, ws=PTR, nbytes=1 << 30, stream=None), **o}[k]
                                              for k in ("G", "ldg", "op16", "ld16", "dW", "rows", "Nn", "Kc", "cvalid", "dtype", "ws", "nbytes", "stream")])
    assert call(rows=-1) == BAD_ARG and L.mhmr_grad_ctx_gemm_workspace_bytes(-1, 128, 512) == BAD_ARG
    for bad in (dict(Nn=0), dict(Kc=0), dict(ldg=127), dict(ld16=511), dict(cvalid=-1), dict(cvalid=513), dict(dtype=2)):
        assert call(**bad) == BAD_SHAPE, bad
    need = L.mhmr_grad_ctx_gemm_workspace_bytes(1000, 128, 512)
    for bad in (dict(dW=None), dict(ws=None), dict(nbytes=need - 1), dict(G=None), dict(op16=None)):
        assert call(**bad) == BAD_ARG, bad
    assert L.mhmr_grad_ctx_gemm_workspace_bytes(1000, 0, 512) == BAD_SHAPE


def _stack_desc(**over):
    d = _lib.XattnBackwardDesc()
    d.depth, d.dim, d.heads, d.mlp, d.Kc, d.N, d.B, d.dtype = 2, 1024, 8, 1024, 1152, 256, 2, _lib.DT_F16
    d.P, d.ngroups, d.nmax, d.nchunks, d.ctx_valid = 5, 2, 5, 3, 1123
    keep = [(_lib.HphLayer * 2)(), (_lib.HphLayerGrads * 2)()]
    for arr in keep:
        for e in arr:
            for n, _ in e._fields_:
                setattr(e, n, PTR)
    d.layers, d.grads = C.cast(keep[0], C.POINTER(_lib.HphLayer)), C.cast(keep[1], C.POINTER(_lib.HphLayerGrads))
    for n in ("x0", "ctx16", "gstart", "chunks", "g_x_out", "g_x0", "workspace"):
        setattr(d, n, PTR)
    d.workspace_bytes = 1 << 40
    for k, v in over.items():
        setattr(d, k, v)
    d._keep = keep
    return d


def test_stack_backward_validation(L):
    call = lambda **o: L.mhmr_xattn_layers_backward(C.byref(_stack_desc(**o)), None)
    assert L.mhmr_xattn_layers_backward(None, None) == BAD_ARG
    assert call(P=0) == 0
    for bad in (dict(P=-1), dict(depth=-1), dict(ngroups=-1), dict(nmax=-1), dict(nchunks=-1), dict(x0=None), dict(ctx16=None), dict(gstart=None),
                dict(chunks=None), dict(g_x_out=None), dict(g_x0=None), dict(workspace=None), dict(workspace_bytes=1024), dict(g_ctx=PTR),
                dict(ngroups=0), dict(nmax=0), dict(nchunks=0)):             # persons that no group / no work item covers
        assert call(**bad) == BAD_ARG, bad
    for bad in (dict(Kc=1100), dict(dim=1000), dict(dim=2112), dict(mlp=1000), dict(heads=0), dict(heads=3), dict(N=0), dict(B=0), dict(B=65536),
                dict(dtype=5), dict(ctx_valid=-1), dict(ctx_valid=1153), dict(P=16 * 65535 + 1, nmax=5)):
        assert call(**bad) == BAD_SHAPE, bad
    d = _stack_desc()
    d._keep[1][1].to_kv = None
    assert L.mhmr_xattn_layers_backward(C.byref(d), None) == BAD_ARG
    d = _stack_desc()
    d._keep[0][0].ff1_w = None
    assert L.mhmr_xattn_layers_backward(C.byref(d), None) == BAD_ARG


def _head_desc(**over):
    f = _lib.HphDesc()
    f.dtype, f.C, f.G, f.N, f.Kc, f.dim, f.heads, f.mlp, f.depth, f.nb, f.Ktok, f.Ndec, f.patch, f.nearness = (
        _lib.DT_F16, 384, 16, 256, 512, 1024, 8, 1024, 2, 10, 816, 341, 14, 1)
    f.cam_dim = 99
    layers = (_lib.HphLayer * 2)()
    for e in layers:
        for n, _ in e._fields_:
            setattr(e, n, PTR)
    f.layers = C.cast(layers, C.POINTER(_lib.HphLayer))
    for n, t in f._fields_:
        if t is _lib._vp:
            setattr(f, n, PTR)
    d = _lib.HphBackwardDesc()
    lg = (_lib.HphLayerGrads * 2)()
    for e in lg:
        for n, _ in e._fields_:
            setattr(e, n, PTR)
    d.layer_grads = C.cast(lg, C.POINTER(_lib.HphLayerGrads))
    for n, t in d._fields_:
        if t is _lib._vp:
            setattr(d, n, PTR)
    d.ngroups, d.nmax, d.nchunks, d.P, d.B, d.ldg, d.workspace_bytes = 2, 5, 3, 5, 2, 341, 1 << 40
    fo = {k[4:]: v for k, v in over.items() if k.startswith("fwd_")}
    for k, v in fo.items():
        setattr(f, k, v)
    d.fwd = C.pointer(f)
    for k, v in over.items():
        if not k.startswith("fwd_"):
            setattr(d, k, v)
    d._keep = (f, layers, lg)
    return d


def test_head_backward_validation(L):
    call = lambda **o: L.mhmr_hph_backward(C.byref(_head_desc(**o)), None)
    assert L.mhmr_hph_backward(None, None) == BAD_ARG
    d = _head_desc()
    d.fwd = None
    assert L.mhmr_hph_backward(C.byref(d), None) == BAD_ARG
    assert call(P=0) == 0
    ptrs = ["ctx16", "det_y", "det_x", "gstart", "chunks", "g_readout", "g_offset", "g_zc", "g_token", "workspace"] + list(_lib.HphBackwardDesc.GRADS)
    for bad in ([dict(P=-1), dict(ngroups=-1), dict(ngroups=0), dict(nmax=0), dict(nchunks=0), dict(workspace_bytes=4096), dict(layer_grads=None), dict(fwd_depth=-1)] + [{p: None} for p in ptrs] +
                [{"fwd_" + p: None} for p in ("off1_w", "off2_w", "tok_w", "tok_b", "dec_w", "zc", "token", "x", "det_row")]):
        assert call(**bad) == BAD_ARG, bad
    for bad in (dict(fwd_Ktok=810), dict(fwd_Kc=500), dict(fwd_C=380), dict(fwd_nb=65), dict(fwd_Ndec=340), dict(fwd_Ktok=800), dict(fwd_dim=1000),
                dict(fwd_mlp=1001), dict(fwd_heads=0), dict(ldg=340), dict(B=0), dict(fwd_dtype=3), dict(fwd_cam_dim=200)):
        assert call(**bad) == BAD_SHAPE, bad
    f = _head_desc()._keep[0]
    assert L.mhmr_hph_backward_workspace_bytes(None, 2, 5) == BAD_ARG and L.mhmr_hph_backward_workspace_bytes(C.byref(f), 2, -1) == BAD_ARG
    assert L.mhmr_hph_backward_workspace_bytes(C.byref(f), 0, 5) == BAD_SHAPE


def test_workspace_sizes_are_monotone_and_non_negative(L):
    f = _head_desc()._keep[0]
    prev = [-1, -1, -1, -1]
    for P in (0, 1, 2, 15, 16, 17, 64, 130, 256, 1000):
        cur = [L.mhmr_xattn_layers_backward_workspace_bytes(2, 1024, 8, 1024, 1152, 256, 2, P), L.mhmr_hph_backward_workspace_bytes(C.byref(f), 2, P),
               L.mhmr_layernorm_f32_backward_workspace_bytes(P, 1024), L.mhmr_grad_ctx_gemm_workspace_bytes(P * 37, 512, 1152)]
        assert all(c >= 0 and c >= p for c, p in zip(cur, prev)), (P, cur, prev)
        prev = cur
    by_depth = [L.mhmr_xattn_layers_backward_workspace_bytes(dp, 512, 16, 2048, 512, 256, 4, 40) for dp in (0, 1, 2, 8)]
    assert by_depth == sorted(by_depth) and by_depth[0] >= 0
    by_B = [L.mhmr_xattn_layers_backward_workspace_bytes(2, 1024, 8, 1024, 1152, 4096, B, 40) for B in (1, 2, 32)]
    assert by_B == sorted(by_B)
    assert L.mhmr_xattn_layers_backward_workspace_bytes(2, 1024, 8, 1024, 1152, 256, 2, -1) == BAD_ARG
    assert L.mhmr_xattn_layers_backward_workspace_bytes(2, 1000, 8, 1024, 1152, 256, 2, 5) == BAD_SHAPE


# ------------------------------------------------------------------------------------------------------ the gradient mapping
def test_packed_gradients_map_onto_the_parameters():
    """Slices (tok_w, to_kv), the dec_w / dec_b split and the folded biases, on CPU tensors: packing a parameter-shaped set of tensors the
    way Model._head_tensors packs the weights and mapping it back returns the same tensors."""
    C_, E, nb, dim, inner, mlp, depth, G = 384, 99, 10, 1024, 256, 1024, 2, 16
    Cc, Kc, Ktok, Ndec = C_ + E, 512, 816, 341
    names = heads_train.head_parameter_names(depth)
    assert len(names) == len(set(names)) == 4 + 7 + 17 * depth + 8
    g = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.empty(*s).normal_(0, 1, generator=g)
    packed = {"g_off1_w": rnd(C_, C_), "g_off1_b": rnd(C_), "g_off2_w": rnd(2, C_), "g_off2_b": rnd(2), "g_tok_w": rnd(dim, Ktok), "g_tok_b": rnd(dim),
              "g_dec_w": rnd(Ndec, dim), "g_dec_b": rnd(Ndec), "g_cq_x": rnd(G, Cc), "g_cq_y": rnd(G, Cc), "g_cv_x": rnd(G, Cc), "g_cv_y": rnd(G, Cc)}
    assert set(packed) == set(_lib.HphBackwardDesc.GRADS)
    shapes = heads_train.layer_grad_shapes(inner, dim, mlp, Kc)
    layers = [{n: rnd(*shapes[n]) for n in _lib.HphLayerGrads.FIELDS} for _ in range(depth)]
    out = heads_train.packed_to_parameter_grads(packed, layers, Cc, nb, dim)
    assert set(out) == set(names)
    h = "x_attention_head."
    assert torch.equal(out[h + "transformer.to_token_embedding.weight"], packed["g_tok_w"][:, :Cc + 318 + nb + 3])
    assert torch.equal(out[h + "transformer.pos_embedding"][0, 0], packed["g_tok_b"]) and out[h + "transformer.pos_embedding"].shape == (1, 1, dim)
    assert torch.equal(out[h + "transformer.to_token_embedding.bias"], packed["g_tok_b"])
    assert torch.equal(torch.cat([out[h + m + ".weight"] for m in heads_train.DEC_PARTS]), packed["g_dec_w"])
    assert torch.equal(torch.cat([out[h + m + ".bias"] for m in heads_train.DEC_PARTS]), packed["g_dec_b"])
    assert [out[h + m + ".weight"].shape[0] for m in heads_train.DEC_PARTS] == [318, nb, 3, 10]
    for l in range(depth):
        t = f"{h}transformer.transformer.layers.{l}."
        assert torch.equal(out[t + "1.fn.to_kv.weight"], layers[l]["to_kv"][:, :Cc])
        assert out[t + "0.fn.to_qkv.weight"] is layers[l]["to_qkv"] and out[t + "2.fn.net.3.bias"] is layers[l]["ff2_b"]
        assert out[t + "1.norm.weight"] is layers[l]["ln_ca_w"] and out[t + "2.fn.net.0.weight"] is layers[l]["ff1_w"]
    assert out["mlp_offset.2.weight"] is packed["g_off2_w"] and out[h + "cross_values_y"] is packed["g_cv_y"]


def test_head_parameter_names_are_the_models_head_parameters():
    """heads_parameters() is every parameter of mlp_offset and x_attention_head, requires_grad False until train_heads_(True)."""
    import synthetic
    from multi_hmr_amd import Model
    m = Model(backbone="dinov2_vits14", img_size=224, smplx_data=synthetic.make_smplx_data(seed=0), mean_params=synthetic.make_mean_params(seed=0),
              backbone_depth=1)
    want = [k for k, _ in m.named_parameters() if k.startswith(("mlp_offset.", "x_attention_head."))]
    assert sorted(heads_train.head_parameter_names(m.xat_depth)) == sorted(want)
    assert not any(p.requires_grad for p in m.parameters())
    m.train_heads_(True)
    on = {k for k, p in m.named_parameters() if p.requires_grad}
    assert on == set(want) and len(m.heads_parameters()) == len(want)
    m.train_heads_(False)
    assert not any(p.requires_grad for p in m.parameters())
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 224, 224), train_heads=True)
    m.repack_heads()                                  # nothing packed yet: a no-op


def test_workspace_bytes_returns_the_count_and_raises_on_an_error_code(L):
    """_lib.workspace_bytes: the values tests/test_heads_backward_host.py asserts on the raw entry."""
    assert _lib.workspace_bytes("mhmr_heads_place_workspace_bytes", 10475, 127, 3) == 3 * 12 * 24
    assert _lib.workspace_bytes("mhmr_heads_place_workspace_bytes", 10475, 127, 0) == 0
    with pytest.raises(_lib.MhmrError, match="mhmr_heads_place_workspace_bytes failed: bad argument"):
        _lib.workspace_bytes("mhmr_heads_place_workspace_bytes", 0, 127, 1)


def test_call_switches():
    """model.call_switches: one record of what a forward call's keywords ask for; no device, no model."""
    from multi_hmr_amd.model import Switches, call_switches
    off = Switches(False, False, False, False, False, False)
    assert call_switches(False, {}) == off and call_switches(True, {}, from_features=True) == off
    assert Switches._fields == ("with_ids", "batched", "with_readout", "train_heads", "train_detection", "train_backbone")
    every = dict(return_image_index=1, return_batched=True, return_readout=True, train_heads=True, train_detection=True, train_backbone=True)
    assert call_switches(True, every) == Switches(True, True, True, True, True, True)
    assert all(type(v) is bool for v in call_switches(True, every))
    assert call_switches(False, dict(return_batched=True, return_image_index=True)) == off._replace(with_ids=True, batched=True)
    with pytest.raises(AttributeError):
        call_switches(True, every).train_heads = False                       # immutable
    # the three invalid combinations, for both callers where both read the switch
    for ff in (False, True):
        with pytest.raises(ValueError, match="^train_detection=True needs is_training=True$"):
            call_switches(False, dict(train_detection=True), from_features=ff)
        for kw in (dict(train_heads=True), dict(train_heads=True, return_readout=True)):
            with pytest.raises(ValueError, match="^train_heads=True needs is_training=True and return_readout=True$"):
                call_switches(False, kw, from_features=ff)
        with pytest.raises(ValueError, match="^train_heads=True needs is_training=True and return_readout=True$"):
            call_switches(True, dict(train_heads=True), from_features=ff)
    with pytest.raises(ValueError, match="^train_backbone=True needs is_training=True$"):
        call_switches(False, dict(train_backbone=True))
    # forward_features has no backbone to train: the keyword is not read there, in either mode
    assert call_switches(False, dict(train_backbone=True), from_features=True) == off
    assert call_switches(True, dict(train_backbone=True, train_detection=True), from_features=True) == off._replace(train_detection=True)
    assert call_switches(True, dict(train_backbone=True)) == off._replace(train_backbone=True)
    # keywords that are none of ours are ignored, as the reference's *args, **kwargs ignores them
    assert call_switches(False, dict(verbose=True, return_readout=True, train_everything=True)) == off._replace(with_readout=True)


# ------------------------------------------------------------------------------------------------------ the oracle itself
def _fd_check(f, leaves, grads, seed, tag):
    """Central differences of the fp64 scalar f(leaves) along four seeded directions against <grads, direction>; gate 1e-6 relative."""
    g = torch.Generator().manual_seed(seed)
    for n in range(4):
        dirs = [torch.empty(t.shape, dtype=torch.float64).normal_(0, 1, generator=g) * float(t.abs().mean() + 1e-3) for t in leaves]
        h = 1e-6
        with torch.no_grad():
            fp = f([t + h * d for t, d in zip(leaves, dirs)])
            fm = f([t - h * d for t, d in zip(leaves, dirs)])
        fd = float(fp - fm) / (2 * h)
        an = float(sum((gr * d).sum() for gr, d in zip(grads, dirs)))
        rel = abs(fd - an) / abs(an)
        print(f"[{tag}] direction {n}: finite difference {fd:.9e}, autograd {an:.9e}, relative {rel:.2e}")
        assert rel < 1e-6, (tag, n, rel)


@pytest.mark.parametrize("name", list(ho.STACK_CASES))
def test_stack_oracle_against_finite_differences(name):
    case = ho.stack_case(name)
    sd, x, ctx = ho.stack_operands(case, "f16", torch.float64)
    names = list(sd)
    grads = ho.stack_grads(case, "f16", torch.float64)

    def f(leaves):
        return ho.stack_scalar(case, dict(zip(names, leaves[1:])), leaves[0], ctx)
    _fd_check(f, [x] + [sd[k] for k in names], [grads["x"]] + [grads[k] for k in names], 40, f"stack {name}")


def test_head_oracle_against_finite_differences():
    """The whole-head oracle without the 16-bit rounding (a step function under a finite difference; its straight-through gradient is a
    convention): parameters, g_zc and g_token along four directions."""
    import synthetic
    mean = synthetic.make_mean_params(seed=0)
    sd_all = synthetic.make_state_dict("dinov2_vits14", 224, seed=42, depth_override=1, mean_params=mean)
    g = torch.Generator().manual_seed(5)
    B, G, C_ = 3, 16, 384
    feat = torch.empty(B, G * G, C_, dtype=torch.float64).normal_(0, 1, generator=g)
    K = torch.zeros(B, 3, 3, dtype=torch.float64)
    K[:, 0, 0] = K[:, 1, 1] = 250.0
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 113.0, 110.0, 1.0
    idx = (torch.tensor([0, 0, 0, 2]), torch.tensor([3, 3, 9, 7]), torch.tensor([2, 11, 4, 4]))
    cr, co = torch.empty(4, 341, dtype=torch.float64).normal_(0, 1, generator=g), torch.empty(4, 2, dtype=torch.float64).normal_(0, 1, generator=g)
    grads, _, _ = ho.head_grads(sd_all, feat, K, idx, cr, co, 2, 8, G, None, torch.float64)
    sd = ho.head_operands(sd_all, None, torch.float64)
    names = [k for k in sd if "init_" not in k]
    rows = idx[1] * G + idx[2]
    zK = ho.embedd_camera(K, G).reshape(B, G * G, -1)
    zc, zq = feat[idx[0], rows], torch.cat([feat[idx[0], rows], zK[idx[0], rows]], 1)

    def f(leaves):
        s = dict(sd)
        s.update(zip(names, leaves[2:]))
        ro, off = ho.head_forward(s, leaves[0], leaves[1], feat, K, idx, 2, 8, G, None)
        return (ro * cr).sum() + (off * co).sum()
    _fd_check(f, [zc, zq] + [sd[k] for k in names], [grads["g_zc"], grads["g_token"]] + [grads[k] for k in names], 41, "head")
