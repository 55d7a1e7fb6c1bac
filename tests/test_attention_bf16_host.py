"""-m "not gpu": the host side of the attention with bf16 operands -- the new entries are declared, exported and
bound; every validation rule answers before a launch (so these calls run without a GPU); the `_pa` workspace sizes extend the `_p`
ones; the oracle with its rounding switched off is the existing closed form; and the Python surface (Model.train_backbone_, the training
command line) accepts and refuses what it should."""
import ctypes as C
import os
import re

import pytest
import torch

import attention_bf16_oracle as ao
import backbone_bwd_oracle as bo
import linear_bf16_oracle as lo
from multi_hmr_amd import _lib

PTR = 0x10000          # a non-NULL, 16-byte aligned address that is never dereferenced: validation comes before any launch
BAD_ARG, BAD_SHAPE = -1, -2
NEW = {"mhmr_attention_bf16_workspace_bytes", "mhmr_attention_bf16_tape", "mhmr_attention_bf16_backward",
       "mhmr_vit_block_backward_workspace_bytes_pa", "mhmr_vit_tail_backward_workspace_bytes_pa", "mhmr_vit_block_backward_a",
       "mhmr_vit_tail_backward_a"}


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _ws(L, B, Tp, Cd, H):
    n = int(L.mhmr_attention_bf16_workspace_bytes(B, Tp, Cd, H))
    return n if n > 0 else 1 << 40


def _tape(L, qkv=PTR, out32=PTR, lse=PTR, B=2, T=17, Tp=64, Cd=128, H=2, ws=PTR, nbytes=None):
    return L.mhmr_attention_bf16_tape(qkv, out32, lse, B, T, Tp, Cd, H, ws, _ws(L, B, Tp, Cd, H) if nbytes is None else nbytes, None)


def _bwd(L, qkv=PTR, out32=PTR, lse=PTR, dO=PTR, lddo=None, dqkv=PTR, B=2, T=17, Tp=64, Cd=128, H=2, ws=PTR, nbytes=None):
    return L.mhmr_attention_bf16_backward(qkv, out32, lse, dO, Cd if lddo is None else lddo, dqkv, B, T, Tp, Cd, H, ws,
                                          _ws(L, B, Tp, Cd, H) if nbytes is None else nbytes, None)


def test_new_entries_are_declared_exported_and_bound(L):
    assert NEW <= set(_lib.EXPORTS) and all(hasattr(L, n) for n in NEW)
    assert _lib.VERSION == 106 and L.mhmr_version() == 106 and "attention_bf16.hip" in _lib.SOURCES
    with open(os.path.join(os.path.dirname(_lib.HERE), "include", "mhmr.h")) as f:
        header = f.read()
    for n in NEW:
        assert re.search(r"\b" + n + r"\(", header), n
    assert re.search(r"#define MHMR_ATTN_F32 0\b", header) and re.search(r"#define MHMR_ATTN_BF16 1\b", header)
    assert re.search(r"#define MHMR_VERSION 106\b", header)
    # the descriptors did not grow: the switch is an argument
    for cls in (_lib.VitBlockBackwardDesc, _lib.VitTailBackwardDesc):
        assert [f[0] for f in cls._fields_][-2:] == ["workspace_bytes", "linear_precision"]
    assert _lib.ATTN_PRECISIONS == {"f32": 0, "bf16": 1} and _lib.attn_precision("f32") == 0 and _lib.attn_precision("bf16") == 1
    for bad in ("fp8", "f16", None, 1):
        with pytest.raises(ValueError):
            _lib.attn_precision(bad)
    assert _lib.bwd_precision("bf16") == 1 and set(_lib.BWD_PRECISIONS) == {"f32", "bf16"}


def test_attention_entries_validate_before_any_launch(L):
    full = _ws(L, 2, 64, 128, 2)
    for call in (_tape, _bwd):
        for kw in (dict(B=-1), dict(T=-1), dict(Tp=-64), dict(Cd=-128), dict(H=-2), dict(ws=None), dict(nbytes=0), dict(nbytes=full - 1),
                   dict(ws=PTR + 8), dict(qkv=None), dict(out32=None), dict(lse=None), dict(qkv=PTR + 4), dict(out32=PTR + 8)):
            assert call(L, **kw) == BAD_ARG, (call.__name__, kw)
        for kw in (dict(B=0), dict(T=0), dict(Tp=96), dict(T=65), dict(Cd=192), dict(H=3), dict(B=65536, Tp=64), dict(B=65535, Tp=128)):
            assert call(L, **kw) == BAD_SHAPE, (call.__name__, kw)
    for kw in (dict(dO=None), dict(dqkv=None), dict(dO=PTR + 4), dict(dqkv=PTR + 8), dict(lse=PTR + 4)):
        assert _bwd(L, **kw) == BAD_ARG, kw
    for kw in (dict(lddo=124), dict(lddo=130), dict(lddo=64)):
        assert _bwd(L, **kw) == BAD_SHAPE, kw
    wb = L.mhmr_attention_bf16_workspace_bytes
    assert wb(-1, 64, 128, 2) == BAD_ARG and wb(1, -64, 128, 2) == BAD_ARG and wb(1, 64, -128, 2) == BAD_ARG and wb(1, 64, 128, -2) == BAD_ARG
    assert wb(0, 64, 128, 2) == BAD_SHAPE and wb(1, 65, 128, 2) == BAD_SHAPE and wb(1, 64, 128, 3) == BAD_SHAPE and wb(1, 0, 128, 2) == BAD_SHAPE
    # one size for both entries: bf16 copies of qkv and dO as they lie, three transposed copies, D
    assert wb(2, 64, 128, 2) >= 2 * 64 * 128 * 2 * 7 + 2 * 2 * 64 * 4
    assert 0 < wb(1, 64, 64, 1) < wb(2, 64, 64, 1) < wb(2, 128, 64, 1) < wb(2, 128, 128, 2)


def _block_desc(L, precision, attention, **over):
    d = _lib.VitBlockBackwardDesc()
    d.B, d.T, d.Tp, d.C, d.H = 2, 17, 64, 128, 2
    for n, t in d._fields_:
        if t is _lib._vp:
            setattr(d, n, PTR)
    d.g_in = PTR + 64
    d.linear_precision = precision
    d.workspace_bytes = int(L.mhmr_vit_block_backward_workspace_bytes_pa(2, 64, 128, precision, attention if attention in (0, 1) else 0))
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_attention_precision_argument_and_pa_sizes(L):
    bp, bpa = L.mhmr_vit_block_backward_workspace_bytes_p, L.mhmr_vit_block_backward_workspace_bytes_pa
    tp, tpa = L.mhmr_vit_tail_backward_workspace_bytes_p, L.mhmr_vit_tail_backward_workspace_bytes_pa
    for B, Tp, Cd in ((1, 64, 64), (2, 64, 128), (2, 320, 384), (8, 4160, 1024)):
        att = int(L.mhmr_attention_bf16_workspace_bytes(B, Tp, Cd, Cd // 64))
        for p in (0, 1):
            assert bpa(B, Tp, Cd, p, 0) == bp(B, Tp, Cd, p) > 0 and tpa(B, Tp, Cd, p, 0) == tp(B, Tp, Cd, p) > 0
            assert bpa(B, Tp, Cd, p, 1) > bpa(B, Tp, Cd, p, 0) and tpa(B, Tp, Cd, p, 1) > tpa(B, Tp, Cd, p, 0)
            assert bpa(B, Tp, Cd, p, 1) - bpa(B, Tp, Cd, p, 0) == att == tpa(B, Tp, Cd, p, 1) - tpa(B, Tp, Cd, p, 0)
    for fn in (bpa, tpa):
        for bad in (2, -1, 7):
            assert fn(2, 64, 128, 0, bad) == BAD_ARG and fn(2, 64, 128, bad, 1) == BAD_ARG
        assert fn(-1, 64, 128, 1, 1) == BAD_ARG
        assert fn(1, 65, 128, 1, 1) == BAD_SHAPE and fn(1, 64, 100, 0, 1) == BAD_SHAPE and fn(0, 64, 128, 1, 1) == BAD_SHAPE
    # the block: any other attention_precision is refused; mode 1 wants the `_pa` size; all four combinations pass the same other checks
    blk = L.mhmr_vit_block_backward_a
    for bad in (2, -1, 7):
        assert blk(C.byref(_block_desc(L, 0, bad)), bad, None) == BAD_ARG
        assert blk(C.byref(_block_desc(L, bad, 1, workspace_bytes=1 << 40)), 1, None) == BAD_ARG
    assert blk(None, 1, None) == BAD_ARG
    for p in (0, 1):
        small = int(bpa(2, 64, 128, p, 0))
        assert blk(C.byref(_block_desc(L, p, 1, workspace_bytes=small)), 1, None) == BAD_ARG
        assert blk(C.byref(_block_desc(L, p, 1, workspace_bytes=int(bpa(2, 64, 128, p, 1)) - 1)), 1, None) == BAD_ARG
        assert blk(C.byref(_block_desc(L, p, 1, workspace=PTR + 8)), 1, None) == BAD_ARG
        assert blk(C.byref(_block_desc(L, p, 1, Tp=96)), 1, None) == BAD_SHAPE
        for a in (0, 1):
            for n, t in _lib.VitBlockBackwardDesc._fields_:
                if t is _lib._vp:
                    assert blk(C.byref(_block_desc(L, p, a, **{n: None})), a, None) == BAD_ARG, (p, a, n)
    # the tail hands its argument to every block and checks it, and the size, before any launch
    blocks = (_lib.VitBlockBackwardDesc * 1)()
    for n, t in blocks[0]._fields_:
        if t is _lib._vp:
            setattr(blocks[0], n, PTR)

    def tail(precision, attention, nbytes):
        d = _lib.VitTailBackwardDesc()
        d.B, d.N, d.T, d.Tp, d.C, d.H, d.n = 2, 16, 17, 64, 128, 2, 1
        for n, t in d._fields_:
            if t is _lib._vp:
                setattr(d, n, PTR)
        d.blocks = C.cast(blocks, C.POINTER(_lib.VitBlockBackwardDesc))
        d.linear_precision, d.workspace_bytes = precision, nbytes
        return L.mhmr_vit_tail_backward_a(C.byref(d), attention, None)
    assert tail(0, 2, 1 << 40) == BAD_ARG and tail(1, -1, 1 << 40) == BAD_ARG and tail(2, 1, 1 << 40) == BAD_ARG
    for p in (0, 1):
        assert tail(p, 1, int(tpa(2, 64, 128, p, 0))) == BAD_ARG and tail(p, 1, int(tpa(2, 64, 128, p, 1)) - 1) == BAD_ARG
        assert tail(p, 0, int(tpa(2, 64, 128, p, 0)) - 1) == BAD_ARG
    assert L.mhmr_vit_tail_backward_a(None, 1, None) == BAD_ARG


# ------------------------------------------------------------------------------------------------------ the oracle
def _operands(T, Tp, B=2, H=2, seed=11):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.empty(B * Tp, 3 * 64 * H).normal_(0, 1, generator=g)
    qkv[:, :64 * H] *= 2.0
    return qkv, torch.empty(B * Tp, 64 * H).normal_(0, 1, generator=g)


@pytest.mark.parametrize("T,Tp", [(2, 64), (17, 64), (65, 128)])
def test_oracle_without_rounding_is_the_closed_form(T, Tp):
    B, H, Cd = 2, 2, 128
    qkv, dO = _operands(T, Tp)
    out, lse, dqkv = ao.attention_closed_form(qkv, dO, B, T, Tp, H, rounding=False)
    o64, l64 = bo.attention_forward(qkv, B, T, Tp, H)
    d64 = bo.attention_backward_closed_form(qkv, dO, B, T, Tp, H)
    for name, a, b in (("out", out, o64), ("lse", lse, l64), ("dqkv", dqkv, d64)):
        assert a.dtype == torch.float64 and a.shape == b.shape
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), name
    # with the rounding on it is another function, by about bf16's half ulp per rounded operand; its padding rows stay zeros
    ro, rl, rd = ao.attention_closed_form(qkv, dO, B, T, Tp, H)
    for i, name in enumerate(("dQ", "dK", "dV")):
        rel = bo.measure(rd[:, i * Cd:(i + 1) * Cd], d64[:, i * Cd:(i + 1) * Cd])[0]
        print(f"[oracle T {T}] {name}: rounded against unrounded, rel L2 {rel:.3e}")
        assert 1e-3 < rel < 3e-2, (name, rel)
    pad = torch.arange(B * Tp) % Tp >= T
    assert bool((rd[pad] == 0).all()) and bool((ro[pad] == 0).all()) and bool((rl[:, :, T:] == 0).all())
    # a longer pitch of dO reads the same columns
    wide = torch.cat([dO, torch.full((B * Tp, 8), 3.0)], 1)
    assert torch.equal(ao.attention_closed_form(qkv, wide, B, T, Tp, H)[2], rd)


def test_autograd_function_is_the_closed_form():
    B, H, T, Tp, Cd = 2, 2, 33, 64, 128
    qkv, dO = _operands(T, Tp, seed=12)
    for dtype in (torch.float64, torch.float32):
        for rounding in (True, False):
            out, _, dqkv = ao.attention_closed_form(qkv, dO, B, T, Tp, H, dtype, rounding)
            x = qkv.to(dtype).clone().requires_grad_()
            q, k, v = (x.reshape(B, Tp, 3, H, 64)[:, :T, i].permute(0, 2, 1, 3) for i in range(3))
            o = ao.RoundedAttention.apply(q, k, v, rounding).permute(0, 2, 1, 3).reshape(B, T, Cd)
            assert torch.equal(o.detach(), out.reshape(B, Tp, Cd)[:, :T])
            (o * dO.to(dtype).reshape(B, Tp, Cd)[:, :T]).sum().backward()
            assert torch.equal(x.grad, dqkv), (dtype, rounding)


def test_rounded_attention_in_the_block_oracle():
    blk = bo.make_block(128, 2, seed=3)
    g = torch.Generator().manual_seed(1)
    x, go = torch.empty(2 * 64, 128).normal_(0, 1, generator=g), torch.empty(2 * 64, 128).normal_(0, 1, generator=g)
    ref = bo.block_backward(blk, x, go, 2, 17, 64)
    # the swapped module without rounding is the module
    plain = bo.block_backward(ao.with_rounded_attention(blk, rounding=False), x, go, 2, 17, 64)
    for k in ref:
        assert float((plain[k] - ref[k]).abs().max()) <= 1e-12 * float(ref[k].abs().max()), k
    both = ao.rounded_block_backward(blk, x, go, 2, 17, 64)
    only_lin = ao.rounded_block_backward(blk, x, go, 2, 17, 64, attention=False)
    only_att = ao.rounded_block_backward(blk, x, go, 2, 17, 64, linears=False)
    neither = ao.rounded_block_backward(blk, x, go, 2, 17, 64, linears=False, attention=False)
    lin = lo.rounded_block_backward(blk, x, go, 2, 17, 64)
    assert all(torch.equal(only_lin[k], lin[k]) for k in lin) and all(torch.equal(neither[k], ref[k]) for k in ref)
    for k in ("g_in", "qkv_w", "ln1_w"):
        assert not torch.equal(both[k], lin[k]) and not torch.equal(only_att[k], ref[k]), k
        assert 1e-5 < bo.measure(only_att[k], ref[k])[0] < 3e-2, k
    assert bool((both["g_in"].reshape(2, 64, 128)[:, 17:] == 0).all())
    assert all(p.grad is None for p in blk.parameters()) and type(blk.attn).forward is blk.attn.forward.__func__      # the block is untouched


# ------------------------------------------------------------------------------------------------------ the Python surface
def test_train_backbone_attention(smplx_data, mean_params):
    from multi_hmr_amd import Model
    m = Model(backbone="dinov2_vits14", img_size=224, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=3)
    assert m._backbone_attention == "f32" and m._backbone_precision == "f32"
    assert m.train_backbone_(1) is m and m._backbone_attention == "f32"
    assert m.train_backbone_(2, attention="bf16") is m and m._backbone_attention == "bf16" and m._backbone_precision == "f32" and m._backbone_n == 2
    m.train_backbone_(1, precision="bf16")                     # None keeps the setting
    assert m._backbone_attention == "bf16" and m._backbone_precision == "bf16" and m._backbone_n == 1
    for kw in (dict(attention="fp8"), dict(precision="f32", attention=1), dict(precision="fp8", attention="f32")):
        with pytest.raises(ValueError):
            m.train_backbone_(3, **kw)
        assert (m._backbone_attention, m._backbone_precision, m._backbone_n) == ("bf16", "bf16", 1)      # a refused call changes nothing
    m.train_backbone_(1, attention="f32")
    assert m._backbone_attention == "f32" and m._backbone_precision == "bf16"


def test_command_line_has_the_attention_switch():
    from multi_hmr_amd import train
    p = train.build_parser()
    a = p.parse_args(["--pretrained", "x"])
    assert a.amp == 1 and a.amp_attention == 0
    a = p.parse_args(["--pretrained", "x", "--train_backbone", "2", "--amp_attention", "1"])
    assert a.train_backbone == 2 and a.amp == 1 and a.amp_attention == 1
    for bad in (["--amp_attention", "2"], ["--amp", "2"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--pretrained", "x"] + bad)


def test_make_optimizer_passes_the_attention_switch(smplx_data, mean_params):
    from multi_hmr_amd import Model, train
    new = lambda: Model(backbone="dinov2_vits14", img_size=224, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=3).train_heads_(True)
    p = train.build_parser()
    for argv, prec, att in ((["--train_backbone", "2"], "bf16", "f32"), (["--train_backbone", "2", "--amp_attention", "1"], "bf16", "bf16"),
                            (["--train_backbone", "3", "--amp", "0", "--amp_attention", "1"], "f32", "bf16")):
        m = new().train_detection_(True)
        opt = train.make_optimizer(m, p.parse_args(["--pretrained", "x"] + argv))
        assert isinstance(opt, torch.optim.Adam) and (m._backbone_precision, m._backbone_attention) == (prec, att)
