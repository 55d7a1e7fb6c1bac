"""-m "not gpu": the host side of the mixed-precision backbone backward -- the bf16 linear entries and the
precision field of the two backward descriptors validate their arguments before any launch (so these calls run without a GPU), the `_p`
workspace sizes extend the old ones, the rounding oracle with its rounding switched off is the existing block oracle, and the Python
surface (Model.train_backbone_, the training command line) accepts and refuses what it should."""
import ctypes as C

import pytest
import torch

import backbone_bwd_oracle as bo
import linear_bf16_oracle as lo
from multi_hmr_amd import _lib

PTR = 0x10000          # a non-NULL, 16-byte aligned address that is never dereferenced: validation comes before any launch
BAD_ARG, BAD_SHAPE = -1, -2
NEW = {"mhmr_linear_bf16_workspace_bytes", "mhmr_linear_bf16", "mhmr_linear_bf16_backward_input", "mhmr_linear_bf16_backward_weight",
       "mhmr_vit_block_backward_workspace_bytes_p", "mhmr_vit_tail_backward_workspace_bytes_p"}


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _ws(L, M, N, K):
    n = int(L.mhmr_linear_bf16_workspace_bytes(M, N, K))
    return n if n > 0 else 1 << 40


def _fwd(L, X=PTR, ldx=None, W=PTR, ldw=None, bias=PTR, Y=PTR, ldy=None, M=128, N=192, K=64, ws=PTR, nbytes=None):
    return L.mhmr_linear_bf16(X, K if ldx is None else ldx, W, K if ldw is None else ldw, bias, Y, N if ldy is None else ldy, M, N, K, ws,
                              _ws(L, M, N, K) if nbytes is None else nbytes, None)


def _bin(L, dY=PTR, lddy=None, W=PTR, ldw=None, dR=PTR, lddr=None, dX=PTR, lddx=None, M=128, N=192, K=64, ws=PTR, nbytes=None):
    return L.mhmr_linear_bf16_backward_input(dY, N if lddy is None else lddy, W, K if ldw is None else ldw, dR, K if lddr is None else lddr, dX,
                                             K if lddx is None else lddx, M, N, K, ws, _ws(L, M, N, K) if nbytes is None else nbytes, None)


def _bw(L, dY=PTR, lddy=None, X=PTR, ldx=None, dW=PTR, lddw=None, db=PTR, M=128, N=192, K=64, ws=PTR, nbytes=None):
    return L.mhmr_linear_bf16_backward_weight(dY, N if lddy is None else lddy, X, K if ldx is None else ldx, dW, K if lddw is None else lddw, db,
                                              M, N, K, ws, _ws(L, M, N, K) if nbytes is None else nbytes, None)


def test_new_entries_are_bound_and_the_version_stays(L):
    assert NEW <= set(_lib.EXPORTS) and all(hasattr(L, n) for n in NEW)
    assert _lib.VERSION == 106 and L.mhmr_version() == 106 and "linear_bf16.hip" in _lib.SOURCES
    # appended fields: zero (a fresh descriptor) is the fp32 mode, every older field keeps its offset
    for cls in (_lib.VitBlockBackwardDesc, _lib.VitTailBackwardDesc):
        assert [f[0] for f in cls._fields_][-2:] == ["workspace_bytes", "linear_precision"]
        assert cls().linear_precision == 0 == _lib.BWD_F32
    assert _lib.bwd_precision("f32") == 0 and _lib.bwd_precision("bf16") == 1
    for bad in ("fp8", "f16", None, 1):
        with pytest.raises(ValueError):
            _lib.bwd_precision(bad)


def test_linear_entries_validate_before_any_launch(L):
    for call in (_fwd, _bin, _bw):
        for kw in (dict(M=-64), dict(N=-64), dict(K=-64), dict(ws=None), dict(nbytes=0), dict(nbytes=_ws(L, 128, 192, 64) - 1), dict(ws=PTR + 8)):
            assert call(L, **kw) == BAD_ARG, (call.__name__, kw)
        for kw in (dict(M=96), dict(N=100), dict(K=32), dict(K=96), dict(M=0), dict(N=0), dict(K=0), dict(M=16 * 65535 + 1), dict(M=16 * 65536)):
            assert call(L, **kw) == BAD_SHAPE, (call.__name__, kw)
    # NULL and misaligned pointers; the nullable ones are accepted as NULL but not misaligned
    for kw in (dict(X=None), dict(W=None), dict(Y=None), dict(X=PTR + 4), dict(W=PTR + 8), dict(Y=PTR + 4), dict(bias=PTR + 4)):
        assert _fwd(L, **kw) == BAD_ARG, kw
    for kw in (dict(dY=None), dict(W=None), dict(dX=None), dict(dY=PTR + 4), dict(W=PTR + 4), dict(dX=PTR + 8), dict(dR=PTR + 4)):
        assert _bin(L, **kw) == BAD_ARG, kw
    for kw in (dict(dY=None), dict(X=None), dict(dW=None, db=None), dict(dY=PTR + 4), dict(X=PTR + 4), dict(dW=PTR + 4)):
        assert _bw(L, **kw) == BAD_ARG, kw
    # leading dimensions: at least the row, a multiple of 4
    for kw in (dict(ldx=60), dict(ldx=66), dict(ldw=63), dict(ldy=188), dict(ldy=194)):
        assert _fwd(L, **kw) == BAD_SHAPE, kw
    for kw in (dict(lddy=191), dict(ldw=60), dict(lddr=62), dict(lddr=60), dict(lddx=63)):
        assert _bin(L, **kw) == BAD_SHAPE, kw
    for kw in (dict(lddy=190), dict(ldx=32), dict(lddw=65)):
        assert _bw(L, **kw) == BAD_SHAPE, kw
    wb = L.mhmr_linear_bf16_workspace_bytes
    assert wb(-64, 64, 64) == BAD_ARG and wb(64, -64, 64) == BAD_ARG and wb(64, 64, -1) == BAD_ARG
    assert wb(65, 64, 64) == BAD_SHAPE and wb(64, 32, 64) == BAD_SHAPE and wb(64, 64, 0) == BAD_SHAPE and wb(16 * 65535 + 64, 64, 64) == BAD_SHAPE
    # one size for the three products: the bf16 copies of both operands in either layout and one fp32 partial product per 4096 rows
    assert wb(64, 64, 64) >= 2 * 64 * 64 * 2 + 64 * 64 * 4
    assert wb(8192, 64, 128) >= 2 * (8192 * 128) * 2 + 2 * 64 * 128 * 4
    assert 0 < wb(64, 64, 64) < wb(128, 64, 64) < wb(128, 128, 64) < wb(128, 128, 128)


def _block_desc(L, precision, **over):
    d = _lib.VitBlockBackwardDesc()
    d.B, d.T, d.Tp, d.C, d.H = 2, 17, 64, 128, 2
    for n, t in d._fields_:
        if t is _lib._vp:
            setattr(d, n, PTR)
    d.g_in = PTR + 64
    d.linear_precision = precision
    d.workspace_bytes = int(L.mhmr_vit_block_backward_workspace_bytes_p(2, 64, 128, precision if precision in (0, 1) else 0))
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_precision_field_and_p_sizes(L):
    bb, bp = L.mhmr_vit_block_backward_workspace_bytes, L.mhmr_vit_block_backward_workspace_bytes_p
    tb, tp = L.mhmr_vit_tail_backward_workspace_bytes, L.mhmr_vit_tail_backward_workspace_bytes_p
    for B, Tp, Cd in ((1, 64, 64), (2, 64, 128), (2, 320, 384), (8, 4160, 1024)):
        assert bp(B, Tp, Cd, 0) == bb(B, Tp, Cd) > 0 and tp(B, Tp, Cd, 0) == tb(B, Tp, Cd) > 0
        lin = int(L.mhmr_linear_bf16_workspace_bytes(B * Tp, 4 * Cd, Cd))
        assert bp(B, Tp, Cd, 1) >= bb(B, Tp, Cd) + lin and tp(B, Tp, Cd, 1) - tb(B, Tp, Cd) == bp(B, Tp, Cd, 1) - bb(B, Tp, Cd)
    for fn in (bp, tp):
        assert fn(2, 64, 128, 2) == BAD_ARG and fn(2, 64, 128, -1) == BAD_ARG and fn(-1, 64, 128, 1) == BAD_ARG
        assert fn(1, 65, 128, 1) == BAD_SHAPE and fn(1, 64, 100, 1) == BAD_SHAPE and fn(0, 64, 128, 1) == BAD_SHAPE
    # the block: any other precision is refused; mode 1 wants the `_p` size and 16-byte aligned biases
    for bad in (2, -1, 7):
        assert L.mhmr_vit_block_backward(C.byref(_block_desc(L, bad)), None) == BAD_ARG
    small = int(bb(2, 64, 128))
    assert small < int(bp(2, 64, 128, 1))
    assert L.mhmr_vit_block_backward(C.byref(_block_desc(L, 1, workspace_bytes=small)), None) == BAD_ARG
    assert L.mhmr_vit_block_backward(C.byref(_block_desc(L, 1, workspace_bytes=int(bp(2, 64, 128, 1)) - 1)), None) == BAD_ARG
    assert L.mhmr_vit_block_backward(C.byref(_block_desc(L, 1, fc1_b=PTR + 4)), None) == BAD_ARG
    for n, t in _lib.VitBlockBackwardDesc._fields_:
        if t is _lib._vp:
            assert L.mhmr_vit_block_backward(C.byref(_block_desc(L, 1, **{n: None})), None) == BAD_ARG, n
    assert L.mhmr_vit_block_backward(C.byref(_block_desc(L, 1, Tp=96)), None) == BAD_SHAPE
    # the tail: its own field decides (the blocks' field is ignored), checked before any launch
    blocks = (_lib.VitBlockBackwardDesc * 1)()
    for n, t in blocks[0]._fields_:
        if t is _lib._vp:
            setattr(blocks[0], n, PTR)
    blocks[0].linear_precision = 9

    def tail(precision, nbytes):
        d = _lib.VitTailBackwardDesc()
        d.B, d.N, d.T, d.Tp, d.C, d.H, d.n = 2, 16, 17, 64, 128, 2, 1
        for n, t in d._fields_:
            if t is _lib._vp:
                setattr(d, n, PTR)
        d.blocks = C.cast(blocks, C.POINTER(_lib.VitBlockBackwardDesc))
        d.linear_precision, d.workspace_bytes = precision, nbytes
        return L.mhmr_vit_tail_backward(C.byref(d), None)
    assert tail(2, 1 << 40) == BAD_ARG and tail(-1, 1 << 40) == BAD_ARG
    assert tail(1, int(tb(2, 64, 128))) == BAD_ARG and tail(1, int(tp(2, 64, 128, 1)) - 1) == BAD_ARG and tail(0, int(tb(2, 64, 128)) - 1) == BAD_ARG


# ------------------------------------------------------------------------------------------------------ the oracle
def test_round_bf16_is_torch_bfloat16():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.3, 0.0, 3.0e38, 1e-40])
    r = lo.round_bf16(t)
    assert r.dtype == torch.float32 and torch.equal(r, t.bfloat16().float())
    assert r[1] == 1.0 and r[2] == 1.0 + 2.0 ** -6 and r[3] == 1.0 + 2.0 ** -7           # ties to even, above a tie upwards
    assert lo.round_bf16(t.double()).dtype == torch.float64 and torch.equal(lo.round_bf16(t.double()), r.double())
    assert torch.equal(lo.round_bf16(r), r)                                                  # idempotent


def test_rounding_oracle_without_rounding_is_the_block_oracle():
    blk = bo.make_block(128, 2, seed=3)
    g = torch.Generator().manual_seed(1)
    x, go = torch.empty(2 * 64, 128).normal_(0, 1, generator=g), torch.empty(2 * 64, 128).normal_(0, 1, generator=g)
    ref = bo.block_backward(blk, x, go, 2, 17, 64)
    plain = lo.rounded_block_backward(blk, x, go, 2, 17, 64, rounding=False)
    rounded = lo.rounded_block_backward(blk, x, go, 2, 17, 64)
    assert set(plain) == set(ref) == set(rounded)
    for k in ref:
        assert plain[k].dtype == torch.float64 and plain[k].shape == ref[k].shape
        assert float((plain[k] - ref[k]).abs().max()) <= 1e-12 * float(ref[k].abs().max()), k
    # with the rounding on it is a different function, by about bf16's half ulp, and its padding rows stay zeros
    for k in ("g_in", "qkv_w", "fc1_w", "fc2_w", "proj_w", "fc1_b"):
        rel = bo.measure(rounded[k], ref[k])[0]
        assert 1e-4 < rel < 3e-2, (k, rel)
    assert bool((rounded["g_in"].reshape(2, 64, 128)[:, 17:] == 0).all())
    assert all(p.grad is None for p in blk.parameters()) and blk.attn.qkv.weight.dtype == torch.float64      # the block itself is untouched
    # one linear: the three products of rounded operands, the bias sum of the unrounded cotangent
    X, W, b = torch.randn(8, 16, dtype=torch.float64, requires_grad=True), torch.randn(4, 16, dtype=torch.float64, requires_grad=True), \
        torch.randn(4, dtype=torch.float64, requires_grad=True)
    dY = torch.randn(8, 4, dtype=torch.float64)
    lo.RoundedLinear.apply(X, W, b, True).backward(dY)
    Xr, Wr, dYr = lo.round_bf16(X.detach()), lo.round_bf16(W.detach()), lo.round_bf16(dY)
    assert torch.equal(X.grad, dYr @ Wr) and torch.equal(W.grad, dYr.T @ Xr) and torch.equal(b.grad, dY.sum(0))


# ------------------------------------------------------------------------------------------------------ the Python surface
def test_train_backbone_precision(smplx_data, mean_params):
    from multi_hmr_amd import Model
    m = Model(backbone="dinov2_vits14", img_size=224, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=3)
    assert m._backbone_precision == "f32"
    assert m.train_backbone_(1) is m and m._backbone_precision == "f32"
    assert m.train_backbone_(2, precision="bf16") is m and m._backbone_precision == "bf16" and m._backbone_n == 2
    m.train_backbone_(1)                                       # None keeps the setting
    assert m._backbone_precision == "bf16" and m._backbone_n == 1
    with pytest.raises(ValueError):
        m.train_backbone_(1, precision="fp8")
    assert m._backbone_precision == "bf16" and m._backbone_n == 1      # a refused call changes nothing
    m.train_backbone_(1, precision="f32")
    assert m._backbone_precision == "f32"


def test_command_line_accepts_the_backbone_switches():
    from multi_hmr_amd import train
    p = train.build_parser()
    a = p.parse_args(["--pretrained", "x"])
    assert a.train_backbone == 0 and a.amp == 1
    a = p.parse_args(["--pretrained", "x", "--train_backbone", "2", "--amp", "0"])
    assert a.train_backbone == 2 and a.amp == 0
    with pytest.raises(SystemExit):
        p.parse_args(["--pretrained", "x", "--amp", "2"])
    assert "not trained here" not in p.format_help()


def test_make_optimizer_follows_the_switches(smplx_data, mean_params):
    from multi_hmr_amd import Model, train
    from multi_hmr_amd import backbone_train as bt
    new = lambda: Model(backbone="dinov2_vits14", img_size=224, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=3).train_heads_(True)
    p = train.build_parser()
    for argv, n, prec, embed in ((["--train_backbone", "2", "--amp", "0"], 2, "f32", False), (["--train_backbone", "3"], 3, "bf16", True)):
        m = new().train_detection_(True)
        opt = train.make_optimizer(m, p.parse_args(["--pretrained", "x"] + argv))
        assert isinstance(opt, torch.optim.Adam) and m._backbone_n == n and m._backbone_precision == prec
        named = dict(m.named_parameters())
        want = set(bt.backbone_parameter_names(3, n)) | (set(bt.embedding_parameter_names()) if embed else set())
        in_opt = {id(q) for g in opt.param_groups for q in g["params"]}
        assert all(id(named[k]) in in_opt and named[k].requires_grad for k in want)
        assert all(id(q) in in_opt for q in m.heads_parameters() + m.detection_parameters())
        assert any(q.requires_grad for q in m.embedding_parameters()) == embed
        assert len(in_opt) == len(want) + len(m.heads_parameters()) + len(m.detection_parameters())
