"""-m gpu: the backward of the last backbone blocks (csrc/vit_bwd.hip, csrc/attention_f32.hip, multi_hmr_amd/backbone_train.py) -- the
attention backward against the fp64 closed form, the block backward against fp64 autograd of oracle/dinov2_ref's own Block.

Measure and gate (tests/backbone_bwd_oracle.py): per tensor the relative L2 error against fp64 and the maximum error relative to the
tensor's largest fp64 magnitude; the yardstick is fp32 CPU torch autograd of the same oracle module, and the kernels may be at most 4x
worse in either measure.  Every test prints both columns before it asserts."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import backbone_bwd_oracle as bo  # noqa: E402
from multi_hmr_amd import _lib, backbone_train as bt  # noqa: E402

SENT = 7.25                       # sentinel behind every output
TAIL = 64                         # sentinel elements


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def rn(g, *shape, std=1.0):
    return torch.empty(*shape).normal_(0, 1, generator=g) * std


def guarded(*shape):
    """An fp32 device buffer of `shape` with TAIL sentinel elements behind it -> (flat buffer, the view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + TAIL,), SENT, dtype=torch.float32, device=dev())
    return buf, buf[:n].view(*shape)


def intact(*bufs):
    return all(bool((b[-TAIL:] == SENT).all()) for b in bufs)


# ------------------------------------------------------------------------------------------------------ (1) attention backward
ATT_B, ATT_H = 2, 2
ATT_CASES = [(T, bo.roundup(T, 64)) for T in (2, 16, 17, 33, 64, 65, 129, 257)] + [(65, bo.roundup(65, 64) + 64)]


@functools.lru_cache(maxsize=None)
def _attention_case(T, Tp):
    """CPU operands (padding rows hold finite values of their own) and the references, computed once and left unchanged."""
    B, H, Cd = ATT_B, ATT_H, 64 * ATT_H
    g = torch.Generator().manual_seed(5000 + 7 * T + Tp)
    qkv = rn(g, B * Tp, 3 * Cd)
    qkv[:, :Cd] *= 2.0                                         # logits of standard deviation ~2: the softmax is not flat
    dO = rn(g, B * Tp, Cd)
    r64 = bo.attention_backward_closed_form(qkv, dO, B, T, Tp, H, torch.float64)
    y32 = bo.attention_backward_autograd(qkv, dO, B, T, Tp, H, torch.float32)
    o64, lse64 = bo.attention_forward(qkv, B, T, Tp, H, torch.float64)
    o32, _ = bo.attention_forward(qkv, B, T, Tp, H, torch.float32)
    return dict(qkv=qkv, dO=dO, r64=r64, y32=y32, o64=o64, o32=o32, lse64=lse64)


def _attention_run(L, qkv, dO, B, T, Tp, H, refill=None):
    """tape + backward into sentinel-guarded buffers -> (out32, lse, dqkv) views and the flat buffers.  ``refill``: a generator seed; the
    rows >= T of qkv, dO and out32 are overwritten with other finite values before the backward runs."""
    Cd = 64 * H
    qkv, dO = qkv.to(dev()).contiguous(), dO.to(dev()).contiguous()
    ob, out32 = guarded(B * Tp, Cd)
    lb, lse = guarded(B, H, Tp)
    gb, dqkv = guarded(B * Tp, 3 * Cd)
    nbytes = int(L.mhmr_attention_f32_backward_workspace_bytes(B, Tp, H))
    assert nbytes >= B * H * Tp * 4
    wb = torch.full((nbytes // 4 + TAIL,), SENT, dtype=torch.float32, device=dev())
    _lib.check(L.mhmr_attention_f32_tape(qkv.data_ptr(), out32.data_ptr(), lse.data_ptr(), B, T, Tp, Cd, H, stream()), "tape")
    tape_out = out32.clone()
    if refill is not None:
        g = torch.Generator().manual_seed(refill)
        pad = (torch.arange(B * Tp) % Tp >= T).to(dev())
        qkv, dO = qkv.clone(), dO.clone()
        qkv[pad] = (rn(g, B * Tp, 3 * Cd) * 3.0 + 1.0).to(dev())[pad]
        dO[pad] = (rn(g, B * Tp, Cd) * 5.0 - 2.0).to(dev())[pad]
        out32[pad] = (rn(g, B * Tp, Cd) * 4.0).to(dev())[pad]
    _lib.check(L.mhmr_attention_f32_backward(qkv.data_ptr(), out32.data_ptr(), lse.data_ptr(), dO.data_ptr(), Cd, dqkv.data_ptr(), B, T, Tp, Cd, H,
                                             wb.data_ptr(), nbytes, stream()), "backward")
    torch.cuda.synchronize()
    assert intact(ob, lb, gb, wb), "a write behind an output"
    return tape_out, lse, dqkv


@pytest.mark.parametrize("T,Tp", ATT_CASES)
def test_attention_backward_against_the_fp64_closed_form(L, T, Tp):
    B, H, Cd = ATT_B, ATT_H, 64 * ATT_H
    c = _attention_case(T, Tp)
    out32, lse, dqkv = _attention_run(L, c["qkv"], c["dO"], B, T, Tp, H)
    real = (torch.arange(B * Tp) % Tp < T)
    # the tape: values, the log-sum, zeros in the padding rows
    o, l = out32.cpu(), lse.cpu()
    assert bool((o[~real] == 0).all()) and bool((l.reshape(B, H, Tp)[:, :, T:] == 0).all())
    # (lse: logits of |value| < 32 here, where fp32 numbers are 3.8e-6 apart, and a handful of roundings: 1e-5 absolute)
    lmx = float((l.double() - c["lse64"]).abs().max())
    print(f"[attention T {T} Tp {Tp}] tape: lse max abs error {lmx:.3e}, largest |lse| {float(c['lse64'].abs().max()):.2f}")
    assert float(c["lse64"].abs().max()) < 32 and lmx < 1e-5
    bo.gate(f"attention T {T} Tp {Tp}", [("tape out32", o, c["o32"], c["o64"])])
    # the backward: padding rows are exact zeros, then the gate per third and on the whole tensor
    d = dqkv.cpu()
    assert bool(torch.isfinite(d).all()) and bool((d[~real] == 0).all()), "rows >= T of dqkv are not exact zeros"
    rows = [("dqkv", d, c["y32"], c["r64"])]
    rows += [(n, d[:, i * Cd:(i + 1) * Cd], c["y32"][:, i * Cd:(i + 1) * Cd], c["r64"][:, i * Cd:(i + 1) * Cd]) for i, n in enumerate(("dQ", "dK", "dV"))]
    # two calls give equal bits
    _, _, again = _attention_run(L, c["qkv"], c["dO"], B, T, Tp, H)
    assert torch.equal(again, dqkv), "two calls differ"
    # image 0 alone gives image 0's bits
    _, _, one = _attention_run(L, c["qkv"][:Tp], c["dO"][:Tp], 1, T, Tp, H)
    assert torch.equal(one, dqkv[:Tp]), "image 0 of B = 2 differs from B = 1"
    # other finite values in the rows >= T of qkv, dO and out32 move no bit
    if Tp > T:
        _, _, other = _attention_run(L, c["qkv"], c["dO"], B, T, Tp, H, refill=77 + T)
        assert torch.equal(other, dqkv), "the padding rows reached a real row"
    bo.gate(f"attention T {T} Tp {Tp}", rows)


@pytest.mark.parametrize("name,dt,tdt", [("f16", _lib.DT_F16, torch.float16), ("bf16", _lib.DT_BF16, torch.bfloat16)])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 64, 65, 130])
def test_the_tape_is_the_forward_with_an_fp32_output(L, T, name, dt, tdt):
    """csrc/attention_f32.hip: mhmr_attention_f32 and mhmr_attention_f32_tape run one key-tile step, so on every real row the forward's
    [hi | lo] pair is, bit for bit, the split of the tape's fp32 out32 (conversions round to nearest even, as torch's do).  Rows >= T are
    not compared: the forward leaves finite values in the rest of T's 16-row group, the tape writes zeros."""
    B, H, Cd, Tp = 2, 2, 128, bo.roundup(T, 64)
    g = torch.Generator().manual_seed(6100 + T)
    qkv = rn(g, B * Tp, 3 * Cd)                                # the padding rows hold finite values of their own
    qkv[:, :Cd] *= 2.0
    qkv = qkv.to(dev())
    pair = torch.full((B * Tp, 2 * Cd), float("nan"), dtype=tdt, device=dev())
    ob, out32 = guarded(B * Tp, Cd)
    lb, lse = guarded(B, H, Tp)
    _lib.check(L.mhmr_attention_f32(qkv.data_ptr(), pair.data_ptr(), B, T, Tp, Cd, H, dt, stream()), "attention_f32")
    _lib.check(L.mhmr_attention_f32_tape(qkv.data_ptr(), out32.data_ptr(), lse.data_ptr(), B, T, Tp, Cd, H, stream()), "tape")
    torch.cuda.synchronize()
    assert intact(ob, lb), "a write behind an output"
    real = torch.arange(B * Tp) % Tp < T
    o, p = out32.cpu()[real], pair.cpu()[real]
    hi, lo = p[:, :Cd], p[:, Cd:]
    want_hi = o.to(tdt)
    want_lo = (o - want_hi.float()).to(tdt)
    nh, nl = int((hi.view(torch.int16) != want_hi.view(torch.int16)).sum()), int((lo.view(torch.int16) != want_lo.view(torch.int16)).sum())
    print(f"[tape == forward, T {T} {name}] {o.numel()} elements: hi differs in {nh}, lo differs in {nl}")
    assert bool(torch.isfinite(o).all()) and nh == 0 and nl == 0


# ------------------------------------------------------------------------------------------------------ (2) block backward
BLK_B, BLK_C, BLK_H = 2, 384, 6


@functools.lru_cache(maxsize=None)
def _block_case(T, Tp):
    B, Cd, H = BLK_B, BLK_C, BLK_H
    g = torch.Generator().manual_seed(6000 + T)
    blk = bo.make_block(Cd, H, seed=60 + T)
    x_in, g_out = rn(g, B * Tp, Cd), rn(g, B * Tp, Cd)      # padding rows: finite values that must not matter
    r64 = bo.block_backward(blk, x_in, g_out, B, T, Tp, torch.float64)
    y32 = bo.block_backward(blk, x_in, g_out, B, T, Tp, torch.float32)
    g_nocls = g_out.clone().reshape(B, Tp, Cd)
    g_nocls[:, T - 1] = 0                                    # the class token is the last real row
    n64 = bo.block_backward(blk, x_in, g_nocls.reshape(B * Tp, Cd), B, T, Tp, torch.float64)
    return dict(blk=blk, x_in=x_in, g_out=g_out, r64=r64, y32=y32, n64=n64)


@pytest.mark.parametrize("T,Tp", [(17, 64), (257, 320)])
def test_block_backward_against_fp64_autograd(L, T, Tp):
    B, Cd, H = BLK_B, BLK_C, BLK_H
    c = _block_case(T, Tp)
    params = {k: v.detach().float().to(dev()).contiguous() for k, v in bo.block_params(c["blk"]).items()}
    g_in, grads = bt.block_backward(params, c["x_in"].to(dev()), c["g_out"].to(dev()), B, T, Tp, H)
    torch.cuda.synchronize()
    got = dict(grads, g_in=g_in)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    real = (torch.arange(B * Tp) % Tp < T)
    assert bool((g_in.cpu()[~real] == 0).all()), "padding rows of g_in are not zeros"
    # qkv_b as ONE tensor: its K third is zero in exact arithmetic
    assert float(c["r64"]["qkv_b"][Cd:2 * Cd].abs().max()) < 1e-12 * float(c["r64"]["qkv_b"].abs().max())
    # the class row's cotangent is part of the result: the oracle without it differs, and the kernels follow the full one
    for name in ("g_in", "qkv_w", "fc1_w"):
        full, without = bo.measure(got[name], c["r64"][name])[0], bo.measure(got[name], c["n64"][name])[0]
        print(f"[block T {T}] {name}: rel L2 to the oracle {full:.3e}, to the oracle without the class row's cotangent {without:.3e}")
        assert without > 1e-3 and without > 100 * full
    # two calls give equal bits; other finite values in the padding rows of x_in and g_out move no bit
    g2, grads2 = bt.block_backward(params, c["x_in"].to(dev()), c["g_out"].to(dev()), B, T, Tp, H)
    assert torch.equal(g2, g_in) and all(torch.equal(grads2[k], grads[k]) for k in grads), "two calls differ"
    gsw = c["g_out"].clone()
    gsw[~real] = 3.0
    g3, grads3 = bt.block_backward(params, c["x_in"].to(dev()), gsw.to(dev()), B, T, Tp, H)
    assert torch.equal(g3, g_in) and all(torch.equal(grads3[k], grads[k]) for k in grads), "g_out's padding rows were read as cotangents"
    bo.gate(f"block T {T} Tp {Tp}", [(n, got[n], c["y32"][n], c["r64"][n]) for n in ("g_in",) + bo.PARAMS])


# ------------------------------------------------------------------------------------------------------ (3) + (4): the tap and the tail
import ctypes as C  # noqa: E402

import vit_forms as vf  # noqa: E402


def _case_setup(monkeypatch, name):
    for k, v in vf.case_env(name).items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    P = vf.pack_case(name)
    B = vf.case_batch(name, vf.cu_count())
    return P, B, vf.make_images(B)


def _run_tapped(name, P, B, x, cache, tap_first):
    """vit_forms.run_form with a tap on the copied description: -> (feat32, ctx16, resid, bits, tap [L - tap_first, B, Tp, C])."""
    lib, c = _lib.lib(), vf.CASES[name]
    Pw = vf._ALL_ROWS_PACKS.setdefault(id(P), (P, dict(P, fold=True)))[1] if c.get("tp_all_rows") else P
    ws = cache.get(Pw, B, vf._extra)
    d = _lib.VitDesc.from_buffer_copy(ws["vit_desc"])
    for n in c.get("null", ()):
        setattr(d, n, None)
        for m in vf.NULLABLE[n]:
            setattr(d, m, 0)
    Tp, Cd, L_ = ws["Tp"], P["C"], P["L"]
    tb = torch.full(((L_ - tap_first) * B * Tp * Cd + TAIL,), SENT, dtype=torch.float32, device=dev())
    d.tap, d.tap_first = tb.data_ptr(), tap_first
    x = x.to(dev()).contiguous()
    bits = C.c_uint(0)
    _lib.check(lib.mhmr_vit_form_bits(C.byref(d), stream(), C.byref(bits)), "mhmr_vit_form_bits")
    ws["ctx16"].fill_(vf.SENTINEL)
    _lib.check(lib.mhmr_vit_forward(C.byref(d), x.data_ptr(), ws["feat32"].data_ptr(), ws["ctx16"].data_ptr(), Cd + 64, stream()), "mhmr_vit_forward")
    torch.cuda.synchronize()
    assert intact(tb), "a write behind the tap"
    return dict(feat32=ws["feat32"].view(B, P["N"], Cd).clone(), ctx16=ws["ctx16"].clone(), resid=ws["resid"].view(B, Tp, Cd).clone(),
                bits=vf.bit_names(bits.value), tap=tb[:-TAIL].view(L_ - tap_first, B, Tp, Cd).clone(), Tp=Tp)


@pytest.mark.parametrize("name", ["plain128", "rowmap_fold_cst"])
def test_tap_holds_every_block_input_and_changes_nothing(L, monkeypatch, name):
    """Tap slot l - tap_first == resid after a forward of depth l, bit for bit (all rows); feat32, ctx16 and the form bits with and without
    a tap are identical; after the call `resid` is the stream the final norm read; a bad tap_first is refused before any launch."""
    P, B, x = _case_setup(monkeypatch, name)
    cache = vf.vit.WorkspaceCache()
    base = vf.run_case(name, P, B, x, cache)
    vf.check_want(base["bits"], vf.CASES[name]["want"], name)
    shallow = {l: vf.run_case(name, P, B, x, cache, L=l)["resid"] for l in range(vf.DEPTH)}
    for tap_first in (0, 1):
        t = _run_tapped(name, P, B, x, cache, tap_first)
        assert t["bits"] == base["bits"] and torch.equal(t["feat32"], base["feat32"]) and torch.equal(t["ctx16"], base["ctx16"])
        assert torch.equal(t["resid"], base["resid"])
        for l in range(tap_first, vf.DEPTH):
            assert torch.equal(t["tap"][l - tap_first], shallow[l]), (name, tap_first, l)
    # the description is checked before the first launch
    ws = cache.get(P, B, vf._extra)
    d = _lib.VitDesc.from_buffer_copy(ws["vit_desc"])
    d.tap = ws["resid"].data_ptr()
    for bad in (-1, vf.DEPTH + 1):
        d.tap_first = bad
        assert L.mhmr_vit_forward(C.byref(d), x.to(dev()).data_ptr(), ws["feat32"].data_ptr(), ws["ctx16"].data_ptr(), P["C"] + 64, stream()) == -1


def _tail_oracle(enc, tap, resid, g_feat, B, N, Tp, dtype):
    """The contract of the tail in torch autograd: the final norm at `resid`, then every block at ITS OWN tapped input (the 16-bit roundings
    of the forward between two blocks are straight-through), last block first.  -> dict of gradients, fp of `dtype`."""
    import copy
    T, Cd, n = N + 1, resid.shape[-1], tap.shape[0]
    depth = len(enc.blocks)
    norm = copy.deepcopy(enc.norm).to(dtype).requires_grad_(True)
    xr = resid.to(dtype).reshape(B, Tp, Cd)[:, :T].clone().requires_grad_()
    (norm(xr)[:, :N] * g_feat.to(dtype).reshape(B, N, Cd)).sum().backward()
    out = {"norm_w": norm.weight.grad.clone(), "norm_b": norm.bias.grad.clone()}
    g = torch.zeros(B, Tp, Cd, dtype=dtype)
    g[:, :T] = xr.grad
    for i in range(n - 1, -1, -1):
        blk = copy.deepcopy(enc.blocks[depth - n + i]).requires_grad_(True)
        r = bo.block_backward(blk, tap[i].reshape(B * Tp, Cd), g.reshape(B * Tp, Cd), B, T, Tp, dtype)
        for k in bo.PARAMS:
            out[f"block{depth - n + i}.{k}"] = r[k]
        g = r["g_in"].reshape(B, Tp, Cd)
    out["g_stream"] = g.reshape(B * Tp, Cd)
    return out


def test_tail_backward_against_fp64_autograd(L, monkeypatch):
    """Final norm + the last 2 blocks of the depth-3 encoder of tests/vit_forms.py (plain128) on the tapped streams of its forward."""
    name, n = "plain128", 2
    P, B, x = _case_setup(monkeypatch, name)
    t = _run_tapped(name, P, B, x, vf.vit.WorkspaceCache(), vf.DEPTH - n)
    enc = vf.make_encoder(vf.CASES[name]["backbone"])
    N, Cd, H, Tp = P["N"], P["C"], P["H"], t["Tp"]
    g_feat = rn(torch.Generator().manual_seed(31), B * N, Cd)
    tap, resid = t["tap"].reshape(n, B * Tp, Cd).contiguous(), t["resid"].reshape(B * Tp, Cd).contiguous()
    blocks = [bt.block_tensors(enc.blocks[vf.DEPTH - n + i], dev()) for i in range(n)]
    f32 = lambda p: p.detach().float().to(dev()).contiguous()
    g_stream, gw, gb, grads = bt.tail_backward(f32(enc.norm.weight), f32(enc.norm.bias), blocks, tap, resid, g_feat.to(dev()), B, N, Tp, H)
    torch.cuda.synchronize()
    got = {"norm_w": gw, "norm_b": gb, "g_stream": g_stream}
    for i in range(n):
        got.update({f"block{vf.DEPTH - n + i}.{k}": v for k, v in grads[i].items()})
    r64 = _tail_oracle(enc, tap.cpu(), resid.cpu(), g_feat, B, N, Tp, torch.float64)
    y32 = _tail_oracle(enc, tap.cpu(), resid.cpu(), g_feat, B, N, Tp, torch.float32)
    assert set(got) == set(r64)
    pad = torch.arange(B * Tp) % Tp >= N + 1
    assert bool((g_stream.cpu()[pad] == 0).all())
    # the class row receives nothing from the final norm, but the attention of the last block hands it a cotangent
    cls = torch.arange(B * Tp) % Tp == N
    assert bool((g_stream.cpu()[cls] != 0).any())
    g2 = bt.tail_backward(f32(enc.norm.weight), f32(enc.norm.bias), blocks, tap, resid, g_feat.to(dev()), B, N, Tp, H)
    assert torch.equal(g2[0], g_stream) and all(torch.equal(g2[3][i][k], grads[i][k]) for i in range(n) for k in bo.PARAMS), "two calls differ"
    bo.gate("tail", [(k, got[k], y32[k], r64[k]) for k in sorted(got)])


# ------------------------------------------------------------------------------------------------------ (5) + (6): the model
def _training_scene():
    import gt_oracle as go
    import loss_oracle as lo
    import test_gpu_feature_grad as tf
    from multi_hmr_amd import BodyModel, GroundTruth, Loss
    a = tf._assets()
    builder = GroundTruth(tf.S, patch_size=14, smplx_neutral=BodyModel(a["data"], "smplx", num_betas=11))
    y = go.make_y("smplx", 51, tf.S, [2, 1], depth=2.6)
    gt = builder.prepare({k: (v.to(dev()) if isinstance(v, torch.Tensor) else v) for k, v in y.items()})
    x = torch.randn(2, 3, tf.S, tf.S, generator=torch.Generator().manual_seed(0)).to(dev())
    loss, epoch = Loss(lo.default_args()), lo.DEFAULTS["start_2d_epoch"]
    kw = dict(idx=gt["idx"], K=gt["K"], is_training=True, return_readout=True)

    def total(m, out):
        d = m.decode_readout(out["readout"], out["offset"], gt["idx"], gt["K"])
        return loss(dict(d, scores=out["scores"]), gt, epoch=epoch, img_size=tf.S)[0]
    return tf, x, y, builder, kw, total


def test_model_train_backbone():
    tf, x, y, builder, kw, total = _training_scene()
    m = tf._new_model().train_backbone_(2)
    names = bt.backbone_parameter_names(4, 2)
    named = dict(m.named_parameters())
    assert {k for k, p in named.items() if p.requires_grad} == set(names)
    plain = m(x, **kw)
    out = m(x, train_backbone=True, **kw)
    tf._same(plain, out)
    assert out["scores"].requires_grad and out["readout"].requires_grad and out["offset"].requires_grad
    total(m, out).backward()
    grads = {k: named[k].grad.clone() for k in names}
    for k, g in grads.items():
        assert g.shape == named[k].shape and bool(torch.isfinite(g).all()) and bool((g != 0).any()), k
    assert all(p.grad is None for k, p in named.items() if k not in names)
    # the same gradients from the feature cotangent of the leaf route, handed to mhmr_vit_tail_backward on the tapped workspace
    ws = m._workspace(m._packed, 2, tap=2)
    f = m.backbone_features(x).clone().requires_grad_()
    total(m, m.forward_features(f, **kw)).backward()
    assert f.grad is not None and bool((f.grad != 0).any())
    direct = bt.model_tail_backward(m, m._packed, ws, 2, f.grad, 2)
    for k in names:
        assert torch.equal(direct[k].view_as(grads[k]), grads[k]), k
    # composition with the other switches: the same values, the head and detector gradients of a run without the backbone
    m2 = tf._new_model().train_backbone_(1).train_heads_(True).train_detection_(True)
    o2 = m2(x, train_backbone=True, train_heads=True, train_detection=True, **kw)
    tf._same(plain, o2)
    total(m2, o2).backward()
    n2 = dict(m2.named_parameters())
    trained = set(bt.backbone_parameter_names(4, 1)) | {k for k, p in n2.items() if p.requires_grad}
    assert all((p.grad is not None) == (k in trained) for k, p in n2.items())
    assert all(torch.equal(n2[k].grad, grads[k]) for k in bt.backbone_parameter_names(4, 1))      # the last block does not depend on n
    # the backbone tail alone
    tf._clear(m)
    fa = m.backbone_features(x, train_backbone=True)
    assert fa.requires_grad and fa.data_ptr() != m._workspace(m._packed, 2, tap=2)["feat32"].data_ptr()
    assert torch.equal(fa.detach(), m.backbone_features(x))
    fa = m.backbone_features(x, train_backbone=True)
    fa.backward(f.grad)
    assert all(torch.equal(named[k].grad, grads[k]) for k in names)
    # a backward after another forward of the same batch size raises
    out = m(x, train_backbone=True, **kw)
    m(x, train_backbone=True, **kw)
    with pytest.raises(_lib.MhmrError, match="before the next forward"):
        total(m, out).backward()
    with pytest.raises(ValueError):
        m(x, K=kw["K"], train_backbone=True)


def test_repack_backbone_and_a_trainer_step(tmp_path):
    import loss_oracle as lo
    from multi_hmr_amd import Loss, Trainer
    tf, x, y, builder, kw, total = _training_scene()
    m = tf._new_model().train_backbone_(1)
    total(m, m(x, train_backbone=True, **kw)).backward()
    before = [p.detach().clone() for p in m.backbone_parameters(1)]
    torch.optim.SGD(m.backbone_parameters(1), lr=0.05).step()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, m.backbone_parameters(1)))
    stale = m(x, **kw)
    m.repack_backbone()
    fresh = m(x, **kw)
    assert not torch.equal(stale["readout"], fresh["readout"]), "the step did not reach the packed weights"
    m.repack()
    tf._same(m(x, **kw), fresh)
    # a Trainer over heads + backbone with a torch optimiser
    m = tf._new_model().train_heads_(True).train_backbone_(1)
    ns = lo.default_args(save_dir=str(tmp_path), name="run", nb_max_ckpt=2, max_epochs=1, log_freq=1, det_thresh=0.3, nms_kernel_size=3)
    opt = torch.optim.AdamW(m.heads_parameters() + m.backbone_parameters(1), lr=1e-4)
    tr = Trainer(m, Loss(ns), opt, ns, builder)
    tr.current_epoch = lo.DEFAULTS["start_2d_epoch"]
    w0 = m.backbone_parameters(1)[3].detach().clone()
    d = tr.train_step(x, y)
    assert all(bool(torch.isfinite(v).all()) for v in d.values()) and not torch.equal(w0, m.backbone_parameters(1)[3].detach())
    o = m(x, **kw)
    assert all(bool(torch.isfinite(v).all()) for v in o.values())
    with pytest.raises(ValueError):
        tr.train_step_features(m.backbone_features(x).clone(), y)
