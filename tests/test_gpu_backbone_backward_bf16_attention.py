"""-m gpu: the block and tail backward and the model with bf16-operand attention (attention_precision = MHMR_ATTN_BF16 of the `_a` entries;
csrc/attention_bf16.hip, csrc/vit_bwd.hip) at the shapes of tests/test_gpu_backbone_backward_bf16.py.

Reference: tests/attention_bf16_oracle.py's restatement -- oracle/dinov2_ref's Block with rounded linears (section 30) and the rounded
attention of section 31 -- in fp64.  Yardstick: the same restatement in fp32 on the CPU.  Gate: the project's factor 4 in both measures,
per tensor.  Each test also prints, without gating, every tensor's distance to the UNROUNDED fp64 oracle: the cost of the mode."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_bf16_oracle as ao  # noqa: E402
import backbone_bwd_oracle as bo  # noqa: E402
import test_gpu_backbone_backward as tb  # noqa: E402
import test_gpu_backbone_backward_bf16 as tbf  # noqa: E402
import vit_forms as vf  # noqa: E402
from multi_hmr_amd import _lib, backbone_train as bt  # noqa: E402

SENT, TAIL = 7.25, 64
BLK_B, BLK_C, BLK_H = 2, 384, 6


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def dev():
    return torch.device("cuda:0")


def raw_block_a(L, params, x_in, g_out, B, T, Tp, H, precision, attention, nbytes=None):
    """mhmr_vit_block_backward_a through a descriptor filled here, every output and the workspace followed by sentinels
    -> (g_in, {field: gradient})."""
    Cd = x_in.shape[1]
    x_in, g_out = x_in.to(dev()).contiguous(), g_out.to(dev()).contiguous()
    bufs = {f: torch.full((params[f].numel() + TAIL,), SENT, dtype=torch.float32, device=dev()) for f in _lib.VitBlockBackwardDesc.PARAMS}
    grads = {f: bufs[f][:params[f].numel()].view(params[f].shape) for f in bufs}
    gb = torch.full((B * Tp * Cd + TAIL,), SENT, dtype=torch.float32, device=dev())
    if nbytes is None:
        nbytes = int(L.mhmr_vit_block_backward_workspace_bytes_pa(B, Tp, Cd, precision, attention))
    wb = torch.full((nbytes // 4 + TAIL,), SENT, dtype=torch.float32, device=dev())
    d = bt.fill_block_desc(_lib.VitBlockBackwardDesc(), params, grads, B, T, Tp, Cd, H)
    d.x_in, d.g_out, d.g_in, d.workspace, d.workspace_bytes = x_in.data_ptr(), g_out.data_ptr(), gb.data_ptr(), wb.data_ptr(), nbytes
    d.linear_precision = precision
    _lib.check(L.mhmr_vit_block_backward_a(C.byref(d), attention, torch.cuda.current_stream().cuda_stream), "mhmr_vit_block_backward_a")
    torch.cuda.synchronize()
    assert all(bool((b[-TAIL:] == SENT).all()) for b in list(bufs.values()) + [gb, wb]), "a write behind an output or the workspace"
    return gb[:-TAIL].view(B * Tp, Cd).clone(), {f: g.clone() for f, g in grads.items()}


@functools.lru_cache(maxsize=None)
def _block_case(T, Tp):
    B, Cd, H = BLK_B, BLK_C, BLK_H
    g = torch.Generator().manual_seed(6200 + T)
    blk = bo.make_block(Cd, H, seed=62 + T)
    x_in, g_out = tb.rn(g, B * Tp, Cd), tb.rn(g, B * Tp, Cd)      # padding rows: finite values that must not matter
    return dict(blk=blk, x_in=x_in, g_out=g_out,
                r64=ao.rounded_block_backward(blk, x_in, g_out, B, T, Tp, torch.float64),
                y32=ao.rounded_block_backward(blk, x_in, g_out, B, T, Tp, torch.float32),
                u64=bo.block_backward(blk, x_in, g_out, B, T, Tp, torch.float64))


_equal = tbf._equal


@pytest.mark.parametrize("T,Tp", [(17, 64), (257, 320)])
def test_block_backward_bf16_attention_against_the_rounding_restatement(L, T, Tp):
    B, Cd, H = BLK_B, BLK_C, BLK_H
    c = _block_case(T, Tp)
    params = {k: v.detach().float().to(dev()).contiguous() for k, v in bo.block_params(c["blk"]).items()}
    x, go = c["x_in"], c["g_out"]
    res = raw_block_a(L, params, x, go, B, T, Tp, H, 1, 1)
    g_in, grads = res
    got = dict(grads, g_in=g_in)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    real = torch.arange(B * Tp) % Tp < T
    assert bool((g_in.cpu()[~real] == 0).all()), "rows >= T of g_in are not exact zeros"
    # two calls; the wrapper
    assert _equal(raw_block_a(L, params, x, go, B, T, Tp, H, 1, 1), res), "two calls differ"
    assert _equal(bt.block_backward(params, x.to(dev()), go.to(dev()), B, T, Tp, H, precision="bf16", attention="bf16"), res), "the wrapper differs"
    # image 0 of B = 2 is B = 1 (g_in)
    one, _ = raw_block_a(L, params, x[:Tp], go[:Tp], 1, T, Tp, H, 1, 1)
    assert torch.equal(one, g_in[:Tp]), "image 0 of B = 2 differs from B = 1"
    # other finite values in the rows >= T of x_in and g_out move no bit of anything
    g = torch.Generator().manual_seed(T)
    xs, gs = x.clone(), go.clone()
    xs[~real] = (tb.rn(g, B * Tp, Cd) * 3.0 + 1.0)[~real]
    gs[~real] = (tb.rn(g, B * Tp, Cd) * 5.0 - 2.0)[~real]
    assert _equal(raw_block_a(L, params, xs, gs, B, T, Tp, H, 1, 1), res), "the padding rows reached a real row or a parameter gradient"
    # attention_precision 0: the old entry's bits at the old workspace size, for both linear precisions; the wrapper's default is that mode
    for p, name in ((0, "f32"), (1, "bf16")):
        old_bytes = int(L.mhmr_vit_block_backward_workspace_bytes_p(B, Tp, Cd, p))
        old = tbf.raw_block(L, params, x, go, B, T, Tp, H, p, nbytes=old_bytes)
        assert _equal(raw_block_a(L, params, x, go, B, T, Tp, H, p, 0, nbytes=old_bytes), old), f"_a(d, 0) is not the old entry (linear_precision {p})"
        assert _equal(bt.block_backward(params, x.to(dev()), go.to(dev()), B, T, Tp, H, precision=name), old)
        assert _equal(bt.block_backward(params, x.to(dev()), go.to(dev()), B, T, Tp, H, precision=name, attention="f32"), old)
        # the attention switch changes what passes through the attention, in either linear precision
        new = raw_block_a(L, params, x, go, B, T, Tp, H, p, 1)
        assert not torch.equal(old[0], new[0]) and not torch.equal(old[1]["qkv_w"], new[1]["qkv_w"]), p
    names = ("g_in",) + bo.PARAMS
    tbf.cost_of_the_mode(f"block bf16+attention T {T} Tp {Tp}", names, got, c["r64"], c["u64"])
    bo.gate(f"block bf16+attention T {T} Tp {Tp}", [(n, got[n], c["y32"][n], c["r64"][n]) for n in names])


def test_tail_backward_bf16_attention_against_the_rounding_restatement(L, monkeypatch):
    """Final norm + the last 2 blocks of the depth-3 ViT-S of tests/vit_forms.py (plain128; T = 257, Tp = 384, B = 2) at its tapped streams."""
    name, n = "plain128", 2
    P, B, x = tb._case_setup(monkeypatch, name)
    t = tb._run_tapped(name, P, B, x, vf.vit.WorkspaceCache(), vf.DEPTH - n)
    enc = vf.make_encoder(vf.CASES[name]["backbone"])
    N, Cd, H, Tp = P["N"], P["C"], P["H"], t["Tp"]
    assert (N + 1, Tp, B) == (257, 384, 2)
    g_feat = tb.rn(torch.Generator().manual_seed(33), B * N, Cd)
    tap, resid = t["tap"].reshape(n, B * Tp, Cd).contiguous(), t["resid"].reshape(B * Tp, Cd).contiguous()
    blocks = [bt.block_tensors(enc.blocks[vf.DEPTH - n + i], dev()) for i in range(n)]
    f32 = lambda p: p.detach().float().to(dev()).contiguous()

    def run(**kw):
        g_stream, gw, gb, grads = bt.tail_backward(f32(enc.norm.weight), f32(enc.norm.bias), blocks, tap, resid, g_feat.to(dev()), B, N, Tp, H, **kw)
        torch.cuda.synchronize()
        out = {"norm_w": gw, "norm_b": gb, "g_stream": g_stream}
        for i in range(n):
            out.update({f"block{vf.DEPTH - n + i}.{k}": v for k, v in grads[i].items()})
        return out
    got = run(precision="bf16", attention="bf16")
    again, lin, lin0 = run(precision="bf16", attention="bf16"), run(precision="bf16"), run(precision="bf16", attention="f32")
    assert all(torch.equal(again[k], got[k]) for k in got), "two calls differ"
    assert all(torch.equal(lin0[k], lin[k]) for k in lin), "attention f32 through the _a entry is not the call without the keyword"
    assert all(torch.equal(run(attention="f32")[k], v) for k, v in run().items())
    assert torch.equal(lin["norm_w"], got["norm_w"]) and torch.equal(lin["norm_b"], got["norm_b"])      # the final norm does not depend on it
    last = f"block{vf.DEPTH - 1}."
    assert not torch.equal(lin["g_stream"], got["g_stream"]) and not torch.equal(lin[last + "qkv_w"], got[last + "qkv_w"])
    pad = torch.arange(B * Tp) % Tp >= N + 1
    assert bool((got["g_stream"].cpu()[pad] == 0).all()) and all(bool(torch.isfinite(v).all()) for v in got.values())
    enc_r = ao.rounded(enc)
    r64 = tb._tail_oracle(enc_r, tap.cpu(), resid.cpu(), g_feat, B, N, Tp, torch.float64)
    y32 = tb._tail_oracle(enc_r, tap.cpu(), resid.cpu(), g_feat, B, N, Tp, torch.float32)
    u64 = tb._tail_oracle(enc, tap.cpu(), resid.cpu(), g_feat, B, N, Tp, torch.float64)
    assert set(got) == set(r64)
    tbf.cost_of_the_mode("tail bf16+attention", sorted(got), got, r64, u64)
    bo.gate("tail bf16+attention", [(k, got[k], y32[k], r64[k]) for k in sorted(got)])


def test_model_trains_the_whole_encoder_with_bf16_attention(tmp_path):
    import loss_oracle as lso
    from multi_hmr_amd import Loss, Trainer
    tf, x, y, builder, kw, total = tb._training_scene()
    names = bt.backbone_parameter_names(3, 3)
    runs = {}
    for mode in (("bf16", "bf16"), ("bf16", "f32"), ("f32", "f32")):
        m = tbf._new_model3().train_backbone_(3, precision=mode[0], attention=mode[1]).train_embeddings_()
        assert (m._backbone_precision, m._backbone_attention) == mode
        plain = m(x, **kw)
        out = m(x, train_backbone=True, **kw)
        tf._same(plain, out)
        runs[mode] = out, m
        total(m, out).backward()
    (oa, ma), (ol, ml), (of, _) = runs[("bf16", "bf16")], runs[("bf16", "f32")], runs[("f32", "f32")]
    tf._same(oa, of)                                           # the forward depends on neither switch: the returned dict is the f32 mode's
    tf._same(oa, ol)
    na, nl = dict(ma.named_parameters()), dict(ml.named_parameters())
    every = names + bt.embedding_parameter_names()
    assert all(na[k].grad is not None and bool(torch.isfinite(na[k].grad).all()) and bool((na[k].grad != 0).any()) for k in every)
    assert all(not torch.equal(na[k].grad, nl[k].grad) for k in names if k.endswith(("qkv.weight", "norm1.weight"))), "the linears-only mode's gradients"
    # the block / norm gradients are tail_backward(precision="bf16", attention="bf16") fed with the feature cotangent of the leaf route
    ws = ma._workspace(ma._packed, 2, tap=3)
    f = ma.backbone_features(x).clone().requires_grad_()
    total(ma, ma.forward_features(f, **kw)).backward()
    enc, P = ma.backbone.encoder, ma._packed
    N, Cd, H = P["N"], P["C"], P["H"]
    blocks = [bt.block_tensors(enc.blocks[l], dev()) for l in range(3)]
    g_feat, flat = f.grad.reshape(2 * N, Cd), None
    for part in ws["parts"]:
        Bh, i0, bufs = part["B"], part["img0"], part["bufs"]
        _, gw, gb, gr = bt.tail_backward(enc.norm.weight.detach(), enc.norm.bias.detach(), blocks, bufs["tap"], bufs["resid"],
                                         g_feat[i0 * N:(i0 + Bh) * N], Bh, N, ws["Tp"], H, precision="bf16", attention="bf16")
        one = [gw, gb] + [g[k] for g in gr for k in _lib.VitBlockBackwardDesc.PARAMS]
        flat = one if flat is None else [a + b for a, b in zip(flat, one)]
    for k, g in zip(names, flat):
        assert torch.equal(g.view_as(na[k].grad), na[k].grad), k
    # a Trainer step with Adam over all of it; afterwards the packed weights are the parameters'
    m = tbf._new_model3().train_heads_(True).train_detection_(True).train_backbone_(3, precision="bf16", attention="bf16").train_embeddings_()
    ns = lso.default_args(save_dir=str(tmp_path), name="run", nb_max_ckpt=2, max_epochs=1, log_freq=1, det_thresh=0.3, nms_kernel_size=3)
    opt = torch.optim.Adam(m.heads_parameters() + m.detection_parameters() + m.backbone_parameters(3) + m.embedding_parameters(), lr=1e-4)
    tr = Trainer(m, Loss(ns), opt, ns, builder)
    tr.current_epoch = lso.DEFAULTS["start_2d_epoch"]
    w0 = m.backbone_parameters(3)[4].detach().clone()
    d = tr.train_step(x, y)
    assert all(bool(torch.isfinite(v).all()) for v in d.values()) and not torch.equal(w0, m.backbone_parameters(3)[4].detach())
    after = m(x, **kw)
    m.repack()
    tf._same(m(x, **kw), after)
