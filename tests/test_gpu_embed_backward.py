"""-m gpu: the backward of the token embedding (csrc/vit_embed_bwd.hip, multi_hmr_amd/backbone_train.py) against
fp64 autograd of the restated ``prepare_tokens`` (tests/embed_bwd_oracle.py), kernel by kernel and through ``Model``.

Measure and gate (tests/backbone_bwd_oracle.py, the standing rule of section 28): per tensor the relative L2 error against fp64 and the
maximum error relative to the tensor's largest fp64 magnitude; the yardstick is fp32 CPU torch autograd of the same restatement, and the
kernels may be at most 4x worse in either measure.  Every test prints both columns before it asserts."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import backbone_bwd_oracle as bo  # noqa: E402
import embed_bwd_oracle as eo  # noqa: E402
from multi_hmr_amd import _lib, backbone_train as bt, packing  # noqa: E402

SENT = 7.25                       # sentinel behind every output
TAIL = 64                         # sentinel elements
#: (C, G, M, B, Tp): what each shape reaches
CASES = [(128, 3, 5, 2, 64),      # 18 rows, a single chain, down-sampling with clipped taps
         (128, 4, 4, 1, 64),      # the identity table, B = 1
         (128, 16, 37, 2, 320),   # 512 rows: one flush of the first level
         (64, 37, 37, 4, 1408),   # 5 476 rows: the second level flushes
         (128, 9, 4, 2, 128)]     # up-sampling


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def rn(g, *shape):
    return torch.empty(*shape).normal_(0, 1, generator=g)


def guarded(*shape, dtype=torch.float32):
    """A device buffer of `shape` with TAIL sentinel elements behind it -> (flat buffer, the view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + TAIL,), SENT, dtype=dtype, device=dev())
    return buf, buf[:n].view(*shape)


def intact(*bufs):
    return all(bool((b[-TAIL:] == SENT).all()) for b in bufs)


@functools.lru_cache(maxsize=None)
def _case(Cd, G, M, B, Tp):
    """CPU operands (x = N(0, 1) + 0.5, g_stream = N(0, 1) in EVERY row, the padding included) and the two references, computed once and
    left unchanged."""
    g = torch.Generator().manual_seed(9000 + 131 * G + 7 * M + B + Cd)
    x = rn(g, B, 3, 14 * G, 14 * G) + 0.5
    gs = rn(g, B * Tp, Cd)
    params = eo.make_params(Cd, M, seed=G + M)
    return dict(x=x, gs=gs, r64=eo.embed_backward(x, params, gs, B, G, Tp, torch.float64), y32=eo.embed_backward(x, params, gs, B, G, Tp, torch.float32))


def _run(L, x, gs, Cd, G, M, B, Tp):
    """mhmr_vit_embed_backward into sentinel-guarded outputs and a sentinel-guarded workspace -> {name: tensor}."""
    x, gs = x.to(dev()).contiguous(), gs.to(dev()).contiguous()
    interp = torch.from_numpy(packing.pos_embed_matrix(M, G)).to(dev()).contiguous()
    shapes = dict(g_patch_w=(Cd, 588), g_patch_b=(Cd,), g_cls=(Cd,), g_pos=(1 + M * M, Cd))
    bufs = {k: guarded(*s) for k, s in shapes.items()}
    nbytes = int(L.mhmr_vit_embed_backward_workspace_bytes(B, G, M, Cd))
    assert nbytes > 0 and nbytes % 8 == 0
    wb = torch.full((nbytes // 8 + TAIL,), SENT, dtype=torch.float64, device=dev())
    d = _lib.VitEmbedBackwardDesc()
    d.B, d.S, d.G, d.M, d.Tp, d.C = B, 14 * G, G, M, Tp, Cd
    d.x, d.g_stream, d.interp, d.workspace, d.workspace_bytes = x.data_ptr(), gs.data_ptr(), interp.data_ptr(), wb.data_ptr(), nbytes
    for k, (_, view) in bufs.items():
        setattr(d, k, view.data_ptr())
    _lib.check(L.mhmr_vit_embed_backward(C.byref(d), stream()), "mhmr_vit_embed_backward")
    torch.cuda.synchronize()
    assert intact(wb, *[b for b, _ in bufs.values()]), "a write behind an output or behind the workspace"
    out = {k: view.clone() for k, (_, view) in bufs.items()}
    assert all(bool(torch.isfinite(t).all()) for t in out.values()), "an output element was not written (or is not finite)"
    return out


@pytest.mark.parametrize("Cd,G,M,B,Tp", CASES)
def test_embed_backward_against_fp64_autograd(L, Cd, G, M, B, Tp):
    c = _case(Cd, G, M, B, Tp)
    N = G * G
    got = _run(L, c["x"], c["gs"], Cd, G, M, B, Tp)
    tag = f"embed C {Cd} G {G} M {M} B {B} Tp {Tp}"
    assert torch.equal(got["g_pos"][0], got["g_cls"]), "g_pos[0] != g_cls"
    # two calls give equal bits
    again = _run(L, c["x"], c["gs"], Cd, G, M, B, Tp)
    assert all(torch.equal(again[k], got[k]) for k in got), "two calls differ"
    # other finite values in the rows > N of g_stream move no bit
    row = torch.arange(B * Tp) % Tp
    assert Tp > N + 1
    other = c["gs"].clone()
    other[row > N] = rn(torch.Generator().manual_seed(77 + G), B * Tp, Cd)[row > N] * 5.0 - 2.0
    o = _run(L, c["x"], other, Cd, G, M, B, Tp)
    assert all(torch.equal(o[k], got[k]) for k in got), "a row behind the class row was read"
    # another class row changes g_cls and g_pos[0] and nothing else
    other = c["gs"].clone()
    other[row == N] += 1.0 + rn(torch.Generator().manual_seed(78 + G), B, Cd).abs()
    o = _run(L, c["x"], other, Cd, G, M, B, Tp)
    assert torch.equal(o["g_patch_w"], got["g_patch_w"]) and torch.equal(o["g_patch_b"], got["g_patch_b"]), "the class row reached the patch sums"
    assert torch.equal(o["g_pos"][1:], got["g_pos"][1:]), "the class row reached the table's patch rows"
    assert bool((o["g_cls"] != got["g_cls"]).all()) and torch.equal(o["g_pos"][0], o["g_cls"])
    # the backbone_train wrapper is the same call
    w = bt.embed_backward(c["x"].to(dev()), c["gs"].to(dev()), B, G, M, Tp)
    torch.cuda.synchronize()
    assert set(w) == set(got) and all(torch.equal(w[k], got[k]) for k in got)
    bo.gate(tag, [(k, got[k], c["y32"][k], c["r64"][k]) for k in eo.NAMES])


# ------------------------------------------------------------------------------------------------------ the model
def _new_model3():
    """ViT-S, 224^2, backbone depth 3, synthetic weights (stored table 37 x 37, grid 16 x 16); every parameter frozen -> (model, state dict)."""
    import synthetic
    import test_gpu_feature_grad as tf
    from multi_hmr_amd import Model
    a = tf._assets()
    sd = synthetic.make_state_dict(tf.NAME, tf.S, seed=42, depth_override=3, mean_params=a["mean"])
    m = Model(backbone=tf.NAME, img_size=tf.S, smplx_data=a["data"], mean_params=a["mean"], backbone_depth=3, precision="f16")
    m.load_state_dict(sd, strict=True)
    return m.to(dev()).eval(), sd


def _oracle_encoder(sd):
    """oracle/dinov2_ref's encoder with the model's weights, on the CPU."""
    from oracle import dinov2_ref
    import test_gpu_feature_grad as tf
    enc = dinov2_ref.build(tf.NAME, depth_override=3)
    pre = bt.ENCODER
    enc.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)
    return enc


def test_model_train_embeddings():
    import test_gpu_backbone_backward as tgb
    tf, x, y, builder, kw, total = tgb._training_scene()
    m, sd = _new_model3()
    named = dict(m.named_parameters())
    names_b, names_e = bt.backbone_parameter_names(3, 3), bt.embedding_parameter_names()
    plain = m(x, **kw)                                          # no switch at all
    # embeddings off: the block and norm gradients to compare with
    m.train_backbone_(3)
    total(m, m(x, train_backbone=True, **kw)).backward()
    off = {k: named[k].grad.clone() for k in names_b}
    assert all(named[k].grad is None for k in names_e)
    tf._clear(m)
    m.train_embeddings_()
    assert {k for k, p in named.items() if p.requires_grad} == set(names_b) | set(names_e)
    out = m(x, train_backbone=True, **kw)
    tf._same(plain, out)
    total(m, out).backward()
    grads = {k: named[k].grad.clone() for k in names_b + names_e}
    for k in names_e:
        assert grads[k].shape == named[k].shape and bool(torch.isfinite(grads[k]).all()) and bool((grads[k] != 0).any()), k
    assert all(p.grad is None for k, p in named.items() if k not in grads)
    assert all(torch.equal(grads[k], off[k]) for k in names_b), "the embedding switch moved a block or norm gradient"
    # the same four gradients from embed_backward fed with mhmr_vit_tail_backward's g_stream, on the tapped workspace of that forward
    P = m._packed
    ws = m._workspace(P, 2, tap=3)
    assert len(ws["parts"]) == 1
    f = m.backbone_features(x).clone().requires_grad_()
    total(m, m.forward_features(f, **kw)).backward()
    enc, N, Cd, Tp, bufs = m.backbone.encoder, P["N"], P["C"], ws["Tp"], ws["parts"][0]["bufs"]
    blocks = [bt.block_tensors(b, dev()) for b in enc.blocks]
    g_stream, _, _, _ = bt.tail_backward(enc.norm.weight.detach(), enc.norm.bias.detach(), blocks, bufs["tap"], bufs["resid"], f.grad, 2, N, Tp, P["H"])
    direct = bt.embed_backward(x, g_stream, 2, P["G"], 37, Tp)
    for field, pname in bt.EMBED_FIELDS.items():
        assert torch.equal(direct[field].view_as(grads[bt.ENCODER + pname]), grads[bt.ENCODER + pname]), pname
    # the gate: the oracle of the embedding chained behind the tail's own oracle, each in its dtype
    ref = _oracle_encoder(sd)
    tap, resid, g_feat, xc = bufs["tap"].cpu(), bufs["resid"].cpu(), f.grad.cpu().reshape(2 * N, Cd), x.cpu()
    params = dict(patch_w=ref.patch_embed.proj.weight, patch_b=ref.patch_embed.proj.bias, cls_token=ref.cls_token, pos_embed=ref.pos_embed)
    want = {}
    for dt in (torch.float64, torch.float32):
        gs = tgb._tail_oracle(ref, tap, resid, g_feat, 2, N, Tp, dt)["g_stream"]
        want[dt] = eo.embed_backward(xc, params, gs, 2, P["G"], Tp, dt)
    bo.gate("model embeddings", [(k, direct[k], want[torch.float32][k], want[torch.float64][k]) for k in eo.NAMES])
    # a backward after the next forward of the same batch size still raises
    out = m(x, train_backbone=True, **kw)
    m(x, train_backbone=True, **kw)
    with pytest.raises(_lib.MhmrError, match="before the next forward"):
        total(m, out).backward()
    # the tail alone takes the embedding along too
    tf._clear(m)
    fa = m.backbone_features(x, train_backbone=True)
    fa.backward(f.grad)
    assert all(torch.equal(named[k].grad, grads[k]) for k in names_b + names_e)


def test_repack_embeddings_and_a_trainer_step(tmp_path):
    import loss_oracle as lo
    import test_gpu_backbone_backward as tgb
    from multi_hmr_amd import Loss, Trainer
    tf, x, y, builder, kw, total = tgb._training_scene()
    m, _ = _new_model3()
    m.train_backbone_(3).train_embeddings_()
    opt = torch.optim.Adam(m.backbone_parameters(3) + m.embedding_parameters(), lr=1e-4)
    total(m, m(x, train_backbone=True, **kw)).backward()
    before = [p.detach().clone() for p in m.embedding_parameters()]
    packed = {k: t.clone() for k, t in m._packed["vit"]["embed_t"].items()}
    opt.step()
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, m.embedding_parameters())), "an embedding parameter did not move"
    stale = m(x, **kw)
    m.repack_backbone()
    assert all(not torch.equal(packed[k], t) for k, t in m._packed["vit"]["embed_t"].items()), "a packed embedding tensor was not refreshed"
    fresh = m(x, **kw)
    assert not torch.equal(stale["readout"], fresh["readout"]), "the step did not reach the packed weights"
    m.repack()
    tf._same(m(x, **kw), fresh)
    # a Trainer over heads + every block + the embedding with a torch optimiser
    m, _ = _new_model3()
    m.train_heads_(True).train_backbone_(3).train_embeddings_()
    ns = lo.default_args(save_dir=str(tmp_path), name="run", nb_max_ckpt=2, max_epochs=1, log_freq=1, det_thresh=0.3, nms_kernel_size=3)
    opt = torch.optim.Adam(m.heads_parameters() + m.backbone_parameters(3) + m.embedding_parameters(), lr=1e-4)
    tr = Trainer(m, Loss(ns), opt, ns, builder)
    tr.current_epoch = lo.DEFAULTS["start_2d_epoch"]
    w0 = [p.detach().clone() for p in m.embedding_parameters()]
    d = tr.train_step(x, y)
    assert all(bool(torch.isfinite(v).all()) for v in d.values())
    assert all(not torch.equal(a, p.detach()) for a, p in zip(w0, m.embedding_parameters()))
    # the embedding alone in the optimiser still makes the step a backbone step
    m, _ = _new_model3()
    m.train_backbone_(3).train_embeddings_()
    tr = Trainer(m, Loss(ns), torch.optim.Adam(m.embedding_parameters(), lr=1e-4), ns, builder)
    tr.current_epoch = lo.DEFAULTS["start_2d_epoch"]
    w0 = [p.detach().clone() for p in m.embedding_parameters()]
    d = tr.train_step(x, y)
    assert all(bool(torch.isfinite(v).all()) for v in d.values())
    assert all(not torch.equal(a, p.detach()) for a, p in zip(w0, m.embedding_parameters()))
