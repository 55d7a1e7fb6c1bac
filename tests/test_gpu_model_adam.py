"""-m gpu: ``ModelAdam`` -- one fused Adam step over heads, detector, backbone and token embedding that also rewrites the packed encoder
(multi_hmr_amd/optim.py, csrc/optim.hip + csrc/encoder_pack.hip).

Fixtures: a synthetic ViT-B/14 at 224^2 with two blocks and ``wlo="v+proj@0-1"`` (block 1 has both LayerNorm folds, block 0 fc1's; V and
proj carry low halves) and the ViT-S depth-4 model of tests/test_gpu_optim.py (no fold, no low halves); two images, persons (2, 1), random
cotangents.  The contract: after ``step()`` the packed encoder holds what ``repack_backbone()`` writes from the updated parameters -- bit
for bit, except the fp64-sum entries (folded biases, bf16 column sums, position table), which may sit one ulp away (counts are printed)."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import encoder_pack_oracle as eo  # noqa: E402
import optim_oracle as oo  # noqa: E402
import test_gpu_optim as go  # noqa: E402
from multi_hmr_amd import _lib  # noqa: E402
from multi_hmr_amd.optim import ModelAdam  # noqa: E402

LR, BETAS, EPS = go.LR, go.BETAS, go.EPS
FIXED_ORDER = ("qkv_b", "fc1_b", "qkv_colsum", "fc1_colsum", "pos", "cls_pos0")
STALE = "backward must run before the next forward of the same batch size and before repack_(heads|backbone)"
dev = go.dev


@functools.lru_cache(maxsize=None)
def _vitb_sd():
    import synthetic
    a = go._assets()
    return synthetic.make_state_dict("dinov2_vitb14", go.S, seed=42, depth_override=2, mean_params=a["mean"])


def _new_model(kind, precision="f16", sd=None):
    if kind == "vits":
        return go._new_model(precision, sd=sd)
    from multi_hmr_amd import Model
    a = go._assets()
    m = Model(backbone="dinov2_vitb14", img_size=go.S, smplx_data=a["data"], mean_params=a["mean"], backbone_depth=2, precision=precision,
              wlo="v+proj@0-1")
    m.load_state_dict(_vitb_sd() if sd is None else sd, strict=True)
    return m.to(dev()).eval()


def _depth(m):
    return len(m.backbone.encoder.blocks)


def _train_all(m):
    return m.train_heads_(True).train_detection_(True).train_backbone_(_depth(m)).train_embeddings_()


def _trainable(m):
    return m.heads_parameters() + m.detection_parameters() + m.backbone_parameters(m._backbone_n) + m.embedding_parameters()


def _forward(m, x, K, idx):
    return m(x, idx=idx, K=K, is_training=True, return_readout=True, train_heads=True, train_detection=True, train_backbone=True)


def _backward(m, x, K, idx, seed):
    out = _forward(m, x, K, idx)
    g = torch.Generator().manual_seed(seed)
    total = 0.0
    for k in ("readout", "offset", "scores"):
        total = total + (out[k] * torch.randn(out[k].shape, generator=g).to(dev())).sum()
    total.backward()
    return out


def _encoder_bits(m):
    v = m._packed["vit"]
    out = {("norm", n): t for n, t in v["norm_t"].items()}
    out.update({("embed", n): t for n, t in v["embed_t"].items()})
    for l, bt in enumerate(v["block_t"]):
        out.update({("block", l, n): t for n, t in bt.items() if t is not None})
    return {k: oo.bits(t) for k, t in out.items()}, {k: t.dtype for k, t in out.items()}


def _compare(after, repacked, dtypes, bf16):
    """The bit-equal set must be equal; the fixed-order fp64 sums within one ulp.  -> how many of those moved."""
    moved = 0
    for k in after:
        f = k[-1]
        if f in FIXED_ORDER and dtypes[k] == torch.float32 and not (f.endswith("colsum") and not bf16):
            d = eo.ulp_distance(after[k].view(np.float32), repacked[k].view(np.float32))
            assert d.max() <= 1, (k, int(d.max()))
            moved += int((d > 0).sum())
        else:
            assert np.array_equal(after[k], repacked[k]), k
    return moved


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("kind", ["vitb", "vits"])
def test_step_leaves_what_the_two_repacks_would(kind, precision):
    m = _train_all(_new_model(kind, precision))
    x, K, idx = go._scene((2, 1), 1)
    opt = ModelAdam(m, lr=1e-3, max_grad_norm=1e9)
    before, counts = None, []
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        _backward(m, x, K, idx, 10 + step)
        P = m._packed
        gens = P["heads_generation"], P["backbone_generation"]
        if step == 0:
            before, _ = _encoder_bits(m)
            if kind == "vitb":
                assert P["fold"] and [P["vit"]["blocks"][l].flags for l in range(2)] == [2, 3] and P["lo_passes"] == {0: {"v", "proj"}, 1: {"v", "proj"}}
        opt.step()
        assert (P["heads_generation"], P["backbone_generation"]) == (gens[0] + 1, gens[1] + 1) and m._packed is P
        after, dtypes = _encoder_bits(m)
        heads = go._packed_bits(m)
        m.repack_backbone()
        m.repack_heads()
        counts.append(_compare(after, _encoder_bits(m)[0], dtypes, precision == "bf16"))
        assert all(np.array_equal(a, b) for a, b in zip(heads, go._packed_bits(m)))
    assert set(after) == set(before) and sum(int((after[k] != before[k]).sum()) for k in after) > 1000000
    assert all(int((after[k] != before[k]).sum()) > 0 for k in after), "a packed encoder tensor the steps did not move"
    assert float(opt.last_grad_norm) > 0
    print(f"\n{kind} {precision}: fixed-order elements one ulp from repack_backbone()'s after steps 1, 2: {counts}")


@pytest.mark.parametrize("max_norm", [None, 0.05])
def test_three_steps_against_torch_adam_and_the_repacks(max_norm):
    """Twin ViT-S models, the same cotangents: ModelAdam against torch.optim.Adam (+ clip_grad_norm_) + repack_heads() + repack_backbone().
    Per parameter the 4x rule of tests/test_gpu_optim.py: each side's one-step error against the fp64 oracle from the state the step
    started from.  With max_norm (which clips: the norm is ~ 1e3) last_grad_norm is the fp64 norm over ALL stepped gradients to fp32 rounding."""
    ma, mb = (_train_all(_new_model("vits")) for _ in range(2))
    x, K, idx = go._scene((2, 1), 1)
    oa = ModelAdam(ma, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=max_norm)
    ob = torch.optim.Adam(_trainable(mb), lr=LR, betas=BETAS, eps=EPS, foreach=False)
    names, worst = oa._names, []
    assert len(names) == len(_trainable(ma))
    for step in range(3):
        rows = {}
        for tag, m, opt in (("ours", ma, oa), ("torch", mb, ob)):
            opt.zero_grad(set_to_none=True)
            _backward(m, x, K, idx, 20 + step)
            start = []
            for p in _trainable(m):
                st = opt.state.get(p, {})
                z = lambda: torch.zeros_like(p)
                start.append(dict(p=p.detach().cpu().numpy().copy(), m=st.get("exp_avg", z()).cpu().numpy().copy(),
                                  v=st.get("exp_avg_sq", z()).cpu().numpy().copy(), step=int(st.get("step", 0))))
            grads = [p.grad.detach().cpu().numpy().copy() for p in _trainable(m)]
            ref, ref_norm = oo.adam_step(start, grads, LR, BETAS, EPS, max_norm)
            if tag == "torch":
                if max_norm:
                    torch.nn.utils.clip_grad_norm_(_trainable(m), max_norm, foreach=False)
                opt.step()
                m.repack_heads()
                m.repack_backbone()
            else:
                opt.step()
                if max_norm:
                    assert ref_norm > 10 * max_norm                      # (it does clip)
                    got = float(opt.last_grad_norm)
                    assert abs(got - ref_norm) <= 2.0 ** -23 * ref_norm, (got, ref_norm)
            rows[tag] = [max(float(np.max(np.abs(p.detach().cpu().double().numpy() - r["p"]))),
                             float(np.max(np.abs(opt.state[p]["exp_avg"].cpu().double().numpy() - r["m"]))),
                             float(np.max(np.abs(opt.state[p]["exp_avg_sq"].cpu().double().numpy() - r["v"]))))
                         for p, r in zip(_trainable(m), ref)]
            assert all(int(opt.state[p]["step"]) == step + 1 for p in _trainable(m))
        for n, e_us, e_t in zip(names, rows["ours"], rows["torch"]):
            assert e_us <= 4.0 * e_t, (step, n, e_us, e_t)
        i = int(np.argmax([a / max(b, 1e-300) for a, b in zip(rows["ours"], rows["torch"])]))
        worst.append(dict(step=step + 1, parameter=names[i], ours=rows["ours"][i], torch=rows["torch"][i]))
        bound = 2.0 * LR * sum(t ** 0.5 for t in range(1, step + 2))      # (tests/test_gpu_optim.py: why no tighter bound exists)
        for pa, pb in zip(_trainable(ma), _trainable(mb)):
            assert float((pa.detach() - pb.detach()).abs().max()) <= bound
    go.report(f"ModelAdam vs torch.optim.Adam (fp32, same device), max_norm {max_norm}, worst ratio per step: max abs error of p / m / v vs fp64", worst)


def test_one_trained_block_leaves_the_rest_alone():
    """train_backbone_(1) on the ViT-B fixture: block 0 and the token embedding keep every bit -- parameters, moments (none), packed."""
    m = _new_model("vitb").train_heads_(True).train_detection_(True).train_backbone_(1)
    x, K, idx = go._scene((2, 1), 2)
    opt = ModelAdam(m, lr=1e-3)
    _backward(m, x, K, idx, 30)
    named = dict(m.named_parameters())
    frozen = {n: p.detach().clone() for n, p in named.items() if "blocks.0." in n or n.endswith(("pos_embed", "cls_token")) or "patch_embed" in n}
    assert len(frozen) == 14 + 4 and all(named[n].grad is None for n in frozen)
    before, _ = _encoder_bits(m)
    opt.step()
    after, _ = _encoder_bits(m)
    assert all(np.array_equal(oo.bits(named[n]), oo.bits(q)) and named[n] not in opt.state for n, q in frozen.items())
    for k in after:
        if k[0] == "embed" or (k[0] == "block" and k[1] == 0):
            assert np.array_equal(after[k], before[k]), k
        else:
            assert not np.array_equal(after[k], before[k]), k
    m.repack_backbone()
    assert _compare(after, _encoder_bits(m)[0], _encoder_bits(m)[1], False) >= 0


def test_backward_pending_across_the_step_raises():
    m = _train_all(_new_model("vits"))
    x, K, idx = go._scene((2, 1), 4)
    opt = ModelAdam(m, lr=1e-4)
    _backward(m, x, K, idx, 32)
    out = _forward(m, x, K, idx)
    opt.step()
    with pytest.raises(_lib.MhmrError, match=STALE):
        (out["readout"].sum() + out["scores"].sum()).backward()


def test_parameters_only_before_the_first_forward():
    m = _train_all(_new_model("vitb"))
    assert m._packed is None
    opt = ModelAdam(m, lr=1e-3)
    g = torch.Generator().manual_seed(1)
    old = [p.detach().clone() for p in _trainable(m)]
    for p in _trainable(m):
        p.grad = (0.01 * torch.randn(p.shape, generator=g)).to(dev())
    opt.step()
    assert m._packed is None and all(not torch.equal(p, q) for p, q in zip(_trainable(m), old))
    x, K, idx = go._scene((2, 1), 5)
    m(x, idx=idx, K=K, is_training=True)                                         # packs the updated parameters
    opt.step()                                                                  # the table is rebuilt for the new pack
    after, dtypes = _encoder_bits(m)
    m.repack_backbone()
    _compare(after, _encoder_bits(m)[0], dtypes, False)


def test_state_dict_round_trip_through_torch_adam():
    """Two steps; the state through torch.optim.Adam's state_dict and back into a fresh ModelAdam on a twin; the third step has the bits
    of the uninterrupted run."""
    x, K, idx = go._scene((2, 1), 6)
    ma = _train_all(_new_model("vits"))
    oa = ModelAdam(ma, lr=LR)
    for step in range(2):
        oa.zero_grad(set_to_none=True)
        _backward(ma, x, K, idx, 40 + step)
        oa.step()
    mb = _train_all(_new_model("vits", sd=ma.state_dict()))
    via = torch.optim.Adam(_trainable(mb), lr=LR)
    via.load_state_dict(copy.deepcopy(oa.state_dict()))
    ob = ModelAdam(mb, lr=LR)
    ob.load_state_dict(via.state_dict())
    for m, opt in ((ma, oa), (mb, ob)):
        opt.zero_grad(set_to_none=True)
        _backward(m, x, K, idx, 42)
        opt.step()
    for pa, pb in zip(_trainable(ma), _trainable(mb)):
        assert float(oa.state[pa]["step"]) == float(ob.state[pb]["step"]) == 3.0
        assert torch.equal(oa.state[pa]["exp_avg"].isfinite(), ob.state[pb]["exp_avg"].isfinite())
        # (the reloaded twin's fixed-order entries may sit an ulp from the stepped model's: close, not bit-equal)
        assert float((pa.detach() - pb.detach()).abs().max()) <= 2.0 * LR


def test_trainer_step_and_the_next_forward(tmp_path):
    """Trainer.train_step with ModelAdam re-packs nothing afterwards; the next forward is that of the model after repack() on every key
    when no fixed-order entry sits an ulp from the host pack's (the count is printed), and within 1e-3 of it otherwise."""
    import loss_oracle as lso
    import test_gpu_backbone_backward as tb
    from multi_hmr_amd import Loss, Trainer
    _, x, y, builder, kw, _ = tb._training_scene()
    m = _train_all(_new_model("vitb"))
    ns = lso.default_args(save_dir=str(tmp_path), name="run", nb_max_ckpt=2, max_epochs=1, log_freq=1, det_thresh=0.3, nms_kernel_size=3)
    opt = ModelAdam(m, lr=1e-4)
    tr = Trainer(m, Loss(ns), opt, ns, builder)
    tr.current_epoch = lso.DEFAULTS["start_2d_epoch"]
    calls = []
    m.repack_backbone = lambda: calls.append("backbone")
    m.repack_heads = lambda: calls.append("heads")
    w0 = m.backbone_parameters(2)[4].detach().clone()
    d = tr.train_step(x, y)
    assert all(bool(torch.isfinite(v).all()) for v in d.values()) and not torch.equal(w0, m.backbone_parameters(2)[4].detach())
    assert calls == []
    after, (bits_a, dtypes) = m(x, **kw), _encoder_bits(m)
    m.repack()
    ref = m(x, **kw)
    moved = _compare(bits_a, _encoder_bits(m)[0], dtypes, False)
    print(f"\nTrainer step, ViT-B f16: {moved} fixed-order elements one ulp from the host pack's")
    assert list(after) == list(ref)
    for k in after:
        if moved == 0:
            assert torch.equal(after[k], ref[k]), k
        else:
            assert torch.allclose(after[k].float(), ref[k].float(), rtol=1e-3, atol=1e-3), k


def test_step_does_not_synchronise():
    """One step (the second: the table and the taps exist) under torch's synchronisation debug mode: nothing waits for the device."""
    m = _train_all(_new_model("vitb"))
    x, K, idx = go._scene((2, 1), 7)
    opt = ModelAdam(m, lr=1e-4, max_grad_norm=1.0)
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        _backward(m, x, K, idx, 50 + step)
        if step == 0:
            opt.step()
            continue
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):                                    # (the mode does see a synchronisation on this build)
                opt.last_grad_norm.item()
            opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert float(opt.last_grad_norm) > 0
