"""-m "not gpu": the host side of the fused Adam step (csrc/optim.hip, multi_hmr_amd/optim.py) -- the fp64 oracle
against torch.optim.Adam, the segment table against the pack itself (Model._head_tensors / _detect_tensors on the CPU), header / binding
agreement, and every documented error code of mhmr_adam_step before any launch."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import optim_oracle as oo
from multi_hmr_amd import _lib
from multi_hmr_amd.optim import HeadsAdam, head_segments, packed_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, S = "dinov2_vits14", 224


# ------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("max_norm", [None, 0.5, 1e3])
def test_oracle_equals_torch_adam_in_fp64(max_norm):
    """Three steps; tensor 1 has no gradient at step 2 (its step count falls behind), tensor 3 never has one; with and without the clip
    (0.5 clips, 1e3 does not)."""
    g = torch.Generator().manual_seed(3)
    shapes = [(7,), (3, 5), (1,), (4,)]
    params = [torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_(True) for s in shapes]
    opt = torch.optim.Adam(params, lr=3e-3, betas=(0.8, 0.95), eps=1e-6)
    state = [dict(p=p.detach().numpy().copy(), m=np.zeros(s), v=np.zeros(s), step=0) for p, s in zip(params, shapes)]
    for step in range(3):
        grads = [torch.randn(*s, generator=g, dtype=torch.float64) for s in shapes]
        grads[3] = None
        if step == 1:
            grads[1] = None
        grads[0][2] = 0.0
        for p, gr in zip(params, grads):
            p.grad = None if gr is None else gr.clone()
        if max_norm is not None:
            want_norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        state, norm = oo.adam_step(state, [None if gr is None else gr.numpy() for gr in grads], 3e-3, (0.8, 0.95), 1e-6, max_norm)
        if max_norm is not None:
            assert abs(norm - float(want_norm)) <= 1e-14 * float(want_norm)
        for i, (p, st) in enumerate(zip(params, state)):
            ref = p.detach().numpy()
            assert np.max(np.abs(st["p"] - ref)) <= 1e-14 * np.max(np.abs(ref)), (step, i)
            if p in opt.state:
                ts = opt.state[p]
                assert int(ts["step"]) == st["step"]
                for k, tk in (("m", "exp_avg"), ("v", "exp_avg_sq")):
                    r = ts[tk].numpy()
                    assert np.max(np.abs(st[k] - r)) <= 1e-14 * max(np.max(np.abs(r)), 1e-300), (step, i, k)
            else:
                assert st["step"] == 0
    assert [st["step"] for st in state] == [3, 2, 3, 0]


# ------------------------------------------------------------------------------------------------------ the table against the pack
@functools.lru_cache(maxsize=None)
def _assets():
    import synthetic
    data, mean = synthetic.make_smplx_data(seed=0), synthetic.make_mean_params(seed=0)
    return dict(data=data, mean=mean, sd=synthetic.make_state_dict(NAME, S, seed=42, depth_override=4, mean_params=mean))


def _cpu_model():
    from multi_hmr_amd import Model
    a = _assets()
    m = Model(backbone=NAME, img_size=S, smplx_data=a["data"], mean_params=a["mean"], backbone_depth=4, precision="f16")
    m.load_state_dict(a["sd"], strict=True)
    return m.eval()


def _pack(m, tdt):
    from multi_hmr_amd.packing import roundup
    Cc = m.embed_dim + m.camera_embed_dim
    P = dict(hph_t=m._head_tensors(torch.device("cpu"), tdt, Cc, roundup(Cc, 64)))
    P.update(m._detect_tensors(torch.device("cpu"), tdt))
    return P


def _targets(m, P):
    """{target: tensor} of EVERY packed head tensor of the pack (the table must account for each)."""
    out = {("head", n): P["hph_t"][n] for n in m.HEAD_TENSORS}
    for l, layer in enumerate(P["hph_t"]["layers"]):
        out.update({("layer", l, n): t for n, t in layer.items()})
    out.update({("det", n): P[n] for n in ("cls0_w", "cls0_b", "cls2_w", "cls2_b")})
    return out


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16])
def test_segment_table_reproduces_the_pack_bit_for_bit(tdt):
    """The packed tensors of the fixture, then every head / detector parameter perturbed; the table applied in numpy to the OLD packed
    tensors gives the pack of the NEW parameters bit for bit, padding and init_tail included, and every packed element has one writer
    or none -- none exactly in the padding of tok_w and to_kv16 and in init_tail."""
    m = _cpu_model()
    segs = head_segments(m)
    named = dict(m.named_parameters())
    covered = [s["param"] for s in segs] + [s["param2"] for s in segs if s["param2"]]
    want = [n for n, _ in m.named_parameters() if n.startswith(("mlp_offset.", "x_attention_head.", "mlp_classif."))]
    assert sorted(covered) == sorted(want) and len(set(covered)) == len(covered)
    assert sorted(covered) == sorted(HeadsAdam(m)._names)
    old = _pack(m, tdt)
    packed = {k: oo.bits(t) for k, t in _targets(m, old).items()}
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for n in covered:
            named[n].add_(torch.randn(named[n].shape, generator=g) * 0.03)
    new = _targets(m, _pack(m, tdt))
    values = {n: named[n].detach().numpy() for n in covered}
    addends = {n: b[0].detach().numpy() for n, b in m.named_buffers() if n.startswith("x_attention_head.init_")}
    assert set(s["target"] for s in segs) | {("head", "init_tail")} == set(packed)
    claims = oo.apply_segments(segs, values, addends, packed, tdt)
    changed = 0
    for k, t in new.items():
        ref = oo.bits(t)
        assert np.array_equal(packed[k], ref), k
        changed += int((oo.bits(_targets(m, old)[k]) != ref).sum())
        assert claims[k].max() <= 1, k
        free = claims[k].reshape(t.shape) == 0
        if k == ("head", "init_tail"):
            assert free.all()
        elif k == ("head", "tok_w"):
            cols = m.embed_dim + m.camera_embed_dim + 318 + m.num_betas + 3
            assert not free[:, :cols].any() and free[:, cols:].all() and t.shape[1] > cols and not t[:, cols:].any()
        elif k[0] == "layer" and k[2] == "to_kv16":
            Cc = m.embed_dim + m.camera_embed_dim
            assert not free[:, :Cc].any() and free[:, Cc:].all() and t.shape[1] > Cc and not t[:, Cc:].float().any()
        else:
            assert not free.any(), k
    assert changed > 1000        # (the perturbation reached the packed copies: the comparison above is not of unchanged buffers)


def test_packed_target_names_every_tensor_of_a_pack():
    m = _cpu_model()
    P = _pack(m, torch.float16)
    for s in head_segments(m):
        t = packed_target(P, s["target"])
        n = dict(m.named_parameters())[s["param"]].numel()
        assert s["offset"] + (n // s["cols"] - 1) * s["pitch"] + s["cols"] <= t.numel() and n % s["cols"] == 0
        assert t.dtype == (torch.float32 if s["kind"] == "f32" else torch.float16)
    assert len(head_segments(m, detection=False)) == len(head_segments(m)) - 4


# ------------------------------------------------------------------------------------------------------ ABI
def test_header_binding_and_version():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    assert "mhmr_adam_step" in declared and "mhmr_adam_step" in _lib._SIGS and declared == set(_lib.EXPORTS)
    assert re.search(r"#define MHMR_VERSION 106\b", header) and _lib.VERSION == 106
    assert "optim.hip" in _lib.SOURCES and "-ffp-contract=off" in _lib.EXTRA_FLAGS["optim.hip"]
    assert int(re.search(r"#define MHMR_ADAM_CHUNK (\d+)", header).group(1)) == _lib.ADAM_CHUNK
    for i, n in enumerate(("NONE", "F32", "F16", "BF16")):
        assert int(re.search(rf"#define MHMR_ADAM_PACK_{n} (\d+)", header).group(1)) == getattr(_lib, "ADAM_PACK_" + n) == i
    body = re.search(r"typedef struct \{([^}]*)\} mhmr_adam_segment;", header).group(1)
    fields = re.findall(r"(\w+)\s*[;,]", body)
    assert fields == [n for n, _ in _lib.AdamSegment._fields_]
    assert C.sizeof(_lib.AdamSegment) == 120
    _lib.build()
    assert _lib.lib().mhmr_version() == 106


def _seg(**kw):
    """A valid one-segment table over fake (never dereferenced) device addresses."""
    s = _lib.AdamSegment()
    s.param, s.exp_avg, s.exp_avg_sq, s.grad, s.packed = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    s.n, s.cols, s.pitch, s.packed_kind, s.chunk0 = 40, 5, 8, _lib.ADAM_PACK_F32, 0
    s.step_size, s.bc2_sqrt, s.step_size2, s.bc2_sqrt2 = 1e-3, 0.03, 1e-3, 0.03
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _call(segs, nsegs=None, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.0, partials=None, count=0, norm=None, dev=0x9000):
    _lib.build()
    arr = (_lib.AdamSegment * max(len(segs), 1))(*segs)
    return _lib.lib().mhmr_adam_step(arr if segs is not None else None, dev, len(segs) if nsegs is None else nsegs, beta1, beta2, eps, max_norm,
                                     partials, count, norm, None)


def test_bad_arguments_are_refused_before_any_launch():
    """Every call here must return before the first launch: there is no GPU under this test."""
    ARG, SHAPE = -1, -2
    assert _call([], nsegs=0) == 0                                          # nothing to do
    assert _call([], nsegs=-1) == ARG
    assert _call([_seg()], dev=None) == ARG
    assert _lib.lib().mhmr_adam_step(None, 0x9000, 1, 0.9, 0.999, 1e-8, 0.0, None, 0, None, None) == ARG
    for kw in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(eps=-1e-8), dict(max_norm=float("nan"))):
        assert _call([_seg()], **kw) == ARG, kw
    for kw in (dict(param=None), dict(exp_avg=None), dict(exp_avg_sq=None), dict(param2=0x6000), dict(param2=0x6000, exp_avg2=0x7000, exp_avg_sq2=0x8000),
               dict(param2=0x6000, exp_avg2=0x7000, exp_avg_sq2=0x8000, grad2=0x8800, addend=0x8900),
               dict(param2=0x6000, exp_avg2=0x7000, exp_avg_sq2=0x8000, grad2=0x8800, step_size2=0.0),
               dict(packed_kind=4), dict(packed_kind=-1), dict(packed=None), dict(chunk0=1), dict(step_size=0.0), dict(step_size=float("inf")),
               dict(bc2_sqrt=float("nan")), dict(bc2_sqrt=-1.0)):
        assert _call([_seg(**kw)]) == ARG, kw
    for kw in (dict(n=0), dict(n=-5), dict(cols=0), dict(pitch=4), dict(n=41)):
        assert _call([_seg(**kw)]) == SHAPE, kw
    # the second segment's first chunk: 40 elements are one chunk, 2049 are two
    assert _call([_seg(), _seg(packed=0x50000, chunk0=0)]) == ARG
    assert _call([_seg(n=2049, cols=1, pitch=1), _seg(packed=0x50000, chunk0=1)]) == ARG
    # packed copies of two segments that overlap (the second starts inside the first's 5 * 8 floats), also across element sizes
    assert _call([_seg(), _seg(packed=0x5000 + 4 * 36, chunk0=1)]) == ARG
    assert _call([_seg(), _seg(packed=0x5000 - 2, chunk0=1, packed_kind=_lib.ADAM_PACK_F16)]) == ARG
    # clipping needs its buffers, and a partial per chunk
    assert _call([_seg()], max_norm=1.0) == ARG
    assert _call([_seg()], max_norm=1.0, partials=0xA000, count=1) == ARG
    assert _call([_seg()], max_norm=1.0, partials=0xA000, count=0, norm=0xB000) == ARG
    assert _call([_seg()], max_norm=1e-60, partials=0xA000, count=1, norm=0xB000) == ARG


def test_heads_adam_refuses_what_it_does_not_implement():
    m = _cpu_model()
    for kw in (dict(weight_decay=0.01), dict(amsgrad=True), dict(maximize=True), dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(max_grad_norm=0.0)):
        with pytest.raises(ValueError):
            HeadsAdam(m, **kw)
    opt = HeadsAdam(m, lr=1e-4, detection=False)
    assert len(opt.param_groups[0]["params"]) == len(m.heads_parameters())
    with pytest.raises(_lib.MhmrError, match="CPU"):
        opt.step()
    opt.param_groups[0]["weight_decay"] = 0.1
    with pytest.raises(ValueError):
        opt.step()
    # state dicts travel both ways between HeadsAdam and torch.optim.Adam over the same list
    a = torch.optim.Adam(m.heads_parameters() + m.detection_parameters(), lr=1e-4)
    h = HeadsAdam(m, lr=1e-4)
    a.load_state_dict(h.state_dict())
    h.load_state_dict(a.state_dict())
    assert h.param_groups[0]["lr"] == 1e-4 and h.param_groups[0]["weight_decay"] == 0
