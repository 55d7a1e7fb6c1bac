"""-m "not gpu": the host side of the optimiser for the whole model (csrc/encoder_pack.hip, multi_hmr_amd/optim.py ModelAdam; DESIGN.md
section 34) -- ``encoder_segments`` and ``encoder_jobs`` applied in numpy (tests/encoder_pack_oracle.py) against ``vit.pack_block`` /
``vit.pack_embeddings`` on the CPU, that together they write every packed encoder tensor exactly once, the oracle's position table
against ``packing.interpolate_pos_embed``, header / binding agreement, the error codes of ``mhmr_vit_repack`` that come before any launch,
and the command line's ``--fused_adam``."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import encoder_pack_oracle as eo
import optim_oracle as oo
from multi_hmr_amd import _lib, packing, vit
from multi_hmr_amd.backbone_train import ENCODER
from multi_hmr_amd.optim import ModelAdam, encoder_jobs, encoder_segments, packed_target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 224
#: (backbone, depth, precision, wlo, lnfold): ViT-B width with both folds and V / proj low halves; the same without the fold; ViT-S (no
#: fold, no low halves); f16x3 triples; and ViT-S with the fold forced on (the masked form: rows zero-padded to 512)
PACKS = {"vitb_fold": ("dinov2_vitb14", 2, None, "v+proj@0-1", True), "vitb_nofold": ("dinov2_vitb14", 2, None, "v+proj@0-1", False),
         "vits": ("dinov2_vits14", 2, None, None, None), "x3": ("dinov2_vits14", 2, "f16x3", None, None),
         "vits_cpad": ("dinov2_vits14", 2, None, "v+proj@0-1", True)}
FIXED_ORDER = ("qkv_b", "fc1_b", "qkv_colsum", "fc1_colsum", "pos", "cls_pos0")


@functools.lru_cache(maxsize=None)
def _assets(name, depth):
    import synthetic
    data, mean = synthetic.make_smplx_data(seed=0), synthetic.make_mean_params(seed=0)
    return dict(data=data, mean=mean, sd=synthetic.make_state_dict(name, S, seed=42, depth_override=depth, mean_params=mean))


def _cpu_model(name, depth, precision, wlo, lnfold):
    from multi_hmr_amd import Model
    a = _assets(name, depth)
    m = Model(backbone=name, img_size=S, smplx_data=a["data"], mean_params=a["mean"], backbone_depth=depth, precision=precision or "f16",
              wlo=wlo, lnfold=lnfold)
    m.load_state_dict(a["sd"], strict=True)
    return m.eval().train_backbone_(depth).train_embeddings_()


def _pack(m, precision):
    return vit.pack_encoder(m.backbone.encoder, S, precision, torch.device("cpu"), m.wlo, m.lnfold)


def _targets(P):
    """{target: tensor} of EVERY packed encoder tensor of the pack."""
    out = {("norm", n): t for n, t in P["vit"]["norm_t"].items()}
    out.update({("embed", n): t for n, t in P["vit"]["embed_t"].items()})
    for l, bt in enumerate(P["vit"]["block_t"]):
        out.update({("block", l, n): t for n, t in bt.items() if t is not None})
    return out


#: (f16x3 packs f16 operand pairs whatever operand type is asked for: one case)
CASES = [(pack, tdt) for pack in PACKS for tdt in ("f16", "bf16") if (pack, tdt) != ("x3", "bf16")]


@pytest.mark.parametrize("pack,tdt", CASES)
def test_segments_and_jobs_reproduce_the_pack(pack, tdt):
    """The packed encoder of the fixture, then every encoder parameter perturbed; segments and jobs applied in numpy to the OLD packed
    tensors give the pack of the NEW parameters: bit for bit in every copied, cast, [hi | lo] and triple tensor and the f16 column sums,
    within one ulp in the fixed-order fp64 sums.  Every element has one writer; none exactly in the zero padding."""
    name, depth, precision, wlo, lnfold = PACKS[pack]
    precision = precision or tdt
    m = _cpu_model(name, depth, precision, wlo, lnfold)
    old = _pack(m, precision)
    assert old["tdt"] == (torch.float16 if tdt == "f16" else torch.bfloat16)
    segs, jobs = encoder_segments(m, old), encoder_jobs(m, old)
    named = dict(m.named_parameters())
    covered = [s["param"] for s in segs]
    assert sorted(covered) == sorted(n for n in named if n.startswith(ENCODER) and n != ENCODER + "mask_token") and len(set(covered)) == len(covered)
    assert covered == ModelAdam(m)._names[-len(covered):]
    packed = {k: oo.bits(t) for k, t in _targets(old).items()}
    before = {k: v.copy() for k, v in packed.items()}
    g = torch.Generator().manual_seed(13)
    with torch.no_grad():
        for n in covered:
            named[n].add_(torch.randn(named[n].shape, generator=g) * 0.03)
    new = _targets(_pack(m, precision))
    values = {n: named[n].detach().numpy() for n in covered}
    claims = oo.apply_segments([s for s in segs if s["kind"] is not None], values, {}, packed, old["tdt"])
    for k, c in eo.apply_jobs(jobs, values, packed, old["tdt"]).items():
        claims[k] = claims[k] + c
    # completeness: every tensor of block_t / norm_t / embed_t is named by a segment or by a job target
    named_targets = {s["target"] for s in segs if s["kind"] is not None}
    for j in jobs:
        named_targets |= {j[f] for f in (("pos", "cls_pos0") if j["kind"] == "pos" else ("w16", "lo", "bias_out", "colsum")) if j[f] is not None}
    assert named_targets == set(packed)
    Cd, moved, off = old["C"], 0, 0
    for k, t in new.items():
        ref = oo.bits(t)
        field = k[-1]
        if field in FIXED_ORDER and t.dtype == torch.float32 and not (field.endswith("colsum") and tdt == "f16"):
            d = eo.ulp_distance(packed[k].view(np.float32), ref.view(np.float32))
            assert d.max() <= 1, (k, int(d.max()))
            off += int((d > 0).sum())
        else:
            assert np.array_equal(packed[k], ref), k
        moved += int((before[k] != ref).sum())
        assert claims[k].max() <= 1, k
        free = (claims[k] == 0).reshape(t.shape)
        if k == ("embed", "patch_w"):
            cols = np.zeros(t.shape[1], dtype=bool)
            for s0 in range(0, t.shape[1], old["Kp"]):
                cols[s0:s0 + 588] = True
            assert not free[:, cols].any() and free[:, ~cols].all() and not t[:, ~cols].float().any()
        elif old.get("cpad") and t.shape[0] in (old["cpad"], 2 * Cd + old["cpad"]):
            rows = t.shape[0] - (old["cpad"] - Cd)
            assert not free[:rows].any() and free[rows:].all() and not t[rows:].float().any(), k
        else:
            assert not free.any(), k
    assert moved > 100000
    print(f"\n{pack} {tdt}: {off} fixed-order elements one ulp from pack_block's")


def test_jobs_follow_the_pack_choices():
    m = _cpu_model(*PACKS["vitb_fold"][:2], "f16", *PACKS["vitb_fold"][3:])
    P = _pack(m, "f16")
    jobs = encoder_jobs(m, P)
    kinds = [(j["w"].split("blocks.")[1], j["lo_form"], j["ln"] is not None) for j in jobs if j["kind"] == "row"]
    assert kinds == [("0.attn.qkv.weight", "pair", False), ("0.attn.proj.weight", "pair", False), ("0.mlp.fc1.weight", None, True),
                     ("1.attn.qkv.weight", "pair", True), ("1.attn.proj.weight", "pair", False), ("1.mlp.fc1.weight", None, True)]
    assert jobs[-1]["kind"] == "pos" and (jobs[-1]["M"], jobs[-1]["G"]) == (37, 16)
    assert jobs[0]["rows"] == (1536, 768) and jobs[3]["rows"] == (0, 2304) and jobs[3]["lo_rows"] == (1536, 768)
    derived = [s["param"][len(ENCODER):] for s in encoder_segments(m, P) if s["kind"] is None]
    assert derived == ["blocks.0.mlp.fc1.weight", "blocks.0.mlp.fc1.bias", "blocks.1.attn.qkv.weight", "blocks.1.attn.qkv.bias",
                      "blocks.1.mlp.fc1.weight", "blocks.1.mlp.fc1.bias", "pos_embed", "cls_token"]
    for s in encoder_segments(m, P):
        if s["kind"] is not None:
            t, n = packed_target(P, s["target"]), named_numel(m, s["param"])
            assert (n // s["cols"] - 1) * s["pitch"] + s["cols"] <= t.numel() and t.dtype == (torch.float32 if s["kind"] == "f32" else torch.float16)
    # nothing packed: parameters only
    assert m._packed is None and encoder_jobs(m) == [] and all(s["kind"] is None for s in encoder_segments(m))
    m.train_backbone_(1).train_embeddings_(False)
    assert len(encoder_segments(m, P)) == 2 + 14 and [j["w"].split("blocks.")[1][0] for j in encoder_jobs(m, P)] == ["1", "1", "1"]


def named_numel(m, name):
    return dict(m.named_parameters())[name].numel()


@pytest.mark.parametrize("M,G", [(37, 16), (37, 64), (16, 16)])
def test_oracle_position_table_against_numpy(M, G):
    g = np.random.default_rng(5)
    pe = (g.standard_normal((1, 1 + M * M, 24)) * 0.02).astype(np.float32)
    cls = g.standard_normal((1, 1, 24)).astype(np.float32)
    pos, cls0 = eo.pos_job(pe, cls, G)
    ref = packing.interpolate_pos_embed(pe, G)
    d = eo.ulp_distance(pos, ref)
    assert pos.shape == ref.shape == (1 + G * G, 24) and d.max() <= 1
    assert np.array_equal(cls0, cls.reshape(-1) + ref[0])
    if G == M:
        assert d.max() == 0
    print(f"\nM={M} G={G}: {int((d > 0).sum())} of {d.size} elements one ulp from interpolate_pos_embed")


def test_wave_sum_is_a_fixed_order_of_exact_terms():
    g = np.random.default_rng(2)
    x = g.standard_normal((5, 1536))
    s = eo.wave_sum(x)
    assert np.max(np.abs(s - x.sum(1))) <= 1e-12
    ints = g.integers(-1000, 1000, size=(3, 384)).astype(np.float64)
    assert np.array_equal(eo.wave_sum(ints), ints.sum(1))
    assert np.array_equal(eo.wave_sum(np.stack([ints, ints], 2)), 2 * ints.sum(1))


# ------------------------------------------------------------------------------------------------------ ABI
def test_header_and_binding():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    assert "mhmr_vit_repack" in _lib._SIGS and re.search(r"\bint\s+mhmr_vit_repack\s*\(", header)
    assert "encoder_pack.hip" in _lib.SOURCES and "-ffp-contract=off" in _lib.EXTRA_FLAGS["encoder_pack.hip"]
    body = re.search(r"typedef struct \{([^}]*)\} mhmr_pack_job;", header).group(1)
    assert re.findall(r"(\w+)\s*[;,]", body) == [n for n, _ in _lib.PackJob._fields_]
    assert C.sizeof(_lib.PackJob) == 14 * 8 + 14 * 4
    for n in ("ROW", "POS", "LO_NONE", "LO_PAIR", "LO_TRIPLE"):
        assert int(re.search(rf"#define MHMR_PACK_{n} (\d+)", header).group(1)) == getattr(_lib, "PACK_" + n)
    for cited in ("vit.pack_block", "packing.interpolate_pos_embed", "train.py:304"):
        assert cited in header


def _row(**kw):
    """A valid row job over fake (never dereferenced) device addresses."""
    j = _lib.PackJob()
    j.kind, j.dtype, j.N, j.K, j.pitch16 = _lib.PACK_ROW, _lib.ADAM_PACK_F16, 8, 64, 64
    j.w, j.w16 = 0x10000, 0x20000
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _pos(**kw):
    j = _lib.PackJob()
    j.kind, j.M, j.G, j.C = _lib.PACK_POS, 37, 16, 64
    j.pos_embed, j.cls_token, j.tap_w, j.tap_i, j.pos, j.cls_pos0 = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _call(jobs, njobs=None, dev=0x9000):
    _lib.build()
    arr = (_lib.PackJob * max(len(jobs), 1))(*jobs)
    return _lib.lib().mhmr_vit_repack(arr, dev, len(jobs) if njobs is None else njobs, None)


def test_bad_arguments_are_refused_before_any_launch():
    """Every call here must return before the first launch: there is no GPU under this test."""
    ARG, SHAPE = -1, -2
    assert _call([], njobs=0) == 0 and _call([], njobs=-1) == ARG
    assert _call([_row()], dev=None) == ARG and _lib.lib().mhmr_vit_repack(None, 0x9000, 1, None) == ARG
    lo = dict(lo=0x30000, lo_form=_lib.PACK_LO_PAIR, lo_rows=8, lo_section=64, lo_pitch=128)
    fold = dict(ln_w=0x40000, ln_b=0x41000, bias=0x42000, bias_out=0x43000, colsum=0x44000)
    for kw in (dict(w=None), dict(dtype=_lib.ADAM_PACK_F32), dict(kind=2), dict(ln_w=0x40000), dict(ln_b=0x40000), dict(bias_out=0x43000),
               dict(fold, bias=None), dict(lo_form=_lib.PACK_LO_PAIR), dict(lo=0x30000), dict(lo_form=3, lo=0x30000), dict(w16=None), dict(row0=1),
               dict(lo, lo=0x20000 + 64), dict(fold, colsum=0x43000 + 16), dict(fold, bias_out=0x20000)):
        assert _call([_row(**kw)]) == ARG, kw
    for kw in (dict(N=0), dict(K=0), dict(K=62), dict(pitch16=60), dict(lo, lo_rows=9), dict(lo, lo_row0=-1), dict(lo, lo_section=60),
               dict(lo, lo_pitch=120), dict(lo, lo_form=_lib.PACK_LO_TRIPLE)):
        assert _call([_row(**kw)]) == SHAPE, kw
    for kw in (dict(pos=None), dict(cls_pos0=None), dict(pos_embed=None), dict(cls_token=None), dict(tap_w=None), dict(tap_i=None), dict(row0=3),
               dict(cls_pos0=0x500000 + 4 * 64)):
        assert _call([_pos(**kw)]) == ARG, kw
    for kw in (dict(M=0), dict(G=0), dict(C=0)):
        assert _call([_pos(**kw)]) == SHAPE, kw
    assert _call([_pos(), _row()]) == ARG                                    # the row jobs come first
    assert _call([_row(), _row(row0=8)]) == ARG                              # the same target twice
    assert _call([_row(), _row(row0=4, w16=0x80000)]) == ARG                 # a wrong first row


def test_model_adam_refusals_and_state_dict():
    m = _cpu_model(*PACKS["vits"][:2], "f16", None, None)
    for kw in (dict(weight_decay=0.01), dict(amsgrad=True), dict(maximize=True), dict(lr=-1.0), dict(max_grad_norm=0.0)):
        with pytest.raises(ValueError):
            ModelAdam(m, **kw)
    opt = ModelAdam(m, lr=1e-4)
    params = m.heads_parameters() + m.detection_parameters() + m.backbone_parameters(2) + m.embedding_parameters()
    assert len(opt.param_groups[0]["params"]) == len(params) and all(a is b for a, b in zip(opt.param_groups[0]["params"], params))
    with pytest.raises(_lib.MhmrError, match="CPU"):
        opt.step()
    a = torch.optim.Adam(params, lr=1e-4)
    a.load_state_dict(opt.state_dict())
    opt.load_state_dict(a.state_dict())
    assert opt.param_groups[0]["lr"] == 1e-4
    m.train_backbone_(1)
    with pytest.raises(_lib.MhmrError, match="make a new one"):
        opt._specs(None)


def test_command_line_makes_model_adam(smplx_data, mean_params):
    from multi_hmr_amd import HeadsAdam, Model, train
    new = lambda: Model(backbone="dinov2_vits14", img_size=224, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=3).train_heads_(True)
    p = train.build_parser()
    opt = train.make_optimizer(new(), p.parse_args(["--pretrained", "x", "--fused_adam", "1", "--train_backbone", "2", "--max_grad_norm", "0.5"]))
    assert type(opt) is ModelAdam and opt.max_grad_norm == 0.5 and opt.model._backbone_n == 2
    assert type(train.make_optimizer(new(), p.parse_args(["--pretrained", "x", "--train_backbone", "2"]))) is torch.optim.Adam
    for argv in ([], ["--fused_adam", "1"]):
        assert type(train.make_optimizer(new(), p.parse_args(["--pretrained", "x"] + argv))) is HeadsAdam
    with pytest.raises(SystemExit):
        p.parse_args(["--pretrained", "x", "--fused_adam", "2"])
