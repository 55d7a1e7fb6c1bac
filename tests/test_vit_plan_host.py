"""-m "not gpu": ``mhmr_vit_plan`` (csrc/vit_plan.h, the one statement of the ViT forward's layout rule) against the rule as
multi_hmr_amd/vit.py used to state it (tests/vit_plan_oracle.py), field by field over a grid of packs, batches and switches, planned for
256 compute units -- integer arithmetic, no device."""
import ctypes as C
import itertools
import os
import re

import pytest

import vit_plan_oracle as oracle
from multi_hmr_amd import _lib, vit
from multi_hmr_amd.packing import roundup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCU = 256
WIDTHS = (384, 768, 1024, 1280, 1536)
GRIDS = (16, 37, 48, 64, 92)
BATCHES = (1, 2, 3, 4, 6, 8, 11, 16, 32, 128, 512)
#: the environment's default, every switch flipped alone (each default-on switch off, the two opt-in ones on), and everything on
MASKS = [_lib.PLAN_DEFAULT] + [_lib.PLAN_DEFAULT ^ bit for bit in _lib.PLAN.values()] + [sum(_lib.PLAN.values())]
BIT = {n: 1 << i for i, n in enumerate(_lib.VIT_FORM_BITS)}


def packs(Cd: int, G: int):
    """Every (fold, lo8, x3, cpad) vit.pack_encoder can leave in a pack of this width: f16x3 has none of the others; lnfold=True / False can
    force the fold either way; cpad follows fold for a width that is no multiple of 256; fp8 rows only for a multiple of 256."""
    base = {"C": Cd, "H": Cd // 64, "N": G * G, "T": G * G + 1}
    yield dict(base, x3=True, fold=False)
    for fold, lo8 in itertools.product((False, True), (False, True) if Cd % 256 == 0 else (False,)):
        yield dict(base, x3=False, fold=fold, lo8=lo8, cpad=roundup(Cd, 256) if (fold and Cd % 256) else 0)


def _struct_fields(header, name):
    end = header.index("} " + name + ";")
    body = header[header.rindex("typedef struct {", 0, end):end]
    return re.findall(r"[\*\s,]([A-Za-z_0-9]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_header_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    assert _struct_fields(header, "mhmr_vit_plan_request") == [f[0] for f in _lib.VitPlanRequest._fields_]
    assert _struct_fields(header, "mhmr_vit_plan_result") == [f[0] for f in _lib.VitPlan._fields_]
    for name, bit in _lib.PLAN.items():
        m = re.search(rf"#define\s+MHMR_PLAN_{name.upper()}\s+0x([0-9a-fA-F]+)u", header)
        assert m and int(m.group(1), 16) == bit, name
    assert int(re.search(r"#define\s+MHMR_PLAN_DEFAULT\s+0x([0-9a-fA-F]+)u", header).group(1), 16) == _lib.PLAN_DEFAULT
    assert len(re.findall(r"#define\s+MHMR_PLAN_", header)) == len(_lib.PLAN) + 1
    assert "#define MHMR_VERSION 106" in header and "mhmr_vit_plan" in _lib.EXPORTS            # additive


def test_environment_to_switch_mask(monkeypatch):
    names = ("MHMR_ROWMAP", "MHMR_GEMM128", "MHMR_TINY_ALLROWS", "MHMR_LNFOLD", "MHMR_LNFOLD_ALLROWS", "MHMR_VITS_256", "MHMR_LO8")
    for n in names:
        monkeypatch.delenv(n, raising=False)
    assert vit.switches() == _lib.PLAN_DEFAULT
    for n, value, flipped in [("MHMR_ROWMAP", "0", "rowmap"), ("MHMR_GEMM128", "1", "gemm128"), ("MHMR_TINY_ALLROWS", "0", "tiny_allrows"),
                              ("MHMR_LNFOLD", "0", "lnfold"), ("MHMR_LNFOLD_ALLROWS", "0", "lnfold_allrows"), ("MHMR_VITS_256", "1", "vits_256"),
                              ("MHMR_LO8", "1", "lo8")]:
        monkeypatch.setenv(n, value)
        assert vit.switches() == _lib.PLAN_DEFAULT ^ _lib.PLAN[flipped], n
        monkeypatch.delenv(n)
    monkeypatch.setenv("MHMR_LO8", "0")               # the packer's meaning: opt-in
    assert vit.switches() == _lib.PLAN_DEFAULT


def test_plan_equals_the_former_python_rule_in_every_field():
    _lib.build()
    n = 0
    for Cd, G, mask in itertools.product(WIDTHS, GRIDS, MASKS):
        sw = oracle.switches(mask)
        for P in packs(Cd, G):
            elig = dict(fold_eligible=int(oracle.fold_eligible(Cd, P["N"], sw)), lo8_eligible=int(oracle.lo8_eligible(Cd, sw)))
            zero = vit.plan(P, 0, ncu=NCU, sw=mask)                 # B = 0: the pack-time question
            assert {k: getattr(zero, k) for k in elig} == elig, (Cd, G, hex(mask), P)
            for B in BATCHES:
                want = dict(oracle.workspaces(P, B, sw, NCU), tiny_batch=int(oracle.tiny_batch(P, B)), **elig)
                pl = vit.plan(P, B, ncu=NCU, sw=mask)
                got = {k: getattr(pl, k) for k in want}
                assert got == want, (Cd, G, B, hex(mask), P, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
                assert bool(pl.form_bits & BIT["rowmap"]) == bool(pl.row_map), (Cd, G, B, hex(mask), P)
                assert not (pl.form_bits & BIT["splitk"]) or pl.splitk_bytes > 0, (Cd, G, B, hex(mask), P)
                assert not pl.form_bits & BIT["ao"] and bool(pl.form_bits & BIT["x3"]) == bool(P["x3"])
                n += 1
    assert n == len(GRIDS) * len(MASKS) * len(BATCHES) * (3 + 4 * 5)          # three packs of ViT-S, five of every other width


def test_plan_rejects_what_it_cannot_plan():
    _lib.build()
    lib, out = _lib.lib(), _lib.VitPlan()
    rq = lambda **k: C.byref(_lib.VitPlanRequest(**dict(dict(C=768, H=12, N=256, B=1, switches=_lib.PLAN_DEFAULT, ncu=NCU), **k)))
    assert lib.mhmr_vit_plan(rq(), C.byref(out)) == 0 and out.Tp == 320 and out.row_map == 1
    assert lib.mhmr_vit_plan(None, C.byref(out)) == lib.mhmr_vit_plan(rq(), None) == -1
    assert lib.mhmr_vit_plan(rq(H=11), C.byref(out)) == lib.mhmr_vit_plan(rq(B=-1), C.byref(out)) == lib.mhmr_vit_plan(rq(N=0), C.byref(out)) == -1
    assert lib.mhmr_vit_plan(rq(ncu=-1), C.byref(out)) == -1
    assert lib.mhmr_vit_plan(rq(C=384, H=6, lo8=1), C.byref(out)) == -2
    # one ViT-B image at 224^2 with folded LayerNorms is a tiny batch: all rows, split-k (tests/test_vit_forms_host.py: 8 slices at K = 4C)
    assert lib.mhmr_vit_plan(rq(fold=1), C.byref(out)) == 0
    assert (out.Tp, out.row_map, out.tiny_batch, out.splitk_bytes, out.need_v16) == (512, 0, 1, 8 * 512 * 768 * 4, 1)
    assert {n for n, b in BIT.items() if out.form_bits & b} == {"allrows256", "fold", "splitk", "qkv_merge"}
