"""Host tests of tests/vit_forms.py (no GPU): the two references are what they claim to be, and the Python-side prediction of every case's
form is the form the case table asks for (tests/test_gpu_vit_forms.py compares mhmr_vit_form_bits itself against the same prediction)."""
import os
import re

import pytest
import torch

import parity
import vit_forms as vf
from multi_hmr_amd import _lib, vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = "dinov2_vits14"


def test_form_bit_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    for i, name in enumerate(_lib.VIT_FORM_BITS):
        m = re.search(rf"#define\s+MHMR_VIT_FORM_{name.upper()}\s+0x([0-9a-fA-F]+)u", header)
        assert m and int(m.group(1), 16) == 1 << i, name
    assert len(re.findall(r"#define\s+MHMR_VIT_FORM_", header)) == len(_lib.VIT_FORM_BITS)
    assert "mhmr_vit_form_bits" in _lib.EXPORTS


def test_fp64_stream_is_the_oracles_own_output():
    enc, x = vf.make_encoder(SMALL), vf.make_images(2)
    stream, feats = vf.fp64_stream(enc, x)
    import copy
    with torch.no_grad():
        ref = copy.deepcopy(enc).double().get_intermediate_layers(x.double())[0]
    assert len(stream) == len(feats) == vf.DEPTH + 1 and stream[0].shape == (2, 257, 384) and feats[-1].shape == (2, 256, 384)
    assert float(vf.row_errors(feats[-1], ref).max()) <= 1e-12
    # row order of the kernels: the class token (the same in every image before block 0, up to the position embedding) is row N
    assert torch.equal(stream[0][0, 256], stream[0][1, 256]) and not torch.equal(stream[0][0, 0], stream[0][1, 0])


@pytest.mark.parametrize("fold,wlo", [(False, {}), (True, {0: ["v", "proj"], 1: ["v"]})])
def test_rounding_model_is_the_truth_in_fp64_and_strictly_worse_in_f16(fold, wlo):
    enc, x = vf.make_encoder(SMALL), vf.make_images(2)
    stream, feats = vf.truth(SMALL, 2)
    m64 = vf.rounding_model(enc, x, torch.float64, fold=fold, wlo=wlo)
    m16 = vf.rounding_model(enc, x, torch.float16, fold=fold, wlo=wlo)
    for l in range(vf.DEPTH + 1):
        assert float(vf.row_errors(m64[0][l], stream[l]).max()) <= 1e-12, l
        assert float(vf.row_errors(m64[1][l], feats[l]).max()) <= 1e-12, l
        e16 = vf.worst_rows(m16[0][l], stream[l], 256)["all"]["e"]
        assert 1e-6 < e16 < parity.TOL["f16"], (l, e16)          # worse than fp64, and a bound of GATE x this is not vacuous
    # the low halves buy accuracy in the model as they do in the kernels
    if wlo:
        none = vf.rounding_model(enc, x, torch.float16, fold=fold, wlo={})
        assert vf.row_errors(m16[0][1], stream[1]).mean() < vf.row_errors(none[0][1], stream[1]).mean()


def test_worst_rows_names_image_and_row():
    ref = torch.ones(2, 5, 8, dtype=torch.float64)
    got = ref.clone()
    got[1, 2] += 0.5
    got[0, 4] += 0.25
    w = vf.worst_rows(got, ref, 4)
    assert (w["all"]["image"], w["all"]["row"]) == (1, 2) and (w["patch"]["image"], w["patch"]["row"]) == (1, 2)
    assert (w["cls"]["image"], w["cls"]["row"]) == (0, 4) and abs(w["cls"]["e"] - 0.25) < 1e-12
    assert vf.gate(1e-4, "f16") == 4e-4 and vf.gate(1.0, "f16") == 4e-3 and vf.gate(0.0, "f16x3") == 4e-5 and vf.gate(1.0, "bf16") == 8e-2


@pytest.mark.parametrize("precision,name", [("f16", n) for n in vf.CASES] + [("bf16", n) for n in vf.BF16_CASES])
def test_predicted_form_of_every_case_is_the_form_the_table_asks_for(name, precision, monkeypatch):
    for k, v in vf.case_env(name).items():
        monkeypatch.setenv(k, v) if v is not None else monkeypatch.delenv(k, raising=False)
    for k in ("MHMR_ROWMAP", "MHMR_LNFOLD", "MHMR_GEMM128", "MHMR_LNFOLD_ALLROWS"):
        monkeypatch.delenv(k, raising=False)
    P = vf.pack_case(name, precision, device="cpu")
    B = vf.case_batch(name, 256)
    names = vf.predict_bits(P, B, name, 256)
    vf.check_want(names, vf.CASES[name]["want"], name)
    assert vf.case_tokens(P, B, name) == {"plain128": 384, "f16x3": 384}.get(name, 320 if "rowmap" in names else 512)
    if name == "allrows_fc1map":
        assert B == 11 and vit.tiny_batch(P, B)
        # one image fewer: all rows of fc1 fit the chip; the class-row launch of fc1 would not run
        assert "fc1map" not in vf.predict_bits(P, B - 1, name, 256)
        assert vf.fc1map_batch(304) == 13 and vf.fc1map_batch(128) == 6
    if name.startswith("allrows_splitk_merge"):
        assert P["wlo"] == {0: ["proj", "v"]}                    # block 0: Q | K and V; blocks 1, 2: the merged launch


def test_splitk_plan_mirror():
    # csrc/gemm.hip mhmr_splitk_plan on 256 CUs: one ViT-B image over all rows (2 x 3 tiles)
    assert vf.splitk_slices(512, 768, 768, 256) == 3 and vf.splitk_slices(512, 768, 3072, 256) == 8
    assert vf.splitk_slices(512, 768, 768, 4) == 0 and vf.splitk_slices(320, 768, 768, 256) == 0
