"""-m gpu: mhmr_vit_forward form by form (tests/vit_forms.py has the case table, the fp64 truth, the rounding model and the harness).

Every test asserts the bits of mhmr_vit_form_bits before it compares anything: a test that meant to run fc1map and got the fallback fails.
A  every block's residual rows (class row included) and the features, row by row, against fp64: the worst row within GATE x the worst row
   of the rounding model at the same place, and within GATE x parity.TOL;
B  images do not leak into each other and every image offset is right: reversed and identical-image batches, bit for bit;
C  a used workspace is as good as a new one; no NaN / Inf anywhere; the padding rows nobody writes stay zero;
D  ctx16 with a wider pitch: the 16-bit copy of feat32 and nothing else;
E  the token-row-map and the all-rows form agree within the sum of their bounds;
and MHMR_ANYORDER=0 against 1 in child processes.

Measured (MI355X, 256 CUs; profiles/vit_forms.txt has every case, depth and place): the kernels' worst row is 0.92 ... 1.10 x the rounding
model's in every f16 and bf16 case; the whole file takes 30 s, of which the four child-process tests take 22.
"""
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

import parity  # noqa: E402
import vit_forms as vf  # noqa: E402
from multi_hmr_amd import _lib, vit  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#: where check A leaves its figures (pytest -q hides prints): vit_forms.json in the directory MHMR_REPORT_DIR names, else in the temp directory
TABLE_PATH = os.path.join(os.environ.get("MHMR_REPORT_DIR") or tempfile.gettempdir(), "vit_forms.json")
PARAMS = [("f16", n) for n in vf.CASES] + [("bf16", n) for n in vf.BF16_CASES]
cases = pytest.mark.parametrize("precision,name", PARAMS)

_PACKS = {}      # (case, precision) -> (pack, workspace cache): packed once, shared by the tests of the case
_TABLE = {}      # "case/precision" -> rows of profiles/vit_forms.txt


def setup(name, precision, monkeypatch):
    """The case's switches into the environment; -> (pack, batch, workspace cache)"""
    for k, v in vf.case_env(name).items():
        monkeypatch.setenv(k, v) if v is not None else monkeypatch.delenv(k, raising=False)
    if (name, precision) not in _PACKS:
        _PACKS[name, precision] = (vf.pack_case(name, precision), vit.WorkspaceCache())
    P, cache = _PACKS[name, precision]
    return P, vf.case_batch(name, vf.cu_count()), cache


def run_case(*a, **k):
    """vf.run_case; a HIP error ends the session: nothing more is started on a device that has faulted"""
    try:
        return vf.run_case(*a, **k)
    except Exception as e:
        if "hipError" in str(e) or "HIP error" in str(e):
            pytest.exit(f"GPU error, nothing more runs: {e}", returncode=3)
        raise


def check_form(out, P, B, name):
    """the form that ran is the form the case is about, and the form the Python side predicts"""
    vf.check_want(out["bits"], vf.CASES[name]["want"], name)
    assert out["bits"] - {"ao"} == vf.predict_bits(P, B, name, vf.cu_count()), (name, sorted(out["bits"]))
    # ... and the form the library plans for this pack and batch, when the case runs the workspace as planned
    if not vf.CASES[name].get("null") and not vf.CASES[name].get("tp_all_rows"):
        assert out["bits"] - {"ao"} == vf.bit_names(vit.plan(P, B).form_bits), (name, sorted(out["bits"]))


def same_rows(a, b, where):
    assert torch.equal(a, b), (where, "differs in", int((a != b).any(-1).sum()), "rows; first", (a != b).any(-1).nonzero()[:1].tolist())


@cases
def test_every_block_row_by_row_against_fp64(name, precision, monkeypatch):
    """A.  desc.L = 0 (the patch embedding alone) ... 3 on the same pack."""
    P, B, cache = setup(name, precision, monkeypatch)
    prec = vf.case_precision(name, precision)
    backbone = vf.CASES[name]["backbone"]
    x = vf.make_images(B)
    stream, feats = vf.truth(backbone, B)
    mstream, mfeats, mtaps = vf.model_of(backbone, B, prec, P["fold"], P["wlo"])
    taps = vf.truth_taps(backbone, B)
    N, T = P["N"], P["T"]
    rows, late = [], []
    for L in range(vf.DEPTH + 1):
        out = run_case(name, P, B, x, cache, L=L)
        check_form(out, P, B, name)
        places = [("resid", out["resid"][:, :T].cpu(), stream[L], mstream[L]), ("feat32", out["feat32"].cpu(), feats[L], mfeats[L])]
        if L > 0 and "qk" in out["ws"]:
            # what the attention of the last block read: the class row's Q | K | V, and every V^T column, have no other witness this close
            got = vf.attention_operands(out["ws"], P, B)
            places += [(f"block{L - 1}.{n}", got[n].cpu(), taps[L - 1][n], mtaps[L - 1][n]) for n in ("q", "k", "v")]
        for what, got, ref, mod in places:
            k, m = vf.worst_rows(got, ref, N), vf.worst_rows(mod, ref, N)
            bound = vf.gate(m["all"]["e"], prec)
            rows.append(dict(L=L, what=what, kernel=k, model=m, ratio=k["all"]["e"] / max(m["all"]["e"], 1e-300), bound=bound))
            print(f"[vit_forms {name} {precision}] L={L} {what}: kernel {k['all']['e']:.3e} (image {k['all']['image']}, row {k['all']['row']})"
                  f" model {m['all']['e']:.3e} ratio {rows[-1]['ratio']:.2f} bound {bound:.3e}")
            # the bound is not vacuous: correct 16-bit arithmetic is well inside the contract at this place
            assert m["all"]["e"] < parity.TOL["f16" if prec == "f16x3" else prec], (name, L, what, m["all"])
            if not k["all"]["e"] <= bound:
                late.append((L, what, k["all"], m["all"]["e"], bound))
    _TABLE[f"{name}/{precision}"] = dict(form=sorted(out["bits"]), B=B, Tp=out["Tp"], rows=rows)
    os.makedirs(os.path.dirname(TABLE_PATH), exist_ok=True)
    with open(TABLE_PATH, "w") as f:
        json.dump(_TABLE, f, indent=1)
    assert not late, (name, precision, late)


@cases
def test_images_do_not_leak_and_offsets_are_right(name, precision, monkeypatch):
    """B.  Batch against reversed batch, identical images against image 0, and a batch of one against slot 0 of a batch of two."""
    P, B, cache = setup(name, precision, monkeypatch)
    T = P["T"]

    def reversed_and_identical(B, x):
        a = run_case(name, P, B, x, cache)
        b = run_case(name, P, B, x.flip(0).contiguous(), cache)
        same = run_case(name, P, B, x[:1].expand(B, -1, -1, -1).contiguous(), cache)
        assert a["bits"] == b["bits"] == same["bits"]
        for i in range(B):
            same_rows(a["feat32"][i], b["feat32"][B - 1 - i], (name, "feat32 of image", i, "reversed"))
            same_rows(a["resid"][i, :T], b["resid"][B - 1 - i, :T], (name, "resid of image", i, "reversed"))
            same_rows(same["feat32"][i], same["feat32"][0], (name, "feat32 of identical image", i))
            same_rows(same["resid"][i, :T], same["resid"][0, :T], (name, "resid of identical image", i))
        return a, same

    a, same = reversed_and_identical(B, vf.make_images(B))
    check_form(a, P, B, name)
    # the images are different: the comparison above is not between equal things
    if B > 1:
        assert not torch.equal(a["feat32"][0], a["feat32"][1])
    if B == 1:
        x2 = vf.make_images(2)
        a2, same2 = reversed_and_identical(2, x2)
        if a2["bits"] == a["bits"]:
            lib, Cd = _lib.lib(), P["C"]
            slices = lambda M: [lib.mhmr_splitk_workspace_bytes(M, Cd, K) // (4 * M * Cd) for K in (Cd, 2 * Cd, 4 * Cd)]
            if "splitk" not in a["bits"] or slices(a["Tp"]) == slices(2 * a2["Tp"]):     # the same summation order for every row
                same_rows(a["feat32"][0], same2["feat32"][0], (name, "feat32: batch of one against slot 0 of two"))
                same_rows(a["resid"][0, :T], same2["resid"][0, :T], (name, "resid: batch of one against slot 0 of two"))


@cases
def test_used_workspace_is_as_good_as_new_and_ctx16_is_exact(name, precision, monkeypatch):
    """C and D.  x, another batch, x again in one workspace; ctx16 with ldctx = C + 64 into a buffer full of a sentinel."""
    P, B, cache = setup(name, precision, monkeypatch)
    N, T, Cd = P["N"], P["T"], P["C"]
    x, y = vf.make_images(B), vf.make_images(B, seed=5)
    outs = []
    for inp in (x, y, x):
        o = run_case(name, P, B, inp, cache)
        outs.append(o)
        ws, Tp = o["ws"], o["Tp"]
        for buf in ("resid", "att", "hid", "xn"):
            assert bool(torch.isfinite(ws[buf].float()).all()), (name, buf, "holds NaN / Inf")
        if name in vf.PADDING_STAYS:
            att, hid = ws["att"].view(B, Tp, -1), ws["hid"].view(B, Tp, -1)
            # attention stores whole 16-row blocks: the class row's block reaches row N + 15; fc1's class-row launch writes row N alone
            assert not bool(att[:, N + 16:].any()) and not bool(hid[:, N + 1:].any()), (name, "padding rows of att / hid were written")
        # D: columns [0, C) of rows < B * N are the 16-bit copy of feat32; everything else keeps the sentinel
        ctx = o["ctx16"]
        want = o["feat32"].reshape(B * N, Cd).to(P["tdt"])
        differ = ctx[:B * N, :Cd] != want
        if bool(differ.any()):
            print(f"[vit_forms {name} {precision}] ctx16 != op16(feat32) in {int(differ.sum())} of {differ.numel()} elements, "
                  f"largest difference {float((ctx[:B * N, :Cd].float() - want.float()).abs().max()):.3e}")
        assert torch.equal(ctx[:B * N, :Cd], want), (name, "ctx16 is not the 16-bit copy of feat32")
        assert bool((ctx[:B * N, Cd:] == vf.SENTINEL).all()) and bool((ctx[B * N:] == vf.SENTINEL).all()), (name, "ctx16 written outside its columns / rows")
    check_form(outs[0], P, B, name)
    assert not torch.equal(outs[0]["feat32"], outs[1]["feat32"])
    same_rows(outs[0]["feat32"], outs[2]["feat32"], (name, "feat32 after another batch went through the workspace"))
    same_rows(outs[0]["resid"][:, :T], outs[2]["resid"][:, :T], (name, "resid after another batch went through the workspace"))


def test_token_row_map_and_all_rows_forms_agree(monkeypatch):
    """E.  The same image and weights through the token-row map (image 0 of three) and through all rows (a batch of one) differ in
    summation order only: per row, within the sum of the two bounds of A.  A sanity assertion: no new bound."""
    res, bound = {}, 0.0
    stream, feats = vf.truth("dinov2_vitb14", 1)
    for name in ("rowmap_fold_cst", "allrows_fold_unsplit"):
        P, B, cache = setup(name, "f16", monkeypatch)
        out = run_case(name, P, B, vf.make_images(B), cache)
        check_form(out, P, B, name)
        res[name] = out
        m = vf.model_of("dinov2_vitb14", B, "f16", P["fold"], P["wlo"])[:2]
        ref = vf.truth("dinov2_vitb14", B)
        bound += vf.gate(vf.worst_rows(m[0][-1], ref[0][-1], P["N"])["all"]["e"], "f16")
        T = P["T"]
    a, b = res["rowmap_fold_cst"], res["allrows_fold_unsplit"]
    assert "rowmap" in a["bits"] and "allrows256" in b["bits"]
    d_resid = (a["resid"][0, :T].double() - b["resid"][0, :T].double()).norm(dim=-1).cpu() / stream[-1][0].norm(dim=-1)
    d_feat = (a["feat32"][0].double() - b["feat32"][0].double()).norm(dim=-1).cpu() / feats[-1][0].norm(dim=-1)
    print(f"[vit_forms cross-form] resid {float(d_resid.max()):.3e} feat32 {float(d_feat.max()):.3e} bound {bound:.3e}")
    assert float(d_resid.max()) <= bound and float(d_feat.max()) <= bound, (float(d_resid.max()), float(d_feat.max()), bound)


@pytest.mark.parametrize("name", vf.ANYORDER_CASES)
def test_any_order_launches_change_no_bit(name, tmp_path):
    """MHMR_ANYORDER=0 against 1, each in a fresh process (C++ reads the switch once), one child at a time: three forwards inside each child
    bit-equal, and the two children bit-equal to each other.  A child that fails or times out ends the test there."""
    got = {}
    for ao in ("0", "1"):
        out = str(tmp_path / f"ao{ao}.pt")
        env = dict(os.environ, MHMR_ANYORDER=ao)
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vit_forms_child.py"), name, out], env=env, timeout=120,
                             capture_output=True, text=True)
        assert res.returncode == 0, (name, ao, res.returncode, res.stdout[-2000:], res.stderr[-2000:])
        got[ao] = torch.load(out)
        assert ("ao" in got[ao]["bits"]) == (ao == "1"), (name, ao, got[ao]["bits"])
        for key in ("feat32", "resid"):
            for i in (1, 2):
                same_rows(got[ao][key][0], got[ao][key][i], (name, key, "forward", i, "MHMR_ANYORDER=" + ao))
    assert set(got["0"]["bits"]) ^ set(got["1"]["bits"]) == {"ao"}
    for key in ("feat32", "resid"):
        same_rows(got["0"][key][0], got["1"][key][0], (name, key, "MHMR_ANYORDER=0 against 1"))
