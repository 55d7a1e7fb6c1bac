"""-m "not gpu": the training loss's host side -- header / binding / version agree, both C entries validate before any launch (so
they run without a GPU), the stored record of the reference's own loss agrees with the fp64 statement of tests/loss_oracle.py within
the reference's fp32 error, and the drop-in class keeps the reference's argument defaults."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest

import loss_oracle as lo
from multi_hmr_amd import Loss, _lib, loss_and_grads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loss_ref.npz")


def test_loss_entries_are_declared_bound_and_additive():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    ours = {"mhmr_loss_forward", "mhmr_loss_backward", "mhmr_loss_workspace_bytes"}
    assert ours <= declared and ours <= set(_lib._SIGS)
    assert "#define MHMR_VERSION 106" in header and _lib.VERSION == 106            # additive entries: the version stays
    assert int(re.search(r"#define MHMR_LOSS_OUT_BYTES (\d+)", header).group(1)) == _lib.LOSS_OUT_BYTES
    assert "loss.hip" in _lib.SOURCES and "-ffp-contract=off" in _lib.EXTRA_FLAGS["loss.hip"]
    # the ctypes structs mirror the header's field order
    body = header[header.index("typedef struct {\n    const float *scores_hat"):header.index("} mhmr_loss_desc;")]
    names = re.findall(r"[\*\s,]([A-Za-z_0-9]+)(?:\[10\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in _lib.LossDesc._fields_], names
    _lib.build()
    lib = _lib.lib()
    assert lib.mhmr_version() == 106 and lib.mhmr_loss_workspace_bytes() > 0 and lib.mhmr_loss_workspace_bytes() % 8 == 0


def _desc(**over):
    """A descriptor whose pointers are non-null but never dereferenced: validation comes before any launch."""
    d = _lib.LossDesc()
    for n in _lib.LossDesc.TENSORS:
        setattr(d, n + "_hat", 64)
        setattr(d, n, 64)
    d.B, d.G, d.P, d.V, d.J, d.nrot, d.nb_hat, d.nb_gt, d.img_size, d.use_2d = 2, 5, 3, 10475, 127, 477, 10, 11, 224.0, 1
    for k, v in over.items():
        setattr(d, k, v)
    return d


BAD = [dict(V=0), dict(J=0), dict(nb_hat=0), dict(nb_gt=0), dict(P=-1), dict(G=0), dict(B=0), dict(nrot=0), dict(scores_hat=None), dict(scores=None),
       dict(v3d_hat=None), dict(v3d=None), dict(pelvis=None), dict(shape_hat=None), dict(P=1 << 20, V=1 << 12)]


@pytest.mark.parametrize("over", BAD, ids=lambda o: ",".join(o))
def test_loss_entries_reject_invalid_descriptions_before_any_launch(over):
    _lib.build()
    lib = _lib.lib()
    d = _desc(**over)
    g = _lib.LossGrads()
    assert lib.mhmr_loss_forward(C.byref(d), 64, 1 << 20, 64, None) == -1
    assert lib.mhmr_loss_backward(C.byref(d), 64, 64, C.byref(g), None) == -1


def test_loss_entries_reject_null_arguments_before_any_launch():
    _lib.build()
    lib = _lib.lib()
    d, g = _desc(), _lib.LossGrads()
    need = lib.mhmr_loss_workspace_bytes()
    assert lib.mhmr_loss_forward(None, 64, need, 64, None) == -1
    assert lib.mhmr_loss_forward(C.byref(d), None, need, 64, None) == -1
    assert lib.mhmr_loss_forward(C.byref(d), 64, need, None, None) == -1
    assert lib.mhmr_loss_forward(C.byref(d), 64, need - 8, 64, None) == -1
    assert lib.mhmr_loss_backward(None, 64, 64, C.byref(g), None) == -1
    assert lib.mhmr_loss_backward(C.byref(d), None, 64, C.byref(g), None) == -1
    assert lib.mhmr_loss_backward(C.byref(d), 64, None, C.byref(g), None) == -1
    assert lib.mhmr_loss_backward(C.byref(d), 64, 64, None, None) == -1


def test_golden_record_of_the_reference_agrees_with_the_fp64_statement():
    z = np.load(GOLDEN)
    case = dict(zip(z["case_keys"].tolist(), z["case_values"].tolist()))
    ints = {k: int(case[k]) for k in ("seed", "P", "V", "J", "B", "G", "nb_hat", "nb_gt")}
    assert (ints["P"], ints["V"], ints["J"], ints["B"], ints["G"]) == (7, 10475, 127, 2, 5) and int(case["epoch"]) == lo.DEFAULTS["start_2d_epoch"]
    h, y = lo.make_inputs(ints["seed"], ints["P"], ints["V"], ints["J"], ints["B"], ints["G"], ints["nb_hat"], ints["nb_gt"], case["img_size"])
    args = lo.default_args()
    res = lo.loss_ref(h, y, int(case["epoch"]), case["img_size"], args)
    bound, typical = lo.reference_fp32_bound(h, y, res, args), lo.reference_fp32_bound(h, y, res, args, typical=True)
    assert z["value_keys"].tolist() == list(lo.KEYS)
    for k, v in zip(lo.KEYS, z["values"].astype(np.float64)):
        err = abs(v - res["values"][k])
        print(f"{k:7s} reference {v:.9g} fp64 {res['values'][k]:.12g} |diff| {err:.3g} fp32 bound {bound[k]:.3g} (+ storage {abs(v) * lo.U:.3g})")
        assert err <= bound[k] + abs(v) * lo.U, k
        assert err <= typical[k] + abs(v) * lo.U, (k, typical[k])   # ... and within eight standard deviations of independent roundings
    # the gradients the reference's autograd recorded: every stored slice against the oracle's elements.  The reference scales in fp32
    # (1/P, 1/V, alpha, the total's chain: <= 6 roundings) -> 8 * 2^-24 relative; the pelvis gradient is an fp32 SUM of V + J signed
    # constants in torch's order: (V + J) 2^-24 times the sum of their magnitudes, which is at most (alpha_j3d + alpha_v3d) / P
    for k, g in res["grads"].items():
        sl = z["gslice_" + k].astype(np.float64)
        ref = g.reshape(-1)[: sl.size]
        tol = 8 * lo.U * np.abs(ref)
        if k == "transl_pelvis":
            tol = tol + (ints["V"] + ints["J"]) * lo.U * (args.alpha_j3d + args.alpha_v3d) / ints["P"]
        worst = float(np.max(np.abs(sl - ref) - tol))
        print(f"grad {k:18s} slice max |diff| {np.abs(sl - ref).max():.3g}")
        assert worst <= 0, k
        if k != "transl_pelvis":
            assert np.array_equal(sl == 0, ref == 0), k
            s_abs = z["gsum_" + k][1]
            assert abs(s_abs - np.abs(g).sum()) <= 8 * lo.U * np.abs(g).sum(), k


def test_loss_class_keeps_the_reference_defaults_and_surface():
    z = np.load(GOLDEN)
    recorded = list(zip(z["default_names"].tolist(), z["default_values"].tolist()))
    parser = Loss.add_specific_args(argparse.ArgumentParser(add_help=False))
    ours = [(a.dest, float(a.default)) for a in parser._actions if a.dest != "help"]
    assert ours == recorded and dict(ours) == {k: float(v) for k, v in lo.DEFAULTS.items()}
    assert isinstance(parser.parse_args([]).start_2d_epoch, int)
    loss = Loss(parser.parse_args([]))
    assert loss.parser_args.alpha_v3d == 100.0
    import torch
    y_hat, y = {"scores": torch.zeros(1, 2, 2, 1)}, {"scores": torch.zeros(1, 2, 2)}
    with pytest.raises(_lib.MhmrError):                      # no CPU path
        loss(y_hat, y, epoch=0, img_size=224)
    with pytest.raises(_lib.MhmrError):
        loss_and_grads(y_hat, y, 0, 224, loss.parser_args)
