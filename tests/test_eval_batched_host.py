"""-m "not gpu": the host side of the batched evaluation (csrc/evalm.hip, multi_hmr_amd/evaluate.py) -- the numpy
restatement of the device rule (tests/eval_match_oracle.py) against the reference's goldens and against ``match_2d_greedy`` image by
image on the seeded batches of the GPU tests, the input conditions of those batches, the argument errors, the ABI surface."""
import os
import re

import numpy as np
import pytest
import torch

import eval_match_oracle as mo
from multi_hmr_amd import _lib
from multi_hmr_amd import evaluate as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = mo.GOLD
ENTRIES = {"mhmr_eval_match_workspace_bytes", "mhmr_eval_match", "mhmr_eval_mesh_errors_indexed"}
BAD_ARG, BAD_SHAPE = -1, -2


golden_batch, host_per_image = mo.golden_batch, mo.host_per_image


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("pair_pred", "pair_gt", "pred_fp", "gt_miss", "counters"))


def test_oracle_reproduces_the_reference_goldens():
    cnt = np.zeros(4, np.int64)
    for i in range(int(GOLD["n"])):
        pred, gt = GOLD[f"pred{i}"].astype(np.float32), GOLD[f"gt{i}"].astype(np.float32)
        o = mo.match_batch(pred, np.zeros(len(pred), np.int32), gt, np.zeros(len(gt), np.int32), 1)
        n = int(o["counters"][3])
        best = np.stack([o["pair_pred"][:n], o["pair_gt"][:n]], 1).astype(np.int64)
        assert np.array_equal(best, GOLD[f"best{i}"].reshape(-1, 2)), i
        assert list(np.nonzero(o["pred_fp"])[0]) == list(GOLD[f"fp{i}"]) and list(np.nonzero(o["gt_miss"])[0]) == list(GOLD[f"miss{i}"]), i
        assert o["status"] == 0 and (o["pair_pred"][n:] == -1).all()
        bp, bg = mo.boxes(pred), mo.boxes(gt)
        iou = np.asarray([[mo.iou(p, g) for g in bg] for p in bp])
        assert iou.dtype == np.float32 and np.array_equal(iou, GOLD[f"iou{i}"].astype(np.float32)), i
        cnt += o["counters"]
    whole = mo.match_batch(*golden_batch())                  # the same cases as images of one batch: the segments and the running sums
    assert np.array_equal(whole["counters"], cnt) and same(whole, host_per_image(*golden_batch()))


@pytest.mark.parametrize("name", sorted(mo.BATCHES))
def test_seeded_batches_meet_the_input_conditions_and_the_oracle_agrees_with_the_host(name):
    """The conditions (not tolerances) under which the fp64 closed form must order an image's pairs as numpy's fp32 SVD does and the
    IoU test cannot flip: relative gap between two distinct costs >= 1e-5, |IoU - 0.05| >= 1e-4.  The goldens have 6.7e-4 and 0.028."""
    pred, pimg, gt, gimg, B = mo.batch(name)
    J = gt.shape[1]
    for b in range(B):
        kp, kg = pred[pimg == b][:, :J], gt[gimg == b]
        if len(kp) == 0 or len(kg) == 0:
            continue
        c = np.unique(mo.costs(kp, kg))
        svd = np.asarray([[np.linalg.norm(p - g, 2) for g in kg] for p in kp], dtype=np.float64)
        assert len(c) < 2 or float(np.min(np.diff(c) / c[1:])) >= 1e-5, (name, b)
        assert np.allclose(mo.costs(kp, kg), svd, rtol=1e-5, atol=0)            # the closed form IS the spectral norm
        ious = np.asarray([[ev.get_bbx_overlap(p, g) for g in kg] for p in kp])
        assert float(np.abs(ious - 0.05).min()) >= 1e-4, (name, b)
        assert np.array_equal(ious.astype(np.float32), np.asarray([[mo.iou(p, g) for g in mo.boxes(kg)] for p in mo.boxes(kp)]))
    o = mo.match_batch(pred, pimg, gt, gimg, B)
    assert o["status"] == 0 and same(o, host_per_image(pred, pimg, gt, gimg, B))
    if "far" in mo.BATCHES[name]:
        assert o["fp_rounds"] > 0                                               # the false-positive round is exercised
    if "dup" in mo.BATCHES[name]:
        b = mo.BATCHES[name]["dup"][0]
        c = mo.costs(pred[pimg == b][:, :J], gt[gimg == b])
        assert np.array_equal(c[0], c[1])                                       # tied costs: the lowest flat index decides


def test_oracle_status_bits_leave_the_other_images_alone():
    pred, pimg, gt, gimg, B = mo.batch("j127_b6_dup_far")
    clean = mo.match_batch(pred, pimg, gt, gimg, B)
    bad = pred.copy()
    first = int(np.nonzero(pimg == 2)[0][0])
    bad[first, 5, 0] = np.nan
    o = mo.match_batch(bad, pimg, gt, gimg, B)
    keep = pimg != 2
    assert o["status"] == mo.NONFINITE and np.array_equal(o["pred_fp"][keep], clean["pred_fp"][keep]) and not o["pred_fp"][~keep].any()
    flat = gt.copy()
    flat[int(np.nonzero(gimg == 0)[0][0]), :, 0] = 7.0                          # a box without width
    assert mo.match_batch(pred, pimg, flat, gimg, B)["status"] == mo.DEGENERATE_BOX


def test_update_batched_refuses_cpu_tensors():
    e = ev.Evaluator()
    gt = dict(j2d=torch.zeros(1, 17, 2), v3d=torch.zeros(1, 10, 3), transl_pelvis=torch.zeros(1, 1, 3), idx=(torch.zeros(1, dtype=torch.long),),
              scores=torch.zeros(1, 2, 2))
    pred = dict(j2d=torch.zeros(1, 17, 2), v3d=torch.zeros(1, 10, 3), j3d=torch.zeros(1, 17, 3))
    with pytest.raises(_lib.MhmrError):
        e.update_batched(pred, torch.zeros(1, dtype=torch.int32), gt)
    with pytest.raises(_lib.MhmrError):
        ev.match_batched(pred["j2d"], torch.zeros(1, dtype=torch.int32), gt["j2d"], gt["idx"][0], 1, torch.zeros(16, dtype=torch.int64))
    with pytest.raises(_lib.MhmrError):
        ev.mesh_errors_indexed(pred["v3d"], gt["v3d"], torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    s = e.summary()                                                            # nothing was counted, and update's summary is what it was
    assert s["count"] == 0 and s["matched"] == 0 and s["pve"] == 0.0


def test_entries_are_declared_exported_bound_and_validate_before_launching():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    assert ENTRIES <= declared and ENTRIES <= set(_lib._SIGS) and declared == set(_lib.EXPORTS)
    assert "#define MHMR_VERSION 106" in header and _lib.VERSION == 106            # additive entries: the version stays
    for bit, name in enumerate(("DEGENERATE_BOX", "NONFINITE", "BAD_IMAGE_IDS")):
        assert f"#define MHMR_EVAL_{name} {1 << bit}\n" in header
    assert (mo.DEGENERATE_BOX, mo.NONFINITE, mo.BAD_IMAGE_IDS) == (1, 2, 4) and len(_lib.EVAL_STATUS) == 3
    assert f"#define MHMR_EVAL_MAX_PERSONS {_lib.EVAL_MAX_PERSONS}\n" in header and f"#define MHMR_EVAL_MAX_IMAGES {_lib.EVAL_MAX_IMAGES}\n" in header
    _lib.build()
    L = _lib.lib()
    assert L.mhmr_version() == 106 and all(hasattr(L, n) for n in ENTRIES)
    # sizes: the fp64 slab of P G pairs is in there; P = 0, G = 0 are ordinary; B >= 1
    wsb = L.mhmr_eval_match_workspace_bytes
    assert wsb(0, 0, 1) > 0 and wsb(17, 16, 6) >= 17 * 16 * 8 and wsb(17, 16, 6) % 256 == 0
    assert wsb(-1, 0, 1) == BAD_ARG and wsb(0, 0, 0) == BAD_ARG and wsb(_lib.EVAL_MAX_PERSONS + 1, 1, 1) == BAD_SHAPE
    assert wsb(1, 1, _lib.EVAL_MAX_IMAGES + 1) == BAD_SHAPE
    # every refusal comes before the first launch (pointers that are never dereferenced)
    p, n = 256, wsb(3, 2, 2)
    ok = lambda **o: dict(dict(pred=p, stride=34, pimg=p, P=3, gt=p, gimg=p, G=2, J=17, B=2, thr=0.05, ws=p, wsn=n, pp=p, pg=p, fp=p, miss=p,
                               cnt=p, status=p), **o)
    run = lambda a: L.mhmr_eval_match(a["pred"], a["stride"], a["pimg"], a["P"], a["gt"], a["gimg"], a["G"], a["J"], a["B"], a["thr"], a["ws"],
                                      a["wsn"], a["pp"], a["pg"], a["fp"], a["miss"], a["cnt"], a["status"], None)
    for bad in ([{k: None} for k in ("pred", "pimg", "gt", "gimg", "ws", "pp", "pg", "fp", "miss", "cnt", "status")] +
                [dict(P=-1), dict(G=-1), dict(J=0), dict(B=0), dict(stride=33), dict(wsn=n - 1), dict(ws=260), dict(thr=float("nan"))]):
        assert run(ok(**bad)) == BAD_ARG, bad
    assert run(ok(P=_lib.EVAL_MAX_PERSONS + 1)) == BAD_SHAPE and run(ok(B=_lib.EVAL_MAX_IMAGES + 1)) == BAD_SHAPE
    idx = lambda **o: dict(dict(pred=p, gt=p, pc=None, gc=None, pp=p, pg=p, P=3, G=2, M=2, V=14, pve=p, pa=p, sums=None, n=None), **o)
    runi = lambda a: L.mhmr_eval_mesh_errors_indexed(a["pred"], a["gt"], a["pc"], a["gc"], a["pp"], a["pg"], a["P"], a["G"], a["M"], a["V"],
                                                     a["pve"], a["pa"], a["sums"], a["n"], None)
    for bad in [{k: None} for k in ("pred", "gt", "pp", "pg", "pve", "pa")] + [dict(n=p)]:
        assert runi(idx(**bad)) == BAD_ARG, bad
    for bad in (dict(M=-1), dict(V=0), dict(P=-1), dict(G=-1)):
        assert runi(idx(**bad)) == BAD_SHAPE, bad
    assert runi(idx(M=0, pred=None, gt=None, pp=None, pg=None, pve=None, pa=None)) == 0      # nothing to do, nothing launched
    assert L.mhmr_eval_mesh_errors(None, None, None, None, 0, 14, None, None, None, None) == 0   # the plain entry is what it was
    text = open(os.path.join(ROOT, "multi_hmr_amd", "csrc", "evalm.hip")).read()
    code = re.sub(r"//.*", "", text)
    assert not re.search(r"atomic|\basm\b|hipMalloc|Synchronize", code)


def test_trainer_arguments_default_to_the_per_image_path():
    from multi_hmr_amd import train
    p = train.build_parser()
    assert p.get_default("val_batch_size") == 1
    import inspect
    assert inspect.signature(ev.evaluate_dataset).parameters["batched"].default is False
