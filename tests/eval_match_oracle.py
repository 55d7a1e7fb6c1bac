"""TEST INFRASTRUCTURE for the batched evaluation (csrc/evalm.hip mhmr_eval_match): the device rule restated in
numpy -- the fp64 closed form of the spectral-norm cost, the fp32 IoU in the host code's operation order, the greedy loop with np.argmin's
tie rule, per-image segments with the fixed slots -- and the seeded batches the host and the GPU tests share."""
import os

import numpy as np

from multi_hmr_amd import evaluate as ev

F32 = np.float32
DEGENERATE_BOX, NONFINITE, BAD_IMAGE_IDS = 1, 2, 4
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_match.npz"))     # the reference's own 12 cases


def costs(pred, gt):
    """[nP, nG] fp64: sqrt((a + c) / 2 + sqrt(((a - c) / 2)^2 + b^2)) with a, b, c summed in fp64 in joint order over the fp32 differences."""
    D = pred.astype(F32)[:, None] - gt.astype(F32)[None]                        # [nP, nG, J, 2] fp32
    dx, dy = D[..., 0].astype(np.float64), D[..., 1].astype(np.float64)
    a, b, c = (np.zeros(D.shape[:2]) for _ in range(3))
    for j in range(D.shape[2]):
        a, b, c = a + dx[..., j] * dx[..., j], b + dx[..., j] * dy[..., j], c + dy[..., j] * dy[..., j]
    h = (a - c) / 2.0
    return np.sqrt((a + c) / 2.0 + np.sqrt(h * h + b * b))


def boxes(k):
    """[n, 4] fp32 (lo x, lo y, hi x, hi y) over all joints."""
    k = k.astype(F32)
    return np.concatenate([k.min(1), k.max(1)], 1).reshape(len(k), 4)


def iou(p, g):
    """get_bbx_overlap of two boxes in fp32, one rounding per operation."""
    one, zero = F32(1), F32(0)
    iw = (min(p[2], g[2]) - max(p[0], g[0])) + one
    ih = (min(p[3], g[3]) - max(p[1], g[1])) + one
    inter = (iw if iw > 0 else zero) * (ih if ih > 0 else zero)
    a1 = ((p[2] - p[0]) + one) * ((p[3] - p[1]) + one)
    a2 = ((g[2] - g[0]) + one) * ((g[3] - g[1]) + one)
    r = inter / ((a1 + a2) - inter)
    assert r.dtype == F32
    return r


def match_image(pred, gt, thresh=0.05):
    """The loop for one image with nP, nG >= 1 -> (matches [(p, g)] in the order found, false-positive rounds)."""
    nP, nG = len(pred), len(gt)
    err = costs(pred, gt).reshape(-1)
    bp, bg = boxes(pred), boxes(gt)
    p_free, g_free = np.ones(nP, bool), np.ones(nG, bool)
    best, fp_rounds = [], 0
    while len(best) < nG and len(best) + fp_rounds < nP:
        if np.all(np.isinf(err)):
            break
        i = int(np.argmin(err))
        p, g = divmod(i, nG)
        err[i] = np.inf
        ok = iou(bp[p], bg[g]) >= F32(thresh)
        if ok and p_free[p] and g_free[g]:
            best.append((p, g))
            p_free[p] = g_free[g] = False
        elif not ok:
            fp_rounds += 1
    return best, fp_rounds


def match_batch(pred, pred_img, gt, gt_img, B, thresh=0.05):
    """What mhmr_eval_match writes: dict(pair_pred, pair_gt [min(P, G)], pred_fp [P], gt_miss [G], counters [4], status, fp_rounds).
    ``pred [P, >= J, 2]``: the first J joints count."""
    P, G, J = len(pred), len(gt), gt.shape[1]
    pred = pred[:, :J]
    M = min(P, G)
    out = dict(pair_pred=np.full(M, -1, np.int32), pair_gt=np.full(M, -1, np.int32), pred_fp=np.zeros(P, np.int32),
               gt_miss=np.zeros(G, np.int32), counters=np.zeros(4, np.int64), status=0, fp_rounds=0)
    slot = 0
    for b in range(B):
        ps, gs = np.nonzero(pred_img == b)[0], np.nonzero(gt_img == b)[0]
        nP, nG = len(ps), len(gs)
        slot0, slot = slot, slot + min(nP, nG)
        if nP + nG == 0:
            continue
        kp, kg = pred[ps].astype(F32), gt[gs].astype(F32)
        if not (np.isfinite(kp).all() and np.isfinite(kg).all()):
            out["status"] |= NONFINITE
            continue
        if nP and nG:
            bx = np.concatenate([boxes(kp), boxes(kg)])
            if not ((bx[:, 0] < bx[:, 2]) & (bx[:, 1] < bx[:, 3])).all():
                out["status"] |= DEGENERATE_BOX
                continue
        best, fpr = match_image(kp, kg, thresh) if nP and nG else ([], 0)
        out["fp_rounds"] += fpr
        out["pred_fp"][ps] = 1
        out["gt_miss"][gs] = 1
        for k, (p, g) in enumerate(best):
            out["pair_pred"][slot0 + k], out["pair_gt"][slot0 + k] = ps[p], gs[g]
            out["pred_fp"][ps[p]] = out["gt_miss"][gs[g]] = 0
        out["counters"] += (nG, nG - len(best), nP - len(best), len(best))
    return out


def make_batch(seed, J, sizes, Jp=None, dup=(), far=()):
    """A seeded batch: ``sizes`` = (nP, nG) per image; ground-truth persons stand on a jittered grid (sigma 40 px around centres 260 px
    apart), prediction p < min(nP, nG) is a ground truth of its image (in a seeded order) plus 3 px noise, the others stand somewhere in the
    frame.  ``dup``: images whose prediction 1 is a bitwise copy of prediction 0 (tied costs); ``far``: images whose LAST prediction is
    moved 5000 px away (its boxes overlap nothing).  ``Jp`` >= J joints per prediction row (the rest is noise nobody may read).
    -> pred [P, Jp, 2], pred_img [P], gt [G, J, 2], gt_img [G] (fp32 / int32)."""
    r = np.random.RandomState(seed)
    Jp = Jp or J
    pred, pimg, gt, gimg = [], [], [], []
    for b, (nP, nG) in enumerate(sizes):
        cells = r.permutation(16)[:max(nG, 1)] if nG <= 16 else np.arange(nG)
        centres = np.stack([cells % 4, cells // 4 % 4], 1) * 260.0 + 120.0 + r.uniform(-30, 30, (len(cells), 2))
        g = (centres[:nG, None] + r.randn(nG, J, 2) * 40.0).astype(F32)
        order = r.permutation(nG)
        p = np.empty((nP, Jp, 2), F32)
        for i in range(nP):
            base = g[order[i]] + r.randn(J, 2) * 3.0 if i < nG else r.uniform(100, 900, 2) + r.randn(J, 2) * 40.0
            p[i, :J] = base
            p[i, J:] = r.uniform(-1e4, 1e4, (Jp - J, 2))
        if b in dup and nP >= 2:
            p[1] = p[0]
        if b in far and nP >= 1:
            p[-1, :J] += 5000.0
        pred.append(p); gt.append(g)
        pimg += [b] * nP; gimg += [b] * nG
    return (np.concatenate(pred) if pred else np.zeros((0, Jp, 2), F32), np.asarray(pimg, np.int32),
            np.concatenate(gt) if gt else np.zeros((0, J, 2), F32), np.asarray(gimg, np.int32))


#: the seeded batches of the GPU tests: name -> make_batch's arguments and the batch size.  The seeds are the first whose batches meet the
#: input conditions tests/test_eval_batched_host.py asserts (cost gaps, IoU away from the threshold, a false-positive round where asked).
BATCHES = {
    "j55_stride127_b6": dict(seed=2, J=55, Jp=127, sizes=[(0, 0), (0, 3), (3, 0), (1, 1), (9, 8), (17, 16)], B=6),
    "j127_b6_dup_far": dict(seed=5, J=127, sizes=[(3, 2), (0, 0), (4, 4), (2, 3), (1, 1), (5, 3)], dup=(0, 2), far=(2, 3, 5), B=6),
    "j55_b1_17x16": dict(seed=4, J=55, sizes=[(17, 16)], dup=(0,), far=(0,), B=1),
    "j127_b1_1x1": dict(seed=9, J=127, Jp=130, sizes=[(1, 1)], B=1),
}


def batch(name):
    kw = dict(BATCHES[name])
    B = kw.pop("B")
    return make_batch(**kw) + (B,)


def golden_batch():
    """The 12 golden cases as 12 images of one batch (fp32, J = 17)."""
    n = int(GOLD["n"])
    pred, gt = [GOLD[f"pred{i}"].astype(np.float32) for i in range(n)], [GOLD[f"gt{i}"].astype(np.float32) for i in range(n)]
    pimg = np.concatenate([np.full(len(p), i, np.int32) for i, p in enumerate(pred)])
    gimg = np.concatenate([np.full(len(g), i, np.int32) for i, g in enumerate(gt)])
    return np.concatenate(pred), pimg, np.concatenate(gt), gimg, n


def host_per_image(pred, pimg, gt, gimg, B):
    """``ev.match_2d_greedy`` image by image, written out as ``mo.match_batch`` writes (images without pairs by ``Evaluator.update``'s
    rules)."""
    J = gt.shape[1]
    M = min(len(pred), len(gt))
    out = dict(pair_pred=np.full(M, -1, np.int32), pair_gt=np.full(M, -1, np.int32), pred_fp=np.zeros(len(pred), np.int32),
               gt_miss=np.zeros(len(gt), np.int32), counters=np.zeros(4, np.int64))
    slot = 0
    for b in range(B):
        ps, gs = np.nonzero(pimg == b)[0], np.nonzero(gimg == b)[0]
        slot0, slot = slot, slot + min(len(ps), len(gs))
        if len(ps) == 0 or len(gs) == 0:
            best, fps, misses = [], list(range(len(ps))), list(range(len(gs)))
        else:
            kg = gt[gs]
            best, fps, misses = ev.match_2d_greedy(pred[ps][:, :J], kg, np.ones_like(kg[..., 0]).astype(np.bool_))
        for k, (p, g) in enumerate(np.asarray(best, dtype=np.int64).reshape(-1, 2)):
            out["pair_pred"][slot0 + k], out["pair_gt"][slot0 + k] = ps[p], gs[g]
        out["pred_fp"][ps[np.asarray(fps, dtype=np.int64)]] = 1
        out["gt_miss"][gs[np.asarray(misses, dtype=np.int64)]] = 1
        out["counters"] += (len(gs), len(misses), len(fps), len(best))
    return out
