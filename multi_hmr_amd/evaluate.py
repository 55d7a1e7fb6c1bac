"""Accuracy harness: the reference's evaluation loop ``Trainer.evaluate`` (``train.py:336-482``) around the
MI355X path -- greedy 2D matching of predictions to ground truth, detection precision / recall / F1, per-vertex error and
Procrustes-aligned per-vertex error (and the same on regressed joints).  Matching is a few-person combinatorial loop and
stays on the host exactly as in the reference (``utils/training.py:9-195``); the mesh metrics run in
``mhmr_eval_mesh_errors`` on the device where the vertices already are.  Datasets are not part of this repository: the
caller provides ground truth dicts with the keys the reference's ``prepare_gt`` produces (``j2d [G,J,2]``, ``v3d [G,V,3]``,
``transl_pelvis [G,1,3]``, ``K``) -- or builds them from the datasets' annotations with ``groundtruth.GroundTruth``.

The 3DPW branch (train.py:383-384, 396-429): SMPL ground truth (6890 vertices) is compared with the prediction mapped onto the SMPL
topology by the ``smplx2smpl`` matrix, and MPJPE / PA-MPJPE are taken on 14 H36M joints regressed from both meshes.  Both matrices
are sparse (a handful of non-zeros per row of the 6890 x 10475 one, which the reference multiplies as a dense 288 MB matrix): they
are held in CSR form and applied by ``mhmr_sparse_regress``.

Whole batches: ``Evaluator.update_batched`` runs the same matching per image on the device (``mhmr_eval_match``)
and the metrics through its pair list (``mhmr_eval_mesh_errors_indexed``), with no copy to the host; ``evaluate_dataset(batched=True)``."""
from __future__ import annotations

from itertools import product

import numpy as np
import torch

from . import _lib


def compute_prf1(count, miss, fp):
    """utils/training.py:9-24 (precision, recall, F1 in percent, each rounded to 2 decimals before scaling)."""
    if count == 0:
        return 0, 0, 0
    tp, fn = count - miss, miss
    if tp == 0:
        return 0., 0., 0.
    f1 = round(tp / (tp + 0.5 * (fp + fn)), 2)
    recall = round(tp / (tp + fn), 2)
    precision = round(tp / (tp + fp), 2)
    return 100. * precision, 100. * recall, 100. * f1


def get_bbx_overlap(p1, p2):
    """utils/training.py:149-195: IoU of the two keypoint sets' axis-aligned boxes (inclusive +1 pixel convention)."""
    lo1, lo2, hi1, hi2 = np.min(p1, axis=0), np.min(p2, axis=0), np.max(p1, axis=0), np.max(p2, axis=0)
    assert lo1[0] < hi1[0] and lo1[1] < hi1[1] and lo2[0] < hi2[0] and lo2[1] < hi2[1]
    x_left, y_top = max(lo1[0], lo2[0]), max(lo1[1], lo2[1])
    x_right, y_bottom = min(hi1[0], hi2[0]), min(hi1[1], hi2[1])
    inter = max(0, x_right - x_left + 1) * max(0, y_bottom - y_top + 1)
    a1 = (hi1[0] - lo1[0] + 1) * (hi1[1] - lo1[1] + 1)
    a2 = (hi2[0] - lo2[0] + 1) * (hi2[1] - lo2[1] + 1)
    return inter / float(a1 + a2 - inter)


def match_2d_greedy(pred_kps, gtkp, valid_mask, iou_thresh=0.05, valid=None):
    """utils/training.py:26-147: visit (prediction, ground truth) pairs by ascending 2D keypoint distance; a pair whose boxes
    overlap by >= iou_thresh and whose members are both free is a match; the closest remaining pair failing the IoU test is
    counted as one false positive and ends that round.  Returns (matches [n,2] (pred, gt), false-positive pred ids,
    missed gt ids)."""
    n_pred, n_gt = len(pred_kps), len(gtkp)
    combs = list(product(range(n_pred), range(n_gt)))
    err = np.empty(len(combs))
    for c, (p, g) in enumerate(combs):
        vmask = valid_mask[g]
        assert vmask.sum() > 0, "no valid points"
        err[c] = np.linalg.norm(pred_kps[p][vmask, :2] - gtkp[g][vmask, :2], 2)
    gt_assigned = np.zeros(n_gt, dtype=bool)
    op_assigned = np.zeros(n_pred, dtype=bool)
    best, fp_counter = [], 0
    while gt_assigned.sum() < n_gt and op_assigned.sum() + fp_counter < n_pred:
        found = false_positive = False
        while not found:
            if np.all(np.isinf(err)):
                print("something went wrong here")     # the reference prints and would loop forever; stop instead
                return _finish(best, n_pred, n_gt, valid)
            i = int(np.argmin(err))
            p, g = combs[i]
            iou = get_bbx_overlap(pred_kps[p], gtkp[g])
            err[i] = np.inf
            if not op_assigned[p] and not gt_assigned[g] and iou >= iou_thresh:
                found = True
            elif iou < iou_thresh:
                found = false_positive = True
                fp_counter += 1
        if valid is not None:
            if valid[g]:
                if not false_positive:
                    best.append((p, g))
                    op_assigned[p] = gt_assigned[g] = True
            else:
                gt_assigned[g] = True
        elif not false_positive:
            best.append((p, g))
            op_assigned[p] = gt_assigned[g] = True
    return _finish(best, n_pred, n_gt, valid)


def _finish(best, n_pred, n_gt, valid):
    best = np.array(best)
    ops = sorted(int(b[0]) for b in best)
    gts = sorted(int(b[1]) for b in best)
    false_positives = [int(i) for i in np.setdiff1d(np.arange(n_pred), ops)]
    misses = [int(i) for i in np.setdiff1d(np.arange(n_gt), gts) if valid is None or valid[i]]
    return best, false_positives, misses


def mesh_errors(pred_pts, gt_pts, pred_center=None, gt_center=None, return_transform=False):
    """PVE and PA-PVE in millimetres for M pairs (train.py:372-389): ``pred_pts`` / ``gt_pts`` ``[M,V,3]`` fp32 device tensors,
    optional centres ``[M,3]``.  One launch of ``mhmr_eval_mesh_errors``; no host sync."""
    if pred_pts.device.type != "cuda":
        raise _lib.MhmrError("mesh_errors runs on the HIP device only (no CPU fallback)")
    M, V = int(pred_pts.shape[0]), int(pred_pts.shape[1])
    dev = pred_pts.device
    f = lambda t: None if t is None else t.to(device=dev, dtype=torch.float32).reshape(M, 3).contiguous()
    p, g = pred_pts.to(torch.float32).contiguous(), gt_pts.to(device=dev, dtype=torch.float32).contiguous()
    assert g.shape == p.shape and p.shape[2] == 3
    pc, gc = f(pred_center), f(gt_center)
    pve, pa = torch.empty(M, device=dev), torch.empty(M, device=dev)
    rts = torch.empty(M, 13, device=dev) if return_transform else None
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.lib().mhmr_eval_mesh_errors(p.data_ptr(), g.data_ptr(), ptr(pc), ptr(gc), M, V, pve.data_ptr(), pa.data_ptr(), ptr(rts),
                                                torch.cuda.current_stream(dev).cuda_stream), "mhmr_eval_mesh_errors")
    return (pve, pa, rts) if return_transform else (pve, pa)


def new_eval_state(device):
    """The device state of the batched evaluation: 16 int64 words -- ``[0:4]`` count, miss, fp, matched (``mhmr_eval_match``'s counters),
    ``[4]`` / ``[5]`` the pairs that entered the mesh / joint sums, ``[6]`` the sticky status word, ``[8:12]`` the fp64 sums of pve, pa_pve,
    mpjpe, pa_mpjpe (read with ``.view(torch.float64)``)."""
    return torch.zeros(16, dtype=torch.int64, device=device)


def match_batched(pred_j2d, pred_img, gt_j2d, gt_img, batch_size, state, iou_thresh=0.05):
    """``match_2d_greedy`` for every image of a batch in one call of ``mhmr_eval_match`` (include/mhmr.h has the rule): ``pred_j2d [P, Jp, 2]``
    with ``Jp >= J`` (its first J joints are read where they lie), ``pred_img [P]`` and ``gt_img [G]`` ascending image ids, ``gt_j2d [G, J,
    2]``, all on the device; ``state``: ``new_eval_state``'s tensor, whose counters are added to.  Returns ``(pair_pred, pair_gt, pred_fp,
    gt_miss)`` int32 device tensors ``[min(P, G)]``, ``[min(P, G)]``, ``[P]``, ``[G]``.  No host sync."""
    if gt_j2d.device.type != "cuda" or state.device != gt_j2d.device or (pred_j2d is not None and pred_j2d.device != gt_j2d.device):
        raise _lib.MhmrError("match_batched runs on the HIP device only (no CPU fallback)")
    dev = gt_j2d.device
    G, J = int(gt_j2d.shape[0]), int(gt_j2d.shape[1])
    P = 0 if pred_j2d is None else int(pred_j2d.shape[0])
    g2 = gt_j2d.to(torch.float32).contiguous()
    gi = gt_img.to(device=dev, dtype=torch.int32).contiguous()
    if P:
        if int(pred_j2d.shape[1]) < J or int(pred_j2d.shape[2]) != 2:
            raise ValueError(f"the predictions have {tuple(pred_j2d.shape[1:])} keypoints per person, the ground truth {J} x 2")
        p2 = pred_j2d.to(torch.float32)
        if p2.stride(2) != 1 or p2.stride(1) != 2 or p2.stride(0) < 2 * J:
            p2 = p2.contiguous()
        pi, stride = pred_img.to(device=dev, dtype=torch.int32).contiguous(), int(p2.stride(0))
        if int(pi.shape[0]) != P:
            raise ValueError(f"{P} predictions, {int(pi.shape[0])} image ids")
    else:
        p2, pi, stride = None, None, 2 * J
    if int(gi.shape[0]) != G:
        raise ValueError(f"{G} ground-truth persons, {int(gi.shape[0])} image ids")
    M = min(P, G)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    pair_pred, pair_gt, pred_fp, gt_miss = i32(M), i32(M), i32(P), i32(G)
    nbytes = _lib.workspace_bytes("mhmr_eval_match_workspace_bytes", P, G, int(batch_size))
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mhmr_eval_match(_lib.ptr(p2), stride, _lib.ptr(pi), P, g2.data_ptr() if G else None, gi.data_ptr() if G else None,
                                              G, J, int(batch_size), float(iou_thresh), ws.data_ptr(), nbytes, _lib.ptr(pair_pred) if M else None,
                                              _lib.ptr(pair_gt) if M else None, _lib.ptr(pred_fp) if P else None, _lib.ptr(gt_miss) if G else None,
                                              state.data_ptr(), state[6:].data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                   "mhmr_eval_match")
    return pair_pred, pair_gt, pred_fp, gt_miss


def mesh_errors_indexed(pred_pts, gt_pts, pair_pred, pair_gt, pred_center=None, gt_center=None, sums=None, n_valid=None):
    """``mesh_errors`` of the pairs ``(pred_pts[pair_pred[m]], gt_pts[pair_gt[m]])`` read where they lie (``mhmr_eval_mesh_errors_indexed``):
    ``pred_pts [P, V, 3]``, ``gt_pts [G, V, 3]``, centres ``[P, 3]`` / ``[G, 3]``, the index tensors int32 ``[M]`` (-1 = no pair: 0 is
    written).  ``sums``: fp64 device tensor ``[2]`` that gains the valid pairs' pve / pa_pve totals (added in slot order), ``n_valid``: int64
    ``[1]`` that gains their number.  Returns ``(pve [M], pa_pve [M])``; no host sync."""
    if pred_pts.device.type != "cuda":
        raise _lib.MhmrError("mesh_errors_indexed runs on the HIP device only (no CPU fallback)")
    dev = pred_pts.device
    P, V, G, M = int(pred_pts.shape[0]), int(pred_pts.shape[1]), int(gt_pts.shape[0]), int(pair_pred.shape[0])
    p, g = pred_pts.to(torch.float32).contiguous(), gt_pts.to(device=dev, dtype=torch.float32).contiguous()
    assert p.shape[2] == 3 and tuple(g.shape[1:]) == (V, 3) and int(pair_gt.shape[0]) == M
    assert pair_pred.dtype == torch.int32 and pair_gt.dtype == torch.int32 and pair_pred.is_contiguous() and pair_gt.is_contiguous()
    pc = None if pred_center is None else pred_center.to(device=dev, dtype=torch.float32).reshape(P, 3).contiguous()
    gc = None if gt_center is None else gt_center.to(device=dev, dtype=torch.float32).reshape(G, 3).contiguous()
    pve, pa = torch.empty(M, device=dev), torch.empty(M, device=dev)
    assert sums is None or (sums.dtype == torch.float64 and sums.numel() >= 2)
    assert n_valid is None or (sums is not None and n_valid.dtype == torch.int64)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mhmr_eval_mesh_errors_indexed(p.data_ptr(), g.data_ptr(), _lib.ptr(pc), _lib.ptr(gc), pair_pred.data_ptr(),
                                                            pair_gt.data_ptr(), P, G, M, V, pve.data_ptr(), pa.data_ptr(), _lib.ptr(sums),
                                                            _lib.ptr(n_valid), torch.cuda.current_stream(dev).cuda_stream),
                   "mhmr_eval_mesh_errors_indexed")
    return pve, pa


def csr_from_matrix(matrix):
    """Dense (numpy / torch) or scipy-sparse matrix -> (rowptr int32 [R + 1], col int32, val float32, (R, C)); the entries of a row
    are in ascending column order (the kernel sums them in that order), explicit zeros are dropped."""
    if hasattr(matrix, "tocsr"):
        m = matrix.tocsr().copy()
        m.sum_duplicates()
        m.sort_indices()
        m.eliminate_zeros()
        return (np.asarray(m.indptr, dtype=np.int32), np.asarray(m.indices, dtype=np.int32), np.asarray(m.data, dtype=np.float32),
                (int(m.shape[0]), int(m.shape[1])))
    if isinstance(matrix, torch.Tensor):
        matrix = matrix.detach().cpu().numpy()
    a = np.asarray(matrix)
    if a.ndim != 2:
        raise ValueError(f"a regressor is a matrix, got shape {a.shape}")
    rows, cols = np.nonzero(a)                                  # row-major: ascending columns inside a row
    rowptr = np.zeros(a.shape[0] + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=a.shape[0]), out=rowptr[1:])
    return rowptr, cols.astype(np.int32), a[rows, cols].astype(np.float32), (int(a.shape[0]), int(a.shape[1]))


class SparseRegressor:
    """``out [M, R, 3] = A (x [M, C, 3] - center [M, 3])`` on the device for a fixed sparse ``A`` (CSR made once here, uploaded once per
    device).  Deterministic: a row is summed in column order."""

    def __init__(self, matrix):
        self.rowptr, self.col, self.val, self.shape = csr_from_matrix(matrix)
        if self.col.size and not (0 <= int(self.col.min()) and int(self.col.max()) < self.shape[1]):
            raise ValueError("column index outside the matrix")
        self._dev = {}

    @property
    def nnz(self):
        return int(self.val.size)

    def __call__(self, x, center=None):
        if x.device.type != "cuda":
            raise _lib.MhmrError("SparseRegressor runs on the HIP device only (no CPU fallback)")
        R, Cn = self.shape
        assert x.dim() == 3 and x.shape[1] == Cn and x.shape[2] == 3, (tuple(x.shape), self.shape)
        dev, M = x.device, int(x.shape[0])
        key = (dev.type, dev.index)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(dev) for a in (self.rowptr, self.col, self.val))
        rp, co, va = self._dev[key]
        x = x.to(torch.float32).contiguous()
        c = None if center is None else center.to(device=dev, dtype=torch.float32).reshape(M, 3).contiguous()
        out = torch.empty(M, R, 3, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mhmr_sparse_regress(rp.data_ptr(), _lib.ptr(co) if co.numel() else None, _lib.ptr(va) if va.numel() else None,
                                                      R, Cn, x.data_ptr(), _lib.ptr(c), M, out.data_ptr(),
                                                      torch.cuda.current_stream(dev).cuda_stream), "mhmr_sparse_regress")
        return out


def load_smplx2smpl(path) -> SparseRegressor:
    """train.py:44-45: the pickle with key ``'matrix'`` (6890 x 10475, dense or scipy-sparse)."""
    import pickle
    with open(path, "rb") as f:
        return SparseRegressor(pickle.load(f, encoding="latin1")["matrix"])


def load_h36m_regressor(path) -> SparseRegressor:
    """train.py:400: ``J_regressor_h36m.npy`` (17 x 6890)."""
    return SparseRegressor(np.load(path))


class Evaluator:
    """Accumulates the reference's metrics over batches::

        ev = Evaluator()
        for x, gt in data:                       # gt: dict(j2d [G,J,2], v3d [G,V,3], transl_pelvis [G,1,3], K)
            humans = model(x, is_training=False, K=gt['K'], det_thresh=0.2, nms_kernel_size=3)
            ev.update(humans, gt)
        print(ev.summary())                      # pve, pa_pve (mm), precision, recall, f1_score (%)
    """

    def __init__(self, smplx2smpl=None, h36m_regressor=None):
        """``smplx2smpl``: when the ground truth has 6890 vertices the prediction is regressed to SMPL before PVE / PA-PVE
        (train.py:383-384).  ``h36m_regressor``: mpjpe / pa_mpjpe are taken on the 14 joints ``H36M_TO_J14`` regressed from the (SMPL)
        meshes and centred on H36M joint 0 (train.py:396-429) instead of the body model's own joints.  Both: a ``SparseRegressor`` or a
        matrix."""
        as_reg = lambda m: m if m is None or isinstance(m, SparseRegressor) else SparseRegressor(m)
        self.smplx2smpl, self.h36m_regressor = as_reg(smplx2smpl), as_reg(h36m_regressor)
        self.count = self.miss = self.fp = 0
        self._sums = {k: torch.zeros((), dtype=torch.float64) for k in ("pve", "pa_pve", "mpjpe", "pa_mpjpe")}
        self._n = self._nj = 0
        self._state = None              # update_batched's device state (new_eval_state), made on its first call
        self._j14 = {}                  # H36M_TO_J14 on the device(s)

    @torch.no_grad()
    def update_batched(self, pred, img_id, gt, iou_thresh=0.05):
        """``update`` for a whole batch, on the device: ``pred`` the dict of batched tensors ``[P, ...]`` (``j2d``,
        ``v3d``, ``j3d``, ``transl_pelvis`` or joint 0 of ``j3d``) that ``model(x, K=, return_batched=True)`` returns with its image ids
        ``img_id [P]`` -- or the ``is_training=True`` dict with ``gt["idx"][0]``; ``{}`` when nobody was detected -- and ``gt`` what
        ``GroundTruth.prepare`` returns (image column ``gt["idx"][0]``, batch size ``gt["scores"].shape[0]``).  Predictions are matched
        with the ground truth of their own image only (``mhmr_eval_match``), the metrics read the matched rows where they lie
        (``mhmr_eval_mesh_errors_indexed``), and every sum and counter stays in one device state that ``summary()`` reads: no copy to the
        host and no synchronisation here.  The same branches as ``update``; an empty ground truth or ``P == 0`` is legal."""
        gt_j2d = gt["j2d"]
        if gt_j2d.device.type != "cuda" or any(isinstance(v, torch.Tensor) and v.device != gt_j2d.device for v in pred.values()):
            raise _lib.MhmrError("Evaluator.update_batched runs on the HIP device only (no CPU fallback): predictions and ground truth on one GPU")
        dev = gt_j2d.device
        if self._state is None:
            self._state = new_eval_state(dev)
        st = self._state
        if st.device != dev:
            raise _lib.MhmrError(f"this Evaluator's state is on {st.device}, the batch on {dev}")
        P, G = (int(pred["j2d"].shape[0]) if "j2d" in pred else 0), int(gt_j2d.shape[0])
        B = int(gt["scores"].shape[0]) if "scores" in gt else int(gt["K"].shape[0])
        pair_pred, pair_gt, _, _ = match_batched(pred["j2d"] if P else None, img_id if P else None, gt_j2d, gt["idx"][0], B, st, iou_thresh)
        if min(P, G) == 0:
            return
        sums = st[8:12].view(torch.float64)
        v_hat, v_gt = pred["v3d"], gt["v3d"]
        c_hat = (pred["transl_pelvis"] if "transl_pelvis" in pred else pred["j3d"][:, :1]).reshape(P, 3)
        c_gt = gt["transl_pelvis"].reshape(G, 3)
        if v_gt.shape[1] == 6890 and v_hat.shape[1] != 6890:
            if self.smplx2smpl is None:
                raise _lib.MhmrError("the ground truth is an SMPL mesh: Evaluator(smplx2smpl=...) is needed to compare (train.py:383-384)")
            v_hat, c_hat = self.smplx2smpl(v_hat, c_hat), None          # every prediction centred, then regressed; the pairs index the result
        mesh_errors_indexed(v_hat, v_gt, pair_pred, pair_gt, c_hat, c_gt, sums[0:2], st[4:5])
        if self.h36m_regressor is not None:
            from .constants import H36M_TO_J14
            if v_hat.shape[1] != self.h36m_regressor.shape[1] or v_gt.shape[1] != self.h36m_regressor.shape[1]:
                raise _lib.MhmrError("the H36M regressor does not fit the meshes")
            key = (dev.type, dev.index)
            if key not in self._j14:
                self._j14[key] = torch.as_tensor(H36M_TO_J14, device=dev)
            j14 = self._j14[key]
            h_gt, h_hat = self.h36m_regressor(v_gt, c_gt), self.h36m_regressor(v_hat, c_hat)     # [G, 17, 3] / [P, 17, 3] of the centred meshes
            mesh_errors_indexed(h_hat[:, j14], h_gt[:, j14], pair_pred, pair_gt, h_hat[:, 0], h_gt[:, 0], sums[2:4], st[5:6])
        elif "j3d" in gt:
            j_gt = gt["j3d"]
            j_hat = pred["j3d"][:, :j_gt.shape[1]]
            mesh_errors_indexed(j_hat, j_gt, pair_pred, pair_gt, j_hat[:, 0], j_gt[:, 0], sums[2:4], st[5:6])

    @torch.no_grad()
    def update(self, pred, gt):
        kp_gt = gt["j2d"].detach().cpu().numpy()
        if len(pred) == 0:
            self.count += len(kp_gt)
            self.miss += len(kp_gt)
            return
        kp_pred = np.asarray([h["j2d"].detach().cpu().numpy()[:kp_gt.shape[1]] for h in pred])
        best, fps, misses = match_2d_greedy(kp_pred, kp_gt, np.ones_like(kp_gt[..., 0]).astype(np.bool_))
        self.count += len(kp_gt)
        self.miss += len(misses)
        self.fp += len(fps)
        if len(best) == 0:
            return
        dev = pred[0]["v3d"].device
        pid, gid = [int(b[0]) for b in best], [int(b[1]) for b in best]
        v_hat = torch.stack([pred[i]["v3d"] for i in pid])
        c_hat = torch.stack([pred[i]["transl_pelvis"].reshape(3) for i in pid])
        v_gt = gt["v3d"][gid].to(dev)
        c_gt = gt["transl_pelvis"][gid].reshape(-1, 3).to(dev)
        if v_gt.shape[1] == 6890 and v_hat.shape[1] != 6890:
            if self.smplx2smpl is None:
                raise _lib.MhmrError("the ground truth is an SMPL mesh: Evaluator(smplx2smpl=...) is needed to compare (train.py:383-384)")
            v_hat, c_hat = self.smplx2smpl(v_hat, c_hat), None          # centred, then regressed, as the reference
        pve, pa = mesh_errors(v_hat, v_gt, c_hat, c_gt)
        self._sums["pve"] += pve.double().sum().cpu()
        self._sums["pa_pve"] += pa.double().sum().cpu()
        if self.h36m_regressor is not None:
            from .constants import H36M_TO_J14
            if v_hat.shape[1] != self.h36m_regressor.shape[1] or v_gt.shape[1] != self.h36m_regressor.shape[1]:
                raise _lib.MhmrError("the H36M regressor does not fit the meshes")
            j14 = torch.as_tensor(H36M_TO_J14, device=dev)
            h_gt, h_hat = self.h36m_regressor(v_gt, c_gt), self.h36m_regressor(v_hat, c_hat)     # [M, 17, 3] of the centred meshes
            mp, pamp = mesh_errors(h_hat[:, j14], h_gt[:, j14], h_hat[:, 0], h_gt[:, 0])
            self._sums["mpjpe"] += mp.double().sum().cpu()
            self._sums["pa_mpjpe"] += pamp.double().sum().cpu()
            self._nj += len(best)
        elif "j3d" in gt:        # joint errors on the body model's own joints, pelvis-centred (without an H36M regressor)
            j_gt = gt["j3d"][gid].to(dev)
            J = j_gt.shape[1]
            j_hat = torch.stack([pred[i]["j3d"][:J] for i in pid])
            mp, pamp = mesh_errors(j_hat, j_gt, j_hat[:, 0], j_gt[:, 0])
            self._sums["mpjpe"] += mp.double().sum().cpu()
            self._sums["pa_mpjpe"] += pamp.double().sum().cpu()
            self._nj += len(best)
        self._n += len(best)

    def summary(self):
        """The metrics over everything ``update`` (host sums) and ``update_batched`` (the device state, read here in ONE copy) have seen;
        raises ``MhmrError`` when a batched call met a degenerate keypoint box, a non-finite keypoint or unsorted image ids."""
        if self._state is None:
            count, miss, fp, n, nj, sums = self.count, self.miss, self.fp, self._n, self._nj, self._sums
        else:
            host = self._state.cpu()                                    # the one read of the device state
            words, dsum = host.tolist(), host[8:12].view(torch.float64)
            status = words[6] & 0xFFFFFFFF
            if status:
                what = "; ".join(m for b, m in enumerate(_lib.EVAL_STATUS) if status >> b & 1)
                raise _lib.MhmrError(f"Evaluator.update_batched met input the reference's matching refuses (status {status}): {what}")
            count, miss, fp, n, nj = self.count + words[0], self.miss + words[1], self.fp + words[2], self._n + words[4], self._nj + words[5]
            sums = {k: self._sums[k] + dsum[i] for i, k in enumerate(("pve", "pa_pve", "mpjpe", "pa_mpjpe"))}
        precision, recall, f1 = compute_prf1(count, miss, fp)
        out = {k: float(sums[k] / max(n, 1)) for k in ("pve", "pa_pve")}
        if nj:
            out.update({k: float(sums[k] / nj) for k in ("mpjpe", "pa_mpjpe")})
        out.update(precision=precision, recall=recall, f1_score=f1, matched=n, count=count)
        return out


@torch.no_grad()
def evaluate_dataset(model, batches, gt_builder, det_thresh=0.3, nms_kernel_size=3, use_gt_idx=False, evaluator=None, loss=None, epoch=0,
                     batched=False):
    """The reference's evaluation loop (train.py:346-429) over ``batches`` of ``(x, y)``: ``gt = gt_builder.prepare(y)``, the
    inference forward with ``K=gt['K']``, matching and metrics; returns ``Evaluator.summary()``.  ``evaluator``: an ``Evaluator`` carrying
    the regressors (a fresh plain one otherwise).  A batch without humans is skipped (``prepare`` returns None; the reference would fail
    on ``gt['K']``).

    ``use_gt_idx=True`` is OURS -- the reference has no such switch: the ground truth's own ``gt['idx']`` goes through the
    ``is_training=True`` forward, so every ground-truth person gets exactly one prediction at its own cell and the mesh metrics are
    measured without the detector in the way.

    ``loss``: a ``multi_hmr_amd.Loss`` (needs ``use_gt_idx=True``): the ``is_training`` output of every batch also goes through it with
    ``epoch`` and the model's ``img_size``, and the summary gains ``loss/<key>`` -- the mean over the batches of each of its eleven
    values, as the reference's validation meters keep them (train.py:346-429).  The sums stay on the device until the end.

    ``batched=True`` is OURS: batches of several images.  The forward returns batched tensors (``return_batched=True``, or the
    ``use_gt_idx`` dict) and ``Evaluator.update_batched`` matches every image's predictions with that image's ground truth on the device.
    ``batched=False`` pairs ALL predictions with ALL ground truth of a batch, as the reference does: right for batches of one image only."""
    if loss is not None and not use_gt_idx:
        raise _lib.MhmrError("evaluate_dataset(loss=...) needs use_gt_idx=True: the loss reads the is_training output at the ground truth's cells")
    ev = evaluator if evaluator is not None else Evaluator()
    loss_sum, loss_n = None, 0
    dev = next(iter(model.parameters())).device if hasattr(model, "parameters") else torch.device("cuda")
    for x, y in batches:
        y = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in y.items()}
        gt = gt_builder.prepare(y)
        if gt is None:
            continue
        x = x.to(dev)
        if batched:                                      # the whole batch at once: matching per image and the metrics stay on the device
            if use_gt_idx:
                out, ids = model(x, idx=gt["idx"], K=gt["K"], is_training=True), gt["idx"][0]
                if loss is not None:
                    _, dl = loss(out, gt, epoch=epoch, img_size=model.img_size)
                    vals = torch.stack([dl[k] for k in dl]).double()
                    loss_sum, loss_n, loss_keys = (vals if loss_sum is None else loss_sum + vals), loss_n + 1, list(dl)
            else:
                out, ids = model(x, is_training=False, K=gt["K"], det_thresh=det_thresh, nms_kernel_size=nms_kernel_size, return_batched=True)
            ev.update_batched(out, ids, gt)
            continue
        if use_gt_idx:
            out = model(x, idx=gt["idx"], K=gt["K"], is_training=True)
            n = int(gt["idx"][0].shape[0])
            pelvis = out["transl_pelvis"] if "transl_pelvis" in out else out["j3d"][:, :1]
            pred = [dict(v3d=out["v3d"][i], j3d=out["j3d"][i], j2d=out["j2d"][i], transl_pelvis=pelvis[i]) for i in range(n)]
            if loss is not None:
                _, dl = loss(out, gt, epoch=epoch, img_size=model.img_size)
                vals = torch.stack([dl[k] for k in dl]).double()
                loss_sum, loss_n, loss_keys = (vals if loss_sum is None else loss_sum + vals), loss_n + 1, list(dl)
        else:
            pred = model(x, is_training=False, K=gt["K"], det_thresh=det_thresh, nms_kernel_size=nms_kernel_size)
        ev.update(pred, gt)
    summary = ev.summary()
    if loss_n:
        summary.update({"loss/" + k: v / loss_n for k, v in zip(loss_keys, loss_sum.tolist())})
    return summary
