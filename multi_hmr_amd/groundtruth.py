"""Ground truth from the datasets' annotations: the reference's ``Trainer.prepare_gt`` (train.py:58-182) on the
device -- body models through ``mhmr_body_forward``, EHF joints through ``mhmr_sparse_regress``, the detection targets and the
occlusion rule through ``mhmr_gt_targets``.  ``prepare`` takes the collated ``y`` of the reference's datasets
(datasets/bedlam.py:365-426) and returns exactly the keys ``prepare_gt`` returns, so ``gt['idx']`` can drive the
``is_training=True`` forward and ``Evaluator.update`` gets its meshes.

Three annotation families, told apart by their keys as in the reference:
  ``smplx_vertices``                      EHF: raw SMPL-X vertices; joints = J_regressor . vertices (55 joints).
  ``smpl_root_pose`` ...                  3DPW: gendered SMPL parameters (``smpl_gender_id`` == 2 marks a female annotation).
  ``smplx_root_pose`` ...                 BEDLAM: SMPL-X parameters with 11 betas, eye poses and a translation.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .bodymodel import BodyModel
from .constants import SMPLX_JOINT_NAMES
from .evaluate import SparseRegressor


class GroundTruth:
    def __init__(self, img_size, patch_size=14, nearness=True, person_center="head", smplx_neutral=None, smpl_male=None, smpl_female=None,
                 device=None):
        """``smplx_neutral`` / ``smpl_male`` / ``smpl_female``: ``BodyModel`` instances, or model data (dict / path) from which
        ``BodyModel(data, 'smplx', num_betas=11)`` / ``BodyModel(data, 'smpl', num_betas=10)`` are made, as train.py:41-43 does.
        ``device``: where ``prepare`` works; None = the device ``y`` is on (which must be the GPU)."""
        mk = lambda m, kind, nb: m if m is None or isinstance(m, BodyModel) else BodyModel(m, kind, num_betas=nb)
        self.smplx_neutral, self.smpl_male, self.smpl_female = mk(smplx_neutral, "smplx", 11), mk(smpl_male, "smpl", 10), mk(smpl_female, "smpl", 10)
        self.img_size, self.patch_size, self.nearness = int(img_size), int(patch_size), bool(nearness)
        self.center_joint = SMPLX_JOINT_NAMES.index(person_center)              # train.py:117 (the SMPL joints share the first 22 names)
        self.focal_norm = self.img_size / (2 * math.tan(math.radians(60) / 2))  # utils/camera.py:50-69, fovn = 60
        self.device = torch.device(device) if device is not None else None
        self._ehf_regressor = None

    def _need(self, m, name):
        if m is None:
            raise _lib.MhmrError(f"these annotations need GroundTruth({name}=...)")
        return m

    @torch.no_grad()
    def prepare(self, y):
        dev = self.device if self.device is not None else y["valid_humans"].device
        if dev.type != "cuda":
            raise _lib.MhmrError("GroundTruth.prepare runs on the HIP device only (no CPU fallback): move y there or pass device=")
        y = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in y.items()}
        valid_h = y["valid_humans"]
        bs, nh = valid_h.shape
        ib, ih = torch.where(valid_h > 0)                                       # (image, human) order
        n = int(ib.shape[0])
        if n == 0 or not any(k in y for k in ("smplx_vertices", "smpl_root_pose", "smplx_root_pose")):
            return None                                                         # train.py:111-112
        K = y["K"].to(torch.float32)[ib].contiguous()
        sel = lambda key, *shape: y[key].reshape(bs, nh, -1)[ib, ih].reshape(n, *shape).to(torch.float32)
        has_params = False
        if "smplx_vertices" in y:                                               # EHF (train.py:70-73)
            bm = self._need(self.smplx_neutral, "smplx_neutral")
            verts = y["smplx_vertices"].to(torch.float32).reshape(n, -1, 3).contiguous()
            if self._ehf_regressor is None:
                self._ehf_regressor = SparseRegressor(bm.J_regressor)
            jts = self._ehf_regressor(verts)
            v2d, j2d = self._project(verts, K), self._project(jts, K)
        elif "smpl_root_pose" in y:                                             # 3DPW (train.py:74-94)
            male = self._need(self.smpl_male, "smpl_male")
            args = dict(global_orient=sel("smpl_root_pose", 3), body_pose=sel("smpl_body_pose", 69), betas=sel("smpl_shape", 10),
                        transl=sel("smpl_transl", 3))
            # The reference runs the male model on everybody and, when the batch holds a female annotation, the female model on everybody
            # too and overwrites those rows (it indexes them by the human's position in its image: right for its batches of one image).
            # Here each human goes through the model of its own annotation, which gives the same rows.
            female = (y["smpl_gender_id"].reshape(bs, nh)[ib, ih] == 2) if "smpl_gender_id" in y else torch.zeros(n, dtype=torch.bool, device=dev)
            verts = torch.empty(n, male.num_vertices, 3, device=dev)
            jts = torch.empty(n, male.num_out_joints, 3, device=dev)
            v2d, j2d = torch.empty(n, male.num_vertices, 2, device=dev), torch.empty(n, male.num_out_joints, 2, device=dev)
            for mask, bm, name in ((~female, male, "smpl_male"), (female, self.smpl_female, "smpl_female")):
                ids = torch.nonzero(mask).reshape(-1)
                if ids.numel() == 0:
                    continue
                o = self._need(bm, name)(K=K[ids], **{k: v[ids] for k, v in args.items()})
                verts[ids], jts[ids], v2d[ids], j2d[ids] = o.vertices, o.joints, o.v2d, o.j2d
        else:                                                                   # BEDLAM (train.py:95-110)
            has_params = True
            bm = self._need(self.smplx_neutral, "smplx_neutral")
            o = bm(global_orient=sel("smplx_root_pose", 3), body_pose=sel("smplx_body_pose", 63), jaw_pose=sel("smplx_jaw_pose", 3),
                   leye_pose=sel("smplx_leye_pose", 3), reye_pose=sel("smplx_reye_pose", 3), left_hand_pose=sel("smplx_left_hand_pose", 45),
                   right_hand_pose=sel("smplx_right_hand_pose", 45), betas=sel("smplx_shape", bm.num_betas), transl=sel("smplx_transl", 3),
                   expression=bm.expression.to(dev).repeat(n, 1), K=K)
            verts, jts, v2d, j2d = o.vertices, o.joints, o.v2d, o.j2d

        # detection targets and the occlusion rule (train.py:116-158)
        Gp = self.img_size // self.patch_size
        NJ = int(jts.shape[1])
        loc, offset = torch.empty(n, 2, device=dev), torch.empty(n, 2, device=dev)
        pk_idx, visible = torch.empty(n, 2, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        dist_pp, scores = torch.empty(n, device=dev), torch.empty(bs, Gp, Gp, device=dev)
        owner = torch.empty(bs * Gp * Gp, dtype=torch.int32, device=dev)
        img = ib.to(torch.int32).contiguous()
        jts = jts.contiguous()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mhmr_gt_targets(jts.data_ptr(), NJ, self.center_joint, K.data_ptr(), img.data_ptr(), n, bs, Gp, self.patch_size,
                                                  float(self.focal_norm), int(self.nearness), loc.data_ptr(), pk_idx.data_ptr(), offset.data_ptr(),
                                                  dist_pp.data_ptr(), scores.data_ptr(), visible.data_ptr(), owner.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream), "mhmr_gt_targets")
        target = dict(transl=jts[:, self.center_joint], transl_pelvis=jts[:, 0], dist=jts[:, 0, 2], dist_postprocessed=dist_pp, v3d=verts,
                      j3d=jts, j2d=j2d, v2d=v2d, loc=loc, offset=offset)
        if has_params:                                                          # train.py:159-166
            rotvec = torch.cat([y[k].reshape(bs, nh, -1, 3) for k in ("smplx_root_pose", "smplx_body_pose", "smplx_left_hand_pose",
                                                                       "smplx_right_hand_pose", "smplx_jaw_pose")], 2)[ib, ih].to(torch.float32).contiguous()
            rotmat = torch.empty(*rotvec.shape, 3, device=dev)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().mhmr_rotvec_to_rotmat(rotvec.data_ptr(), rotvec.numel() // 3, rotmat.data_ptr(),
                                                            torch.cuda.current_stream(dev).cuda_stream), "mhmr_rotvec_to_rotmat")
            target.update(rotvec=rotvec, rotmat=rotmat, shape=y["smplx_shape"].reshape(bs, nh, -1)[ib, ih].to(torch.float32))

        vis = torch.nonzero(visible).reshape(-1)                                # the host learns the count here (train.py:170)
        occluded = torch.nonzero(visible == 0).reshape(-1)
        if occluded.numel():
            valid_h[ib[occluded], ih[occluded]] = 0                             # train.py:153
        out = dict(idx=(ib[vis], pk_idx[vis, 1].long(), pk_idx[vis, 0].long(), torch.zeros_like(ib[vis])), scores=scores, K=y["K"])
        out.update({k: v[vis] for k, v in target.items()})
        return out

    def _project(self, pts, K):
        """utils/camera.py:14-27 for the EHF family, whose vertices do not come from the body kernel."""
        pts = pts.contiguous()
        out = torch.empty(pts.shape[0], pts.shape[1], 2, device=pts.device)
        with torch.cuda.device(pts.device):
            _lib.check(_lib.lib().mhmr_project_points(pts.data_ptr(), K.data_ptr(), int(pts.shape[0]), int(pts.shape[1]), out.data_ptr(),
                                                      torch.cuda.current_stream(pts.device).cuda_stream), "mhmr_project_points")
        return out
