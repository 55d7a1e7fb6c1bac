"""Fit the predicted persons to 2D keypoints (``mhmr_fit_keypoints``, csrc/fit.hip).

``KeypointFitter(model).fit(readout, offset, idx, K, keypoints, confidence)`` refines the HPH read-out rows and offsets of P persons with
Adam against a detector's 2D keypoints (OpenPose / COCO / whole-body), anchored to the network's own prediction by quadratic priors.  The
whole loop -- decode, the keypoint body model (``BodyModel.keypoint_model()``: the <= 174 vertices the 127 output joints read, not the
mesh), the objective, the three backwards and the optimiser step -- is enqueued by ONE library call; nothing is driven from Python per
iteration.  The refined meshes come from ``model.decode_readout(result.readout, result.offset, idx, K)``.

The rows to start from are what ``model(x, K=K, return_batched=True, return_readout=True)`` returns under ``readout``, ``offset`` and
``idx`` (inference), or the training-mode dict's ``readout`` / ``offset``.

There is no CPU path: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from . import _lib
from .constants import SMPLX_JOINT_NAMES
from .heads import _settings, readout_width
from .model import PATCH

#: the 17 COCO keypoints, in COCO's order, by their SMPL-X joint names
COCO17 = ("nose", "left_eye", "right_eye", "left_ear", "right_ear", "left_shoulder", "right_shoulder", "left_elbow", "right_elbow",
          "left_wrist", "right_wrist", "left_hip", "right_hip", "left_knee", "right_knee", "left_ankle", "right_ankle")
#: the 25 OpenPose BODY_25 keypoints, in OpenPose's order (MidHip = pelvis)
OPENPOSE_BODY25 = ("nose", "neck", "right_shoulder", "right_elbow", "right_wrist", "left_shoulder", "left_elbow", "left_wrist", "pelvis",
                   "right_hip", "right_knee", "right_ankle", "left_hip", "left_knee", "left_ankle", "right_eye", "left_eye", "right_ear",
                   "left_ear", "left_big_toe", "left_small_toe", "left_heel", "right_big_toe", "right_small_toe", "right_heel")
#: groups of read-out / offset columns that ``optimize`` and ``weights`` name
GROUPS = ("pose", "shape", "depth", "expression", "loc")


def joint_indices(names) -> list:
    """Rows of the 127 output joints for a detector's joint names; an unknown or repeated name raises ``ValueError``."""
    names = list(names)
    unknown = [n for n in names if n not in SMPLX_JOINT_NAMES]
    if unknown:
        raise ValueError(f"unknown joint names {unknown}: the names are those of multi_hmr_amd.constants.SMPLX_JOINT_NAMES")
    if len(set(names)) != len(names):
        raise ValueError("a joint name is given twice")
    return [SMPLX_JOINT_NAMES.index(n) for n in names]


for _table in (COCO17, OPENPOSE_BODY25):
    assert len(joint_indices(_table)) == len(_table)


def keypoints_by_name(names, xy: torch.Tensor, conf: torch.Tensor):
    """A detector's layout scattered into the model's: ``names`` (n joint names, e.g. ``COCO17``), ``xy [P, n, 2]`` in pixels and ``conf
    [P, n]`` -> ``(keypoints [P, 127, 2], confidence [P, 127])`` with confidence 0 (= not given) for every joint nobody names."""
    rows = joint_indices(names)
    n = len(rows)
    if xy.dim() != 3 or tuple(xy.shape[1:]) != (n, 2) or tuple(conf.shape) != (xy.shape[0], n):
        raise ValueError(f"xy must be [P, {n}, 2] and conf [P, {n}] for {n} names")
    Pn, NJ = int(xy.shape[0]), len(SMPLX_JOINT_NAMES)
    kp = torch.zeros(Pn, NJ, 2, dtype=torch.float32, device=xy.device)
    c = torch.zeros(Pn, NJ, dtype=torch.float32, device=xy.device)
    at = torch.tensor(rows, dtype=torch.long, device=xy.device)
    kp[:, at] = xy.to(torch.float32)
    c[:, at] = conf.to(device=xy.device, dtype=torch.float32)
    return kp, c


class FitResult(NamedTuple):
    readout: torch.Tensor       # [P, 318 + num_betas + 13] the refined rows (new tensor)
    offset: torch.Tensor        # [P, 2]
    objective: torch.Tensor     # [steps + 1, P] E_p at every iterate, the last included
    state: dict                 # exp_avg, exp_avg_sq [P, D + 2], step, readout0, offset0: pass as ``state=`` to continue


class KeypointFitter:
    """``KeypointFitter(model, sigma=100.0, robust="gmof", weights=dict(pose=, shape=, depth=, expression=, loc=), optimize=("pose", "shape",
    "depth", "loc"), lr=0.01, betas=(0.9, 0.999), eps=1e-8)``.

    ``sigma`` (pixels) scales the residual; ``robust`` is ``"gmof"`` (Geman-McClure, ``s / (1 + s)``) or ``"l2"``; ``weights`` are the
    lambdas of the quadratic priors that hold each group to the network's prediction (missing groups: the defaults); ``optimize`` names
    the groups Adam may move -- ``pose`` the 318 6D numbers, ``shape`` the betas, ``depth`` ``cam[0]``, ``expression``, ``loc`` the offset
    -- a group that is not named keeps its bits."""

    DEFAULT_WEIGHTS = dict(pose=1.0, shape=0.1, depth=0.0, expression=0.1, loc=0.0)

    def __init__(self, model, sigma: float = 100.0, robust: str = "gmof", weights: dict | None = None,
                 optimize=("pose", "shape", "depth", "loc"), lr: float = 0.01, betas=(0.9, 0.999), eps: float = 1e-8):
        if robust not in _lib.FIT_ROBUST:
            raise ValueError(f"robust must be one of {sorted(_lib.FIT_ROBUST)}, not {robust!r}")
        weights = dict(weights or {})
        bad = [k for k in list(weights) + list(optimize) if k not in GROUPS]
        if bad:
            raise ValueError(f"unknown groups {bad}: the groups are {GROUPS}")
        if not sigma > 0:
            raise ValueError("sigma must be positive")
        self.model, self.sigma, self.robust = model, float(sigma), robust
        self.weights = {**self.DEFAULT_WEIGHTS, **{k: float(v) for k, v in weights.items()}}
        self.optimize = tuple(optimize)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self._ws: dict = {}           # (P, device) -> workspace
        self._mask: dict = {}         # device -> column mask

    def column_mask(self, nb: int) -> torch.Tensor:
        """The 0/1 mask over ``[pose6d 318 | betas nb | cam 3 | expr 10 | offset 2]`` that ``optimize`` selects (``cam[1:3]``, which nothing
        reads, are never selected) -- CPU float32."""
        m = torch.zeros(readout_width(nb) + 2)
        spans = dict(pose=(0, 318), shape=(318, 318 + nb), depth=(318 + nb, 318 + nb + 1), expression=(318 + nb + 3, 318 + nb + 13),
                     loc=(318 + nb + 13, 318 + nb + 15))
        for g in self.optimize:
            m[spans[g][0]:spans[g][1]] = 1.0
        return m

    def _workspace(self, body_struct, Pn, dev):
        key = (Pn, dev.type, dev.index)
        if key not in self._ws:
            nbytes = _lib.workspace_bytes("mhmr_fit_keypoints_workspace_bytes", body_struct, Pn)
            self._ws[key] = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
        return self._ws[key]

    @torch.no_grad()
    def fit(self, readout, offset, idx, K, keypoints, confidence, steps: int = 50, state: dict | None = None, return_grad: bool = False):
        """``readout [P, 318 + num_betas + 13]``, ``offset [P, 2]``, ``idx`` the (image, y, x) of every person, ``K [B, 3, 3]``,
        ``keypoints [P, 127, 2]`` (pixels), ``confidence [P, 127]`` (>= 0; 0 = not given: its target is never read) ->
        ``FitResult``.  The inputs are not modified.  ``steps=0`` evaluates only.  ``state`` (a previous result's) continues that
        run: its moments, step count and anchors -- ``fit(steps=30)`` equals ``fit(steps=10)`` followed by ``fit(steps=20, state=...)`` bit
        for bit.  ``return_grad=True`` returns ``(FitResult, grad [P, D + 2])``: the masked gradient at the last iterate."""
        model = self.model
        if not (readout.is_cuda and offset.is_cuda):
            raise _lib.MhmrError("KeypointFitter.fit runs on the HIP device only (no CPU fallback)")
        steps = int(steps)
        if steps < 0:
            raise ValueError("steps must be >= 0")
        dev = readout.device
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        with model._lock, torch.autocast("cuda", enabled=False), torch.cuda.device(dev):
            packed = model._packed_for(dev)
            nb, Pn = packed["hph"]["nb"], int(readout.shape[0])
            W = readout_width(nb)
            body = model._body_model().keypoint_model()
            NJ = body.num_out_joints
            if readout.dim() != 2 or readout.shape[1] != W or tuple(offset.shape) != (Pn, 2):
                raise ValueError(f"readout must be [P, {W}] and offset [P, 2]")
            if tuple(keypoints.shape) != (Pn, NJ, 2) or tuple(confidence.shape) != (Pn, NJ):
                raise ValueError(f"keypoints must be [P, {NJ}, 2] and confidence [P, {NJ}]")
            idx = tuple(i.to(dev) for i in idx)
            if any(int(i.shape[0]) != Pn for i in idx[:3]):
                raise ValueError("idx must hold one (image, y, x) triple per read-out row")
            r0, o0 = f32(readout), f32(offset)
            if state is None:
                m, v = torch.zeros(Pn, W + 2, device=dev), torch.zeros(Pn, W + 2, device=dev)
                step0, a_r, a_o = 0, r0, o0
            else:
                m, v, step0 = state["exp_avg"].clone(), state["exp_avg_sq"].clone(), int(state["step"])
                a_r, a_o = state["readout0"], state["offset0"]
                if tuple(m.shape) != (Pn, W + 2) or tuple(v.shape) != (Pn, W + 2) or tuple(a_r.shape) != (Pn, W) or tuple(a_o.shape) != (Pn, 2):
                    raise ValueError("state belongs to another set of persons")
            r, o = r0.clone(), o0.clone()
            objective = torch.empty(steps + 1, Pn, dtype=torch.float32, device=dev)
            grad = torch.empty(Pn, W + 2, dtype=torch.float32, device=dev) if return_grad else None
            new_state = dict(exp_avg=m, exp_avg_sq=v, step=step0 + steps, readout0=a_r, offset0=a_o)
            if Pn:
                det = torch.stack([idx[0], idx[1], idx[2]]).to(torch.int32).contiguous()
                Kd, kp, cf = f32(K), f32(keypoints), f32(confidence)
                p, pb = body._consts(dev), body._bwd_consts(dev)
                mkey = (dev.type, dev.index)
                if mkey not in self._mask:
                    self._mask[mkey] = self.column_mask(nb).to(dev)
                ws = self._workspace(p["struct"], Pn, dev)
                nearness, fn = _settings(model)
                d = _lib.FitDesc()
                d.c, d.bc = C.pointer(p["struct"]), C.pointer(pb["struct"])
                d.P, d.nb, d.ldr, d.patch, d.nearness, d.center_joint, d.fn = Pn, nb, W, PATCH, nearness, int(packed["lbs"]["center_joint"]), fn
                for n, t in (("readout", r), ("offset", o), ("readout0", a_r), ("offset0", a_o), ("det_b", det[0]), ("det_y", det[1]),
                             ("det_x", det[2]), ("K", Kd), ("keypoints", kp), ("confidence", cf), ("mask", self._mask[mkey]), ("exp_avg", m),
                             ("exp_avg_sq", v), ("objective", objective), ("grad", grad), ("workspace", ws)):
                    setattr(d, n, _lib.ptr(t))
                d.sigma, d.robust = self.sigma, _lib.FIT_ROBUST[self.robust]
                w = self.weights
                d.lambda_pose, d.lambda_shape, d.lambda_depth, d.lambda_expr, d.lambda_loc = (w["pose"], w["shape"], w["depth"], w["expression"],
                                                                                             w["loc"])
                d.steps, d.step0, d.lr, d.beta1, d.beta2, d.eps = steps, step0, self.lr, self.betas[0], self.betas[1], self.eps
                d.workspace_bytes = ws.numel() * 8
                _lib.check(_lib.lib().mhmr_fit_keypoints(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "mhmr_fit_keypoints")
        res = FitResult(r, o, objective, new_state)
        return (res, grad) if return_grad else res


__all__ = ["COCO17", "OPENPOSE_BODY25", "FitResult", "KeypointFitter", "joint_indices", "keypoints_by_name"]
