"""Ground-truth body models: what the reference builds with ``smplx.create(SMPLX_DIR, 'smplx', num_betas=11)`` and
``smplx.create(SMPLX_DIR, 'smpl', gender=...)`` (train.py:41-43) and calls in ``prepare_gt`` (train.py:76-109), on ``mhmr_body_forward``
(csrc/bodymodel.hip): the general fp32 layer -- full pose with the global orientation, eye poses, ``transl``, any vertex / joint count.
``Model``'s own SMPL-X layer (csrc/lbs.hip) is the PREDICTION's layer and cannot serve here (f16 correctives, 53 rotations, no transl).

There is no CPU path: calling a ``BodyModel`` with CPU tensors raises."""
from __future__ import annotations

import ctypes as C
import os
import pickle
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .constants import SMPL_EXTRA_JOINT_VERTS, SMPL_NUM_JOINTS, SMPLX_EXTRA_JOINT_VERTS, SMPLX_NUM_JOINTS

VERTEX_TILE = 64          # csrc/body_shared.h VT
PERSON_GROUP = 8          # csrc/body_shared.h PG


def _dense(a):
    """numpy array of a model-file entry: scipy-sparse matrices (J_regressor of the SMPL pickles) and array wrappers with ``.r``."""
    if hasattr(a, "toarray"):
        a = a.toarray()
    elif hasattr(a, "r") and not isinstance(a, np.ndarray):
        a = a.r
    return np.asarray(a)


def load_body_data(data) -> dict:
    """A dict is taken as it is; ``.npz`` is read with numpy; anything else is tried as a pickle with the latin-1 encoding the
    python-2 SMPL files need.  The original SMPL pickles hold ``chumpy`` arrays: without that package they cannot be read, and the
    error says what to do instead of a bare ModuleNotFoundError."""
    if isinstance(data, dict):
        return data
    path = os.fspath(data)
    if path.endswith(".npz"):
        return dict(np.load(path, allow_pickle=True))
    try:
        with open(path, "rb") as f:
            out = pickle.load(f, encoding="latin1")
    except ModuleNotFoundError as e:
        if "chumpy" in str(e):
            raise _lib.MhmrError(f"{path} stores chumpy arrays and the chumpy package is not installed: convert the file once to plain "
                                 "numpy (the 'clean_ch' step of the smplx tools, or np.savez of the arrays) and pass that") from e
        raise
    if not isinstance(out, dict):
        raise _lib.MhmrError(f"{path}: expected a pickled dict of model arrays, got {type(out).__name__}")
    return out


class BodyModel:
    """``BodyModel(data, model_type='smplx' | 'smpl', num_betas=..., num_expression_coeffs=10)``; called with smplx's keyword names it
    returns an object with ``.vertices [G, V, 3]`` and ``.joints [G, J + E + L, 3]`` (SMPL-X: 55 + 21 + 51 = 127, SMPL: 24 + 21 = 45).
    Ours, not smplx's: ``K=[G, 3, 3]`` also returns ``.v2d`` / ``.j2d`` (utils/camera.py:14-27) from the same launches.
    ``data`` may carry ``extra_joint_verts`` to override the picked vertex ids of constants.py."""

    def __init__(self, data, model_type: str = "smplx", num_betas: int | None = None, num_expression_coeffs: int = 10):
        if model_type not in ("smplx", "smpl"):
            raise ValueError(f"model_type {model_type!r}: 'smplx' or 'smpl'")
        data = load_body_data(data)
        self.model_type = model_type
        self.num_betas = int(num_betas if num_betas is not None else 10)
        self.num_expression_coeffs = int(num_expression_coeffs) if model_type == "smplx" else 0
        f32 = lambda a: np.ascontiguousarray(_dense(a), dtype=np.float32)
        self.v_template = f32(data["v_template"])
        self.num_vertices = V = int(self.v_template.shape[0])
        self.faces = np.asarray(_dense(data["f"]), dtype=np.int64)
        self.J_regressor = f32(data["J_regressor"])
        self.num_joints = J = int(self.J_regressor.shape[0])
        want = SMPLX_NUM_JOINTS if model_type == "smplx" else SMPL_NUM_JOINTS
        if J != want:
            raise ValueError(f"{model_type}: {want} joints expected, the data has {J}")
        sd = _dense(data["shapedirs"])
        if sd.shape[-1] < self.num_betas:
            raise ValueError(f"num_betas={self.num_betas} but shapedirs has {sd.shape[-1]} directions")
        dirs = [sd[:, :, :self.num_betas]]
        if self.num_expression_coeffs:
            if sd.shape[-1] < 300 + self.num_expression_coeffs:
                raise ValueError("shapedirs holds no expression directions at 300:")
            dirs.append(sd[:, :, 300:300 + self.num_expression_coeffs])
        self.shapedirs = np.ascontiguousarray(np.concatenate(dirs, axis=-1), dtype=np.float32)          # [V, 3, nc]
        pd = _dense(data["posedirs"])
        self.posedirs = np.ascontiguousarray(pd.reshape(V, 3, -1), dtype=np.float32)                    # [V, 3, 9 (J - 1)]
        if self.posedirs.shape[-1] != 9 * (J - 1):
            raise ValueError(f"posedirs: {9 * (J - 1)} correctives expected, got {self.posedirs.shape[-1]}")
        self.lbs_weights = f32(data["weights"])
        parents = np.asarray(_dense(data["kintree_table"]))[0].astype(np.int64).copy()
        parents[0] = -1
        if not all(0 <= int(parents[i]) < i for i in range(1, J)):
            raise ValueError("kintree_table: every joint's parent must come before it")
        self.parents = parents
        default = SMPLX_EXTRA_JOINT_VERTS if model_type == "smplx" else SMPL_EXTRA_JOINT_VERTS
        self.extra_joint_verts = np.asarray(data.get("extra_joint_verts", default), dtype=np.int64).reshape(-1)
        if self.extra_joint_verts.size and not (0 <= self.extra_joint_verts.min() and self.extra_joint_verts.max() < V):
            raise ValueError("extra_joint_verts outside the mesh")
        if model_type == "smplx":
            self.lmk_vidx = self.faces[np.asarray(data["lmk_faces_idx"], dtype=np.int64)]               # [L, 3]
            self.lmk_bary = f32(data["lmk_bary_coords"])
            if not (0 <= self.lmk_vidx.min() and self.lmk_vidx.max() < V):
                raise ValueError("landmark faces outside the mesh")
        else:
            self.lmk_vidx, self.lmk_bary = np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3), dtype=np.float32)
        self.num_out_joints = J + len(self.extra_joint_verts) + len(self.lmk_vidx)
        self._packed: dict = {}
        self._source = None           # keypoint_model(): the model this one was gathered from
        self._keypoint = None         # keypoint_model()'s cached result
        self.vertex_ids = None        # keypoint_model(): ids of the kept vertices in the source model, sorted

    def keypoint_model(self) -> "BodyModel":
        """The model of the OUTPUT JOINTS alone (cached): its vertices are the sorted unique ids of the picked vertices and the landmark
        corners -- all that ``joints`` reads besides the chain -- so ``mhmr_body_forward`` / ``mhmr_body_backward`` run on it as they are
        over at most ``E + 3 L`` vertex columns (SMPL-X: <= 174, padded to 192, instead of 10 496).  ``v_template``, ``shapedirs``,
        ``posedirs`` and the skinning weights are gathered; the picked ids and landmark corners are renumbered; the joint regression
        (``J0``, ``JS``), ``parents`` and the barycentric weights are the source's own.  ``joints`` of the result equal the source's bit
        for bit (a vertex is computed from its own columns only); ``vertices`` are the kept ones, in ``vertex_ids`` order; ``faces`` is
        empty.  A model without picked vertices and landmarks has no keypoint model."""
        if self._keypoint is None:
            ids = np.unique(np.concatenate([self.extra_joint_verts, self.lmk_vidx.reshape(-1)]).astype(np.int64))
            if ids.size == 0:
                raise ValueError("keypoint_model: the model has neither picked-vertex joints nor landmarks")
            km = object.__new__(BodyModel)
            km.__dict__.update(self.__dict__)
            km._packed, km._source, km._keypoint, km.vertex_ids = {}, self, None, ids
            km.v_template, km.shapedirs = np.ascontiguousarray(self.v_template[ids]), np.ascontiguousarray(self.shapedirs[ids])
            km.posedirs, km.lbs_weights = np.ascontiguousarray(self.posedirs[ids]), np.ascontiguousarray(self.lbs_weights[ids])
            km.num_vertices = int(ids.size)
            km.faces, km.J_regressor = np.zeros((0, 3), dtype=np.int64), None
            km.extra_joint_verts = np.searchsorted(ids, self.extra_joint_verts).astype(np.int64)
            km.lmk_vidx = np.searchsorted(ids, self.lmk_vidx).astype(np.int64)
            self._keypoint = km
        return self._keypoint

    def _joint_rest(self):
        """(J0 [J, 3], JS [3 J, nc]) in float64: the rest joints and their shape directions -- of the source, for a gathered model."""
        if self._source is not None:
            return self._source._joint_rest()
        Jr = self.J_regressor.astype(np.float64)
        nc = self.shapedirs.shape[-1]
        return (Jr @ self.v_template.astype(np.float64),
                np.einsum("jv,vkl->jkl", Jr, self.shapedirs.astype(np.float64)).reshape(self.num_joints * 3, nc))

    # ---- constants, once per device
    def _consts(self, device):
        key = (device.type, device.index)
        if key in self._packed:
            return self._packed[key]
        V, J = self.num_vertices, self.num_joints
        Vp = -(-V // VERTEX_TILE) * VERTEX_TILE
        nc = self.shapedirs.shape[-1]
        K = nc + 9 * (J - 1)
        basis = np.zeros((K, 3, Vp), dtype=np.float32)
        basis[:nc, :, :V] = self.shapedirs.transpose(2, 1, 0)
        basis[nc:, :, :V] = self.posedirs.transpose(2, 1, 0)
        vtemp = np.zeros((3, Vp), dtype=np.float32)
        vtemp[:, :V] = self.v_template.T
        J0, JS = self._joint_rest()
        W = np.zeros((J, Vp), dtype=np.float32)
        W[:, :V] = self.lbs_weights.T
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)
        p = dict(vtemp=t(vtemp, torch.float32), basis=t(basis, torch.float32), J0=t(J0.reshape(-1), torch.float32), JS=t(JS, torch.float32),
                 parents=t(self.parents, torch.int32), weights=t(W, torch.float32), extra_idx=t(self.extra_joint_verts, torch.int32),
                 lmk_idx=t(self.lmk_vidx, torch.int32), lmk_bary=t(self.lmk_bary, torch.float32))
        c = _lib.BodyConsts()
        c.V, c.Vp, c.J, c.nc, c.K, c.E, c.L = V, Vp, J, nc, K, len(self.extra_joint_verts), len(self.lmk_vidx)
        for k, v in p.items():
            setattr(c, k, v.data_ptr() if v.numel() else None)
        p["struct"], p["K"], p["nc"] = c, K, nc
        self._packed[key] = p
        return p

    def inverted_list(self):
        """The picked-vertex joints and the landmark corners, inverted for the backward: CSR by vertex -> ``(ptr [V + 1], joint [n],
        weight [n])`` with ``n = E + 3 L``; the entries of a vertex are sorted by output joint (a face that names a vertex twice keeps both
        entries, in corner order), so the order in which a vertex sums what its joints send back is fixed by the model alone."""
        V, J, E = self.num_vertices, self.num_joints, len(self.extra_joint_verts)
        vert = np.concatenate([self.extra_joint_verts, self.lmk_vidx.reshape(-1)]).astype(np.int64)
        joint = np.concatenate([J + np.arange(E), J + E + np.repeat(np.arange(len(self.lmk_vidx)), 3)]).astype(np.int64)
        w = np.concatenate([np.ones(E, dtype=np.float32), self.lmk_bary.reshape(-1)]).astype(np.float32)
        if vert.size and not (0 <= vert.min() and vert.max() < V):
            raise ValueError("inverted list: a picked vertex or landmark corner lies outside the mesh")
        if joint.size and not (J <= joint.min() and joint.max() < self.num_out_joints):
            raise ValueError("inverted list: an output joint outside [J, J + E + L)")
        order = np.lexsort((np.arange(vert.size), joint, vert))                   # by vertex, then joint, then corner
        ptr = np.zeros(V + 1, dtype=np.int32)
        np.cumsum(np.bincount(vert, minlength=V), out=ptr[1:])
        return ptr, joint[order].astype(np.int32), w[order]

    def _bwd_consts(self, device):
        key = ("bwd", device.type, device.index)
        if key not in self._packed:
            ptr, joint, w = self.inverted_list()
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            p = dict(inv_ptr=t(ptr), inv_joint=t(joint), inv_w=t(w))
            bc = _lib.BodyBwdConsts()
            bc.n = int(joint.size)
            for k, v in p.items():
                setattr(bc, k, v.data_ptr() if v.numel() else None)
            p["struct"] = bc
            self._packed[key] = p
        return self._packed[key]

    @property
    def basis_bytes(self) -> int:
        """Bytes of the blend basis one pass of the vertex kernel streams (the roofline's numerator, per 8 persons)."""
        Vp = -(-self.num_vertices // VERTEX_TILE) * VERTEX_TILE
        return (self.shapedirs.shape[-1] + 9 * (self.num_joints - 1)) * 3 * Vp * 4

    @property
    def expression(self):
        """Zeros ``[1, num_expression_coeffs]`` (train.py:108 reads ``smplx_neutral_11.expression``)."""
        return torch.zeros(1, self.num_expression_coeffs)

    def full_pose(self, G, dev, global_orient=None, body_pose=None, jaw_pose=None, leye_pose=None, reye_pose=None, left_hand_pose=None,
                  right_hand_pose=None):
        part = lambda t, n: (torch.zeros(G, n, 3, device=dev) if t is None else t.to(device=dev, dtype=torch.float32).reshape(G, n, 3))
        if self.model_type == "smpl":
            if any(t is not None for t in (jaw_pose, leye_pose, reye_pose, left_hand_pose, right_hand_pose)):
                raise TypeError("SMPL takes global_orient, body_pose, betas and transl only")
            parts = [part(global_orient, 1), part(body_pose, 23)]
        else:
            parts = [part(global_orient, 1), part(body_pose, 21), part(jaw_pose, 1), part(leye_pose, 1), part(reye_pose, 1),
                     part(left_hand_pose, 15), part(right_hand_pose, 15)]
        return torch.cat(parts, dim=1).contiguous()

    @torch.no_grad()
    def __call__(self, global_orient=None, body_pose=None, jaw_pose=None, leye_pose=None, reye_pose=None, left_hand_pose=None,
                 right_hand_pose=None, betas=None, expression=None, transl=None, K=None, **unused):
        given = [t for t in (global_orient, body_pose, betas, transl, jaw_pose, left_hand_pose) if t is not None]
        if not given:
            raise ValueError("BodyModel needs at least one of global_orient, body_pose, betas, transl to know the batch")
        dev = given[0].device
        if dev.type != "cuda":
            raise _lib.MhmrError("BodyModel runs on the HIP device only (no CPU fallback)")
        G = int(given[0].shape[0])
        if self.model_type == "smpl" and expression is not None:
            raise TypeError("SMPL has no expression")
        V, NJ, ne = self.num_vertices, self.num_out_joints, self.num_expression_coeffs
        out = SimpleNamespace(vertices=torch.empty(G, V, 3, device=dev), joints=torch.empty(G, NJ, 3, device=dev), v2d=None, j2d=None)
        if K is not None:
            out.v2d, out.j2d = torch.empty(G, V, 2, device=dev), torch.empty(G, NJ, 2, device=dev)
        if G == 0:
            return out
        p = self._consts(dev)
        pose = self.full_pose(G, dev, global_orient, body_pose, jaw_pose, leye_pose, reye_pose, left_hand_pose, right_hand_pose)
        f = lambda t, n: (torch.zeros(G, n, device=dev) if t is None else t.to(device=dev, dtype=torch.float32).reshape(G, n))
        coef = f(betas, self.num_betas)
        if ne:
            coef = torch.cat([coef, f(expression, ne)], dim=1)
        coef = coef.contiguous()
        tr = None if transl is None else transl.to(device=dev, dtype=torch.float32).reshape(G, 3).contiguous()
        Kc = None if K is None else K.to(device=dev, dtype=torch.float32).reshape(G, 3, 3).contiguous()
        groups = -(-G // PERSON_GROUP)
        ws_F = torch.empty(groups, p["K"], PERSON_GROUP, device=dev)
        ws_A = torch.empty(G, self.num_joints, 12, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mhmr_body_forward(p["struct"], pose.data_ptr(), coef.data_ptr(), _lib.ptr(tr), _lib.ptr(Kc), G, ws_F.data_ptr(),
                                                    ws_A.data_ptr(), out.vertices.data_ptr(), out.joints.data_ptr(), _lib.ptr(out.v2d),
                                                    _lib.ptr(out.j2d), torch.cuda.current_stream(dev).cuda_stream), "mhmr_body_forward")
        return out

    forward = __call__

    def differentiable(self, global_orient=None, body_pose=None, jaw_pose=None, leye_pose=None, reye_pose=None, left_hand_pose=None,
                       right_hand_pose=None, betas=None, expression=None, transl=None, K=None, **unused):
        """``__call__`` attached to autograd: the same keywords, the same namespace and bit for bit the same values, with gradients for
        whichever of the pose, ``betas``, ``expression`` and ``transl`` tensors require them (``mhmr_body_backward``; once differentiable;
        ``K`` gets none).  Assembling the full pose and the coefficient row stays ordinary torch."""
        given = [t for t in (global_orient, body_pose, betas, transl, jaw_pose, left_hand_pose) if t is not None]
        if not given:
            raise ValueError("BodyModel needs at least one of global_orient, body_pose, betas, transl to know the batch")
        dev = given[0].device
        if dev.type != "cuda":
            raise _lib.MhmrError("BodyModel runs on the HIP device only (no CPU fallback)")
        G = int(given[0].shape[0])
        if self.model_type == "smpl" and expression is not None:
            raise TypeError("SMPL has no expression")
        ne = self.num_expression_coeffs
        pose = self.full_pose(G, dev, global_orient, body_pose, jaw_pose, leye_pose, reye_pose, left_hand_pose, right_hand_pose)
        f = lambda t, n: (torch.zeros(G, n, device=dev) if t is None else t.to(device=dev, dtype=torch.float32).reshape(G, n))
        coef = f(betas, self.num_betas)
        if ne:
            coef = torch.cat([coef, f(expression, ne)], dim=1)
        tr = None if transl is None else transl.to(device=dev, dtype=torch.float32).reshape(G, 3)
        Kc = None if K is None else K.detach().to(device=dev, dtype=torch.float32).reshape(G, 3, 3).contiguous()
        res = _BodyFunction.apply(self, pose, coef, tr, Kc)
        return SimpleNamespace(vertices=res[0], joints=res[1], v2d=res[2] if K is not None else None, j2d=res[3] if K is not None else None)


class _BodyFunction(torch.autograd.Function):
    """``mhmr_body_forward`` / ``mhmr_body_backward`` over (full pose, coef, transl).  The forward's workspaces and outputs are saved."""

    @staticmethod
    def forward(ctx, model, pose, coef, transl, K):
        dev, G = pose.device, int(pose.shape[0])
        pose, coef = pose.contiguous(), coef.contiguous()
        transl = None if transl is None else transl.contiguous()
        V, NJ, J = model.num_vertices, model.num_out_joints, model.num_joints
        p = model._consts(dev)
        vertices, joints = torch.empty(G, V, 3, device=dev), torch.empty(G, NJ, 3, device=dev)
        v2d = torch.empty(G, V, 2, device=dev) if K is not None else None
        j2d = torch.empty(G, NJ, 2, device=dev) if K is not None else None
        ws_F = torch.empty(-(-G // PERSON_GROUP), p["K"], PERSON_GROUP, device=dev)
        ws_A = torch.empty(G, J, 12, device=dev)
        if G:
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().mhmr_body_forward(p["struct"], pose.data_ptr(), coef.data_ptr(), _lib.ptr(transl), _lib.ptr(K), G,
                                                        ws_F.data_ptr(), ws_A.data_ptr(), vertices.data_ptr(), joints.data_ptr(), _lib.ptr(v2d),
                                                        _lib.ptr(j2d), torch.cuda.current_stream(dev).cuda_stream), "mhmr_body_forward")
        ctx.model, ctx.has_transl, ctx.has_K = model, transl is not None, K is not None
        ctx.save_for_backward(pose, coef, transl, K, ws_F, ws_A, vertices, joints)
        ctx.set_materialize_grads(False)
        if K is None:                                            # autograd wants tensors: empty stand-ins the caller never sees
            v2d, j2d = vertices.new_empty(0), vertices.new_empty(0)
            ctx.mark_non_differentiable(v2d, j2d)
        return vertices, joints, v2d, j2d

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_vertices, g_joints, g_v2d, g_j2d):
        pose, coef, transl, K, ws_F, ws_A, vertices, joints = ctx.saved_tensors
        model, dev, G = ctx.model, pose.device, int(pose.shape[0])
        if not ctx.has_K:
            g_v2d = g_j2d = None
        cot = [None if t is None else t.to(dtype=torch.float32).contiguous() for t in (g_vertices, g_joints, g_v2d, g_j2d)]
        need = ctx.needs_input_grad                                # (model, pose, coef, transl, K)
        g_pose = torch.empty_like(pose) if need[1] else None
        g_coef = torch.empty_like(coef) if need[2] else None
        g_transl = torch.empty_like(transl) if ctx.has_transl and need[3] else None
        if G and any(t is not None for t in (g_pose, g_coef, g_transl)):
            p, pb = model._consts(dev), model._bwd_consts(dev)
            lib = _lib.lib()
            nbytes = _lib.workspace_bytes("mhmr_body_backward_workspace_bytes", p["struct"], G)
            ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
            d = _lib.BodyBackwardDesc()
            d.c, d.bc, d.G = C.pointer(p["struct"]), C.pointer(pb["struct"]), G
            for name, t in (("pose", pose), ("coef", coef if coef.numel() else None), ("transl", transl), ("K", K), ("ws_F", ws_F), ("ws_A", ws_A),
                            ("vertices", vertices), ("joints", joints), ("g_vertices", cot[0]), ("g_joints", cot[1]), ("g_v2d", cot[2]),
                            ("g_j2d", cot[3]), ("g_pose", g_pose), ("g_coef", g_coef if coef.numel() else None), ("g_transl", g_transl),
                            ("workspace", ws)):
                setattr(d, name, _lib.ptr(t))
            d.workspace_bytes = nbytes
            with torch.cuda.device(dev):
                _lib.check(lib.mhmr_body_backward(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "mhmr_body_backward")
        return None, g_pose, g_coef, g_transl, None
