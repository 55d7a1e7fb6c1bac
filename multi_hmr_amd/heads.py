"""Differentiable prediction decode: from the HPH read-out row ``[pose6d 318 | betas nb | cam 3 | expr 10]`` and the
2-vector of ``mlp_offset`` to the training-mode outputs of ``Model``, attached to autograd with respect to both.

Forward: ``mhmr_heads_decode`` (the decode + loc kernels of ``mhmr_hph_forward``) + ``mhmr_lbs_forward`` -- the kernels ``Model`` itself runs,
so the values are bit-equal to ``model(x, idx, K, is_training=True)`` for that call's read-out and offset.
Backward: the fp32 body model (``mhmr_body_forward`` on a lazily built ``BodyModel``) without placement, ``mhmr_heads_place_backward``,
``mhmr_body_backward`` with the two 3D cotangents, ``mhmr_heads_decode_backward``.  The fp32 body forward runs at BACKWARD time: a forward
that is never differentiated costs what it costs today.

The gradient is that of the fp32 layer of DESIGN section 16 at the same parameters; the returned meshes are ``lbs.hip``'s, which differ
from that layer by at most the 5e-5 m of section 5.

There is no CPU path: CPU tensors raise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .bodymodel import PERSON_GROUP
from .model import PATCH

#: the tensors of the training-mode dict that depend on the read-out, in ``Model.OUTPUT_SHAPES`` order (``transl_pelvis`` is a slice of j3d)
DECODE_KEYS = ("offset", "loc", "rotmat", "rotvec", "shape", "expression", "dist_postprocessed", "dist", "v3d", "v2d", "j3d", "j2d", "transl")
NROT = 53


def pose53_to_55(rotvec: torch.Tensor) -> torch.Tensor:
    """The 53 predicted rotations in the SMPL-X layer's 55-joint order (reference blocks/smpl_layer.py:86-101): root, body 1:22, jaw 52,
    the two eyes zero, left hand 22:37, right hand 37:52."""
    P = rotvec.shape[0]
    return torch.cat([rotvec[:, 0:22], rotvec[:, 52:53], rotvec.new_zeros(P, 2, 3), rotvec[:, 22:52]], dim=1)


def pose55_to_53(g_pose: torch.Tensor) -> torch.Tensor:
    """The transpose of ``pose53_to_55``: the eye rows are dropped."""
    return torch.cat([g_pose[:, 0:22], g_pose[:, 25:55], g_pose[:, 22:23]], dim=1)


def readout_width(num_betas: int) -> int:
    return 6 * NROT + int(num_betas) + 3 + 10


def _settings(model):
    return int(bool(model.nearness)), float(model.img_size / (2 * np.tan(np.radians(model.fovn) / 2)))


class _DecodeFunction(torch.autograd.Function):
    """(readout, offset) -> the 13 tensors of DECODE_KEYS; det [3, P] int32 and K [B, 3, 3] are constants."""

    @staticmethod
    def forward(ctx, model, readout, offset, det, K):
        dev, Pn = readout.device, int(readout.shape[0])
        readout, offset = readout.contiguous(), offset.contiguous()
        packed = model._packed_for(dev)
        nb, lb = packed["hph"]["nb"], packed["lbs"]
        V = lb["V"]
        shapes = dict(model._output_shapes(packed))
        o = {n: torch.empty(Pn, *shapes[n], dtype=torch.float32, device=dev) for n in DECODE_KEYS if n != "offset"}
        o["offset"] = offset.clone()
        if Pn:
            L = _lib.lib()
            nearness, fn = _settings(model)
            stream = torch.cuda.current_stream(dev).cuda_stream
            d = _lib.HeadsDecodeDesc()
            d.P, d.nb, d.ldr, d.patch, d.nearness, d.fn = Pn, nb, int(readout.shape[1]), PATCH, nearness, fn
            for n, t in (("readout", readout), ("offset", offset), ("K", K), ("det_b", det[0]), ("det_y", det[1]), ("det_x", det[2]),
                         ("loc", o["loc"]), ("rotmat", o["rotmat"]), ("rotvec", o["rotvec"]), ("shape", o["shape"]), ("expression", o["expression"]),
                         ("dist_postprocessed", o["dist_postprocessed"]), ("dist", o["dist"])):
                setattr(d, n, t.data_ptr())
            with torch.cuda.device(dev):
                _lib.check(L.mhmr_heads_decode(C.byref(d), stream), "mhmr_heads_decode")
                model._lbs(packed, o, K, det[0], Pn, stream)
        ctx.model, ctx.nb, ctx.V = model, nb, V
        ctx.center = int(lb["center_joint"])
        ctx.save_for_backward(readout, offset, det, K, o["rotvec"], o["shape"], o["expression"], o["transl"])
        ctx.set_materialize_grads(False)
        return tuple(o[n] for n in DECODE_KEYS)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *cot):
        readout, offset, det, K, rotvec, shape, expression, transl = ctx.saved_tensors
        model, nb, V, dev, Pn = ctx.model, ctx.nb, ctx.V, readout.device, int(readout.shape[0])
        g = {n: (None if t is None else t.to(dtype=torch.float32).contiguous()) for n, t in zip(DECODE_KEYS, cot)}
        g_readout = torch.empty(Pn, readout_width(nb), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        g_offset = torch.empty(Pn, 2, dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] else None
        if Pn == 0 or (g_readout is None and g_offset is None):
            return None, g_readout, g_offset, None, None
        if g_readout is None:                                     # the kernel writes both
            g_readout = torch.empty(Pn, readout_width(nb), dtype=torch.float32, device=dev)
        if g_offset is None:
            g_offset = torch.empty(Pn, 2, dtype=torch.float32, device=dev)
        L = _lib.lib()
        nearness, fn = _settings(model)
        stream = torch.cuda.current_stream(dev).cuda_stream
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        g_transl_total, g_rot = g["transl"], g["rotvec"]
        g_shape, g_expr = g["shape"], g["expression"]
        with torch.cuda.device(dev):
            if any(g[n] is not None for n in ("v3d", "j3d", "v2d", "j2d")):
                # 1. the fp32 body model at the predicted parameters, unplaced
                body = model._body_model()
                p, pb = body._consts(dev), body._bwd_consts(dev)
                NJ, J = body.num_out_joints, body.num_joints
                pose = pose53_to_55(rotvec).contiguous()
                coef = torch.cat([shape, expression], dim=1).contiguous()
                U, UJ = f(Pn, V, 3), f(Pn, NJ, 3)
                ws_F, ws_A = f(-(-Pn // PERSON_GROUP), p["K"], PERSON_GROUP), f(Pn, J, 12)
                _lib.check(L.mhmr_body_forward(p["struct"], pose.data_ptr(), coef.data_ptr(), None, None, Pn, ws_F.data_ptr(), ws_A.data_ptr(),
                                               U.data_ptr(), UJ.data_ptr(), None, None, stream), "mhmr_body_forward")
                # 2. placement backward: recentring, transl, projection
                nbytes = _lib.workspace_bytes("mhmr_heads_place_workspace_bytes", V, NJ, Pn)
                ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
                gx_v, gx_j, g_transl_total = f(Pn, V, 3), f(Pn, NJ, 3), f(Pn, 3)
                d = _lib.HeadsPlaceDesc()
                d.P, d.V, d.NJ, d.center_joint = Pn, V, NJ, ctx.center
                for n, t in (("verts_u", U), ("joints_u", UJ), ("transl", transl), ("K", K), ("det_b", det[0]), ("g_v3d", g["v3d"]), ("g_j3d", g["j3d"]),
                             ("g_v2d", g["v2d"]), ("g_j2d", g["j2d"]), ("g_transl", g["transl"]), ("gx_v", gx_v), ("gx_j", gx_j),
                             ("g_transl_total", g_transl_total), ("workspace", ws)):
                    setattr(d, n, _lib.ptr(t))
                d.workspace_bytes = nbytes
                _lib.check(L.mhmr_heads_place_backward(C.byref(d), stream), "mhmr_heads_place_backward")
                # 3. body backward with the two 3D cotangents
                nbytes = _lib.workspace_bytes("mhmr_body_backward_workspace_bytes", p["struct"], Pn)
                ws2 = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
                g_pose, g_coef = f(Pn, J, 3), f(Pn, nb + 10)
                b = _lib.BodyBackwardDesc()
                b.c, b.bc, b.G = C.pointer(p["struct"]), C.pointer(pb["struct"]), Pn
                for n, t in (("pose", pose), ("coef", coef), ("ws_F", ws_F), ("ws_A", ws_A), ("vertices", U), ("joints", UJ), ("g_vertices", gx_v),
                             ("g_joints", gx_j), ("g_pose", g_pose), ("g_coef", g_coef), ("workspace", ws2)):
                    setattr(b, n, t.data_ptr())
                b.workspace_bytes = nbytes
                _lib.check(L.mhmr_body_backward(C.byref(b), stream), "mhmr_body_backward")
                # 4. the eye rows are dropped; the caller's own cotangents join
                g53 = pose55_to_53(g_pose)
                g_rot = g53.contiguous() if g_rot is None else (g_rot + g53).contiguous()
                g_shape = g_coef[:, :nb].contiguous() if g_shape is None else (g_shape + g_coef[:, :nb]).contiguous()
                g_expr = g_coef[:, nb:].contiguous() if g_expr is None else (g_expr + g_coef[:, nb:]).contiguous()
            # 5. decode backward
            e = _lib.HeadsDecodeBackwardDesc()
            e.P, e.nb, e.ldr, e.patch, e.nearness, e.fn = Pn, nb, int(readout.shape[1]), PATCH, nearness, fn
            for n, t in (("readout", readout), ("offset", offset), ("K", K), ("det_b", det[0]), ("det_y", det[1]), ("det_x", det[2]),
                         ("g_rotmat", g["rotmat"]), ("g_rotvec", g_rot), ("g_shape", g_shape), ("g_expression", g_expr), ("g_dist", g["dist"]),
                         ("g_dist_postprocessed", g["dist_postprocessed"]), ("g_transl", g_transl_total), ("g_loc", g["loc"]),
                         ("g_offset_direct", g["offset"]), ("g_readout", g_readout), ("g_offset", g_offset)):
                setattr(e, n, _lib.ptr(t))
            _lib.check(L.mhmr_heads_decode_backward(C.byref(e), stream), "mhmr_heads_decode_backward")
        return None, (g_readout if ctx.needs_input_grad[1] else None), (g_offset if ctx.needs_input_grad[2] else None), None, None


def decode_readout(model, readout, offset, idx, K):
    """``Model.decode_readout``: see there."""
    if not (readout.is_cuda and offset.is_cuda):
        raise _lib.MhmrError("Model.decode_readout runs on the HIP device only (no CPU fallback)")
    dev = readout.device
    nb = model._packed_for(dev)["hph"]["nb"]
    Pn = int(readout.shape[0])
    if readout.dim() != 2 or readout.shape[1] != readout_width(nb) or tuple(offset.shape) != (Pn, 2):
        raise ValueError(f"readout must be [P, {readout_width(nb)}] and offset [P, 2]")
    idx = tuple(i.to(dev) for i in idx)
    if any(int(i.shape[0]) != Pn for i in idx[:3]):
        raise ValueError("idx must hold one (image, y, x) triple per read-out row")
    det = (torch.stack([idx[0], idx[1], idx[2]]).to(torch.int32) if Pn else torch.zeros(3, 0, dtype=torch.int32, device=dev)).contiguous()
    K = K.detach().to(device=dev, dtype=torch.float32).contiguous()
    with model._lock, torch.autocast("cuda", enabled=False):
        res = _DecodeFunction.apply(model, readout.to(torch.float32), offset.to(torch.float32), det, K)
    out = dict(zip(DECODE_KEYS, res))
    out["transl_pelvis"] = out["j3d"][:, 0:1]          # outside the function: its cotangent folds into g_j3d
    return out


__all__ = ["DECODE_KEYS", "decode_readout", "pose53_to_55", "pose55_to_53", "readout_width"]
