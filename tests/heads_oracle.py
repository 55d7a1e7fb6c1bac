"""TEST INFRASTRUCTURE for the differentiable prediction decode (multi_hmr_amd/heads.py, csrc/heads_bwd.hip).

The function read-out -> training-mode outputs restated in torch on the CPU, parametrised by dtype and differentiated by autograd:
``oracle.roma_ref`` (special_gramschmidt, rotmat_to_rotvec), the 53 -> 55 pose placement of the reference's SMPL_Layer.forward
(blocks/smpl_layer.py:86-101), ``gt_oracle.OracleBody`` (the fp32 body layer's function: the root rotation applied about the rest
pelvis), the recentring on the person centre (:128-136), the inverse and the forward projection (utils/camera.py:14-48) and the distance
chain (utils/camera.py:71-90, the clamp to [0, 50]).  float64 is the reference value; float32 is the yardstick of the 4x rule.

It also reports the discrete choices the evaluation made for every (person, joint): the quaternion branch (0, 1, 2 = the largest
diagonal entry, 3 = the trace), the sign flip (w < 0), the small-angle series, and per person the side of the clamp (-1, 0, +1)."""
import math

import torch

import gt_oracle as go
from oracle import roma_ref

PATCH = 14
KEYS = ("offset", "loc", "rotmat", "rotvec", "shape", "expression", "dist_postprocessed", "dist", "v3d", "v2d", "j3d", "j2d", "transl",
        "transl_pelvis")
KEYS_2D = ("v2d", "j2d")


def pose53_to_55(rotvec):
    """root, body 1:22, jaw 52, eyes zero, left hand 22:37, right hand 37:52 -- written out by index, not with the package's helper."""
    P = rotvec.shape[0]
    out = torch.zeros(P, 55, 3, dtype=rotvec.dtype)
    src = list(range(0, 22)) + [52] + list(range(22, 52))
    dst = list(range(0, 22)) + [22] + list(range(25, 55))
    out[:, dst] = rotvec[:, src]
    return out


def focal_norm(img_size, fovn=60):
    return img_size / (2 * math.tan(math.radians(fovn) / 2))


def choices(rotmat):
    """rotmat [..., 3, 3] (detached) -> dict of the discrete choices of roma_ref.rotmat_to_rotvec."""
    m = rotmat.detach().reshape(-1, 3, 3)
    dec = torch.cat([m.diagonal(dim1=1, dim2=2), m.diagonal(dim1=1, dim2=2).sum(1, keepdim=True)], 1)
    q = roma_ref.rotmat_to_unitquat(m)
    flip = q[:, 3] < 0
    angle = 2 * torch.atan2(q[:, :3].norm(dim=1), q[:, 3].abs())
    shp = rotmat.shape[:-2]
    return dict(branch=dec.argmax(1).reshape(shp), flip=flip.reshape(shp), small=(angle.abs() <= 1e-3).reshape(shp))


def decode(readout, offset, idx, K, body, *, nb, img_size, nearness=True, center=15, dtype=torch.float64):
    """readout [P, 318 + nb + 13], offset [P, 2] (leaves of ``dtype`` or anything convertible), idx = (image, y, x), K [B, 3, 3], body a
    ``gt_oracle.OracleBody`` of the same dtype -> (dict of the fourteen outputs, report of the discrete choices)."""
    P = readout.shape[0]
    r, off, K = readout.to(dtype), offset.to(dtype), K.to(dtype)
    b, y, x = (i.long() for i in idx[:3])                        # (a fourth entry, as GroundTruth.prepare returns it, is not read)
    rotmat = roma_ref.special_gramschmidt(r[:, :318].reshape(P, 53, 2, 3).transpose(-1, -2))
    rotvec = roma_ref.rotmat_to_rotvec(rotmat)
    shape, cam0, expr = r[:, 318:318 + nb], r[:, 318 + nb], r[:, 318 + nb + 3:]
    d = cam0 * (K[b, 0, 0] / focal_norm(img_size))
    if nearness:
        d = torch.exp(d) - 1e-10
    dist = torch.clamp(d, 0.0, 50.0)
    loc = (torch.stack([x, y], 1).to(dtype) + 0.5 + off) * PATCH
    v, j = body(pose53_to_55(rotvec), torch.cat([shape, expr], 1), None)
    Kp = K[b]
    pts = torch.cat([loc, torch.ones(P, 1, dtype=dtype)], 1)
    transl = torch.einsum("bij,bj->bi", torch.inverse(Kp), pts) * dist[:, None]
    if center is not None and center >= 0:
        c = j[:, [center]]
        v, j = v - c, j - c
    v3d, j3d = v + transl[:, None], j + transl[:, None]
    out = dict(offset=off, loc=loc, rotmat=rotmat, rotvec=rotvec, shape=shape, expression=expr, dist_postprocessed=cam0[:, None],
               dist=dist[:, None], v3d=v3d, v2d=go.perspective_projection(v3d, Kp), j3d=j3d, j2d=go.perspective_projection(j3d, Kp),
               transl=transl, transl_pelvis=j3d[:, 0:1])
    report = choices(rotmat)
    dd = d.detach()
    report["clamp"] = (dd > 50).long() - (dd < 0).long()
    report["in_front"] = bool((v3d.detach()[..., 2] > 0).all() and (j3d.detach()[..., 2] > 0).all())
    return out, report


def grads(readout, offset, idx, K, body, cot, dtype, **kw):
    """Gradient of sum(cotangent * output) over the outputs named in ``cot`` -> (g_readout, g_offset, report), in ``dtype``."""
    r, o = readout.detach().to(dtype).requires_grad_(), offset.detach().to(dtype).requires_grad_()
    out, report = decode(r, o, idx, K, body, dtype=dtype, **kw)
    s = sum((out[k] * c.to(dtype)).sum() for k, c in cot.items())
    g = torch.autograd.grad(s, [r, o], allow_unused=True)
    return (torch.zeros_like(r) if g[0] is None else g[0]), (torch.zeros_like(o) if g[1] is None else g[1]), report


def same_choices(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("branch", "flip", "small", "clamp"))


def make_cotangents(P, V, img_size, seed, use=KEYS, nb=10):
    """Seeded cotangents: N(0, 1) on the 3D and parameter outputs, N(0, 1) / img_size on the 2D ones."""
    g = torch.Generator().manual_seed(seed)
    shapes = dict(offset=(2,), loc=(2,), rotmat=(53, 3, 3), rotvec=(53, 3), shape=(nb,), expression=(10,), dist_postprocessed=(1,), dist=(1,),
                  v3d=(V, 3), v2d=(V, 2), j3d=(127, 3), j2d=(127, 2), transl=(3,), transl_pelvis=(1, 3))
    full = {k: torch.randn(P, *shapes[k], generator=g) / (img_size if k in KEYS_2D else 1.0) for k in KEYS}
    return {k: v for k, v in full.items() if k in use}


def make_inputs(init, P, B, G, img_size, seed, nearness=True, depth=(3.0, 8.0), general_K=False):
    """Seeded read-outs init + N(0, 0.3) with the distance entry set so that the person stands ``depth`` metres away, offsets in
    (-0.5, 0.5), cells and images, cameras -> readout [P, W], offset [P, 2], idx, K [B, 3, 3] (all fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    W = init.numel()
    nb = W - 318 - 13
    readout = init.reshape(1, W).float() + 0.3 * torch.randn(P, W, generator=g)
    offset = torch.rand(P, 2, generator=g) - 0.5
    b = torch.sort(torch.randint(0, B, (P,), generator=g)).values
    lo, hi = G // 4, G - G // 4                                   # cells near the image centre: the whole body in front of the camera
    y, x = torch.randint(lo, hi, (P,), generator=g), torch.randint(lo, hi, (P,), generator=g)
    K = go.camera_K(img_size, B, g)
    if general_K:
        K[:, 1, 1] = K[:, 0, 0] * 1.23
        K[:, 0, 2], K[:, 1, 2] = img_size * 0.41, img_size * 0.57
        K[:, 0, 1] = 0.7                                          # a skew: the inverse is a general 3x3
    dist = depth[0] + (depth[1] - depth[0]) * torch.rand(P, generator=g)
    scale = K[b, 0, 0] / focal_norm(img_size)
    readout[:, 318 + nb] = (torch.log(dist) if nearness else dist) / scale
    return readout, offset, (b, y, x), K
