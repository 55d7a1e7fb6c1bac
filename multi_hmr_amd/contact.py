"""How the persons of an image relate in 3D: per vertex the signed distance to the nearest OTHER person's surface (negative inside
it), the closest point, per person the penetration depth and the inside / contact vertex counts, per ordered pair the smallest signed
distance, all on the GPU (``csrc/contact.hip``).  The contract -- which pairs and vertices are evaluated, the closest point, the winding
number, the sign, the empty values, the determinism -- is stated once, in include/mhmr.h at ``mhmr_contact_desc``; this module adds the
tensor handling and ``penetration_loss``.  There is no CPU path and nothing is copied to the host.
"""
from __future__ import annotations

import ctypes as C
import hashlib
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from .maps import _strided
from .render import _workspace

#: faces per LDS tile of the kernel: the face counts at which its tiling changes (for tests)
FACE_TILE = _lib.CONTACT_FACE_TILE
FIELDS = ("sdf", "nearest_person", "nearest_face", "closest", "penetration_depth", "inside_count", "contact_count", "pair_distance",
          "pair_inside", "aabb", "valid")


class Contacts(NamedTuple):
    """The result of ``contacts`` (include/mhmr.h ``mhmr_contact_desc``); fields that were not asked for are None."""
    sdf: Optional[torch.Tensor]                # float32 [P, V], +inf = nothing within max_dist
    nearest_person: Optional[torch.Tensor]     # int32 [P, V], -1
    nearest_face: Optional[torch.Tensor]       # int32 [P, V], -1
    closest: Optional[torch.Tensor]            # float32 [P, V, 3], the vertex itself
    penetration_depth: Optional[torch.Tensor]  # float32 [P]
    inside_count: Optional[torch.Tensor]       # int32 [P]
    contact_count: Optional[torch.Tensor]      # int32 [P]
    pair_distance: Optional[torch.Tensor]      # float32 [P, P], +inf; [a, b] is measured from a's vertices: not symmetric
    pair_inside: Optional[torch.Tensor]        # int32 [P, P]
    aabb: Optional[torch.Tensor]               # float32 [P, 6]
    valid: Optional[torch.Tensor]              # uint8 [P]


_SHAPES = {"sdf": (lambda P, V: (P, V), torch.float32), "nearest_person": (lambda P, V: (P, V), torch.int32),
           "nearest_face": (lambda P, V: (P, V), torch.int32), "closest": (lambda P, V: (P, V, 3), torch.float32),
           "penetration_depth": (lambda P, V: (P,), torch.float32), "inside_count": (lambda P, V: (P,), torch.int32),
           "contact_count": (lambda P, V: (P,), torch.int32), "pair_distance": (lambda P, V: (P, P), torch.float32),
           "pair_inside": (lambda P, V: (P, P), torch.int32), "aabb": (lambda P, V: (P, 6), torch.float32),
           "valid": (lambda P, V: (P,), torch.uint8)}

_face_cache: dict = {}


def _faces_on(faces, V, dev):
    """Device int32 faces of one face array, its indices checked once per (face array, vertex count, device)
    (``mhmr_contact_check_faces``)."""
    f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
    f = np.ascontiguousarray(f, dtype=np.int32)
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"faces must be [F, 3], got {f.shape}")
    key = (hashlib.sha1(f.tobytes()).hexdigest(), f.shape[0], V, str(dev))
    hit = _face_cache.get(key)
    if hit is None:
        if _lib.lib().mhmr_contact_check_faces(f.ctypes.data if f.size else None, int(f.shape[0]), int(V)) != 0:
            raise ValueError(f"face indices must lie in [0, {V})")
        hit = torch.from_numpy(f).to(dev)
        _face_cache[key] = hit
    return hit


def contacts(verts, image_index, faces, max_dist=0.10, tau=0.01, want=FIELDS) -> Contacts:
    """Signed distances, penetration and contact of P meshes sharing one face array: verts [P, V, 3] cuda float32 (rows of one person
    contiguous, any person stride: the forward's ``v3d`` block is read in place), image_index [P] (a tensor or a list; only persons of
    one image interact), faces [F, 3].  Returns a ``Contacts`` of device tensors as include/mhmr.h ``mhmr_contact_desc`` defines them.

    ``max_dist`` (how far the search looks: farther surfaces report +inf) and ``tau`` (|sdf| <= tau counts as contact) are CONVENTIONS
    in metres, not measurements; the defaults are 0.10 and 0.01.
    ``want``: the field names to compute (default all); the others are None and cost nothing.  Which persons touch, symmetrically:
    ``pd = c.pair_distance; touching = torch.minimum(pd, pd.T) <= tau``.  The result describes ``verts`` as they are now: compute it
    again when the meshes have moved."""
    if not (torch.is_tensor(verts) and verts.is_cuda and verts.dim() == 3 and verts.shape[-1] == 3):
        raise ValueError("verts must be a cuda tensor [P, V, 3]")
    unknown = [n for n in want if n not in FIELDS]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}; the fields are {FIELDS}")
    if not (float(max_dist) >= 0.0 and 0.0 <= float(tau) <= float(max_dist) and np.isfinite(float(max_dist))):
        raise ValueError(f"need a finite max_dist >= 0 and 0 <= tau <= max_dist, got max_dist = {max_dist}, tau = {tau}")
    dev = verts.device
    verts = _strided(verts, dev, "verts")
    P, V = int(verts.shape[0]), int(verts.shape[1])
    idx = torch.as_tensor(image_index).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if idx.numel() != P:
        raise ValueError(f"image_index has {idx.numel()} entries for {P} meshes")
    f_dev = _faces_on(faces, V, dev)
    out = {n: (torch.empty(_SHAPES[n][0](P, V), dtype=_SHAPES[n][1], device=dev) if n in want else None) for n in FIELDS}
    if P:
        nbytes = _lib.workspace_bytes("mhmr_contact_workspace_bytes", P, V)
        with torch.cuda.device(dev):
            ws = _workspace(nbytes, dev)
            d = _lib.ContactDesc()
            d.P, d.V, d.F = P, V, int(f_dev.shape[0])
            d.verts, d.vstride = verts.data_ptr(), int(verts.stride(0)) if P > 1 else 3 * V
            d.image_index, d.faces = idx.data_ptr(), f_dev.data_ptr()
            d.max_dist, d.tau = float(max_dist), float(tau)
            d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
            for n in FIELDS:
                setattr(d, n, _lib.ptr(out[n]))
            _lib.check(_lib.lib().mhmr_contact(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "mhmr_contact")
    return Contacts(**out)


def penetration_loss(verts, c: Contacts) -> torch.Tensor:
    """The one-sided SDF penetration loss of Jiang et al., "Coherent Reconstruction of Multiple Humans from a Single Image" (CVPR
    2020): the sum over the vertices with ``c.sdf < 0`` of ``|v - c.closest|^2``.  Plain torch on the detached ``closest`` and ``sdf``:
    the gradient with respect to an intruding vertex is ``2 (v - closest)``, which pushes it to the nearest point of the surface it is
    inside; that surface is held fixed, and both persons move because both ordered pairs were evaluated.  ``c`` describes the meshes
    it was computed from: after an optimiser step compute ``contacts`` again."""
    if c.sdf is None or c.closest is None:
        raise ValueError("penetration_loss needs the sdf and closest fields")
    mask = (c.sdf.detach() < 0).unsqueeze(-1)
    diff = torch.where(mask, verts - c.closest.detach(), torch.zeros((), dtype=verts.dtype, device=verts.device))
    return (diff * diff).sum()
