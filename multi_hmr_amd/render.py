"""Mesh overlay on the GPU: the drop-in for the reference's ``utils/render.py:175-315 render_meshes`` (pyrender / OpenGL there)
and the batched form behind ``demo.overlay_human_meshes``.  The rasteriser is ``csrc/render.hip`` (include/mhmr.h
``mhmr_render_meshes``); there is no CPU path.

Render contract (one sample per pixel; this text defines the output, and the CPU oracle of the tests restates it in numpy):

1. Camera: per image K [3, 3] (fx = K00, fy = K11, cx = K02, cy = K12, skew ignored) and optional R [3, 3], t [3]; a vertex
   moves to camera coordinates as X = R x + t (OpenCV: X right, Y down, Z forward), u = fx X / Z + cx, v = fy Y / Z + cy.
   Pixel (row r, col c) is sampled at (c + 0.5, r + 0.5).
2. Clipping: znear = fl32(0.05), zfar = 100.  A face with any vertex at Z < znear is dropped, not clipped (a deviation from GL);
   a fragment is kept only if znear <= fl32(Z) <= zfar, the depth its key holds: a face lying on a clip plane keeps every pixel.
3. Culling (cull_back=True): face (a, b, c) is culled when dot((b - a) x (c - a), a) >= 0 in camera coordinates.
4. Coverage: a pixel centre is inside if all three edge functions are > 0, or = 0 on a top-left edge; edges shared by two
   faces are evaluated with their endpoints in one fixed order, so such a pixel is covered exactly once.  Zero-area faces
   cover nothing.
5. Visibility: Z = 1 / sum(lambda_i / Z_i) with lambda the screen-space barycentrics; the winner is the smallest 64-bit key
   (float_bits(Z) << 32) | (person * F + face): depth ties go to the lower (person, face), whatever the arrival order.
6. Normals: smooth=True -> the angle-weighted vertex normal (trimesh's ``vertex_normals`` form: sum over the incident
   non-degenerate faces, in face order, of corner angle x unit face normal, normalised), rotated by R, interpolated with the
   perspective-correct weights and normalised; a vertex without one uses the face normal.  smooth=False: the face normal.
7. Shading: glTF metallic-roughness with one directional light of ``intensity`` along the view axis and ambient 0.3, as
   pyrender's mesh.frag is recalled to implement it -- NOT checked against pyrender:
   l = (0, 0, -1), v = normalize(-p), h = normalize(l + v); nl = clamp(n.l, 0.001, 1), nv = clamp(|n.v|, 0.001, 1),
   nh, vh clamped to [0, 1]; f0 = mix(0.04, b, m), c_diff = b (1 - 0.04)(1 - m), alpha = roughness^2,
   F = f0 + (1 - f0)(1 - vh)^5, G = G1(nl) G1(nv) with G1(x) = 2x / (x + sqrt(a^2 + (1 - a^2) x^2)),
   D = a^2 / (pi ((nh a^2 - nh) nh + 1)^2); c = nl I ((1 - F) c_diff / pi + F G D / (4 nl nv)) + 0.3 b,
   rgb = floor(255 clamp(c^(1/2.2), 0, 1) + 0.5).
8. Edge mask (the reference's 3x3 smoothing, utils/render.py:302-311): m = fg ? max(0, k fl32(2/9) - 1) : 0 in fp32, k = covered
   pixels of the 3x3 neighbourhood (outside the image = not covered).
9. Blend: out = trunc(m (alpha rgb + (1 - alpha) img) + (1 - m) img) in fp32, every operation rounded on its own.
"""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np
import torch

from . import _lib

ZNEAR, ZFAR, AMBIENT = 0.05, 100.0, 0.3

#: the reference demo palette's ten fixed colours (utils/color.py), then a seeded continuation (the reference's is unseeded)
_HEX = ["0047AB", "6495ED", "FF9999", "FF9933", "00CC66", "66B2FF", "FF6666", "FF3333", "C0C0C0", "9933FF"]
PALETTE = [tuple(int(h[i:i + 2], 16) / 255 for i in (0, 2, 4)) for h in _HEX] + \
          [tuple(int(c) / 255 for c in row) for row in np.random.RandomState(0).randint(0, 256, size=(200, 3))]


def build_csr(faces, V):
    """Vertex -> incident (3 face + corner) entries, ascending (hence sorted by face): (adj_off [V + 1], adj) int32."""
    flat = np.asarray(faces, np.int64).reshape(-1)
    if flat.size and (flat.min() < 0 or flat.max() >= V):
        raise ValueError(f"face indices must lie in [0, {V})")
    adj = np.argsort(flat, kind="stable").astype(np.int32)
    adj_off = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(flat, minlength=V), out=adj_off[1:])
    return adj_off.astype(np.int32), adj


_face_cache: dict = {}
_ws_cache: dict = {}


def _faces_on(faces, V, dev):
    """Device faces and CSR of one face array, built once per (face array, vertex count, device)."""
    f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
    f = np.ascontiguousarray(f, dtype=np.int32)
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"faces must be [F, 3], got {f.shape}")
    key = (hashlib.sha1(f.tobytes()).hexdigest(), f.shape[0], V, str(dev))
    hit = _face_cache.get(key)
    if hit is None:
        adj_off, adj = build_csr(f, V)
        hit = tuple(torch.from_numpy(a).to(dev) for a in (f, adj_off, adj))
        _face_cache[key] = hit
    return hit


def _workspace(nbytes, dev):
    ws = _ws_cache.get(str(dev))
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        _ws_cache[str(dev)] = ws
    return ws


def _colors(colors, P):
    if colors is None:
        colors = [PALETTE[i % len(PALETTE)] for i in range(P)]
    c = colors.detach().float().cpu().numpy() if torch.is_tensor(colors) else np.asarray(colors, np.float32)
    c = np.broadcast_to(c.reshape(-1, 3) if c.size != 3 else c.reshape(1, 3), (P, 3)) if P else np.zeros((0, 3), np.float32)
    if c.shape != (P, 3):
        raise ValueError(f"colors must give one RGB triple per mesh ({P}), got {c.shape}")
    return np.array(c, np.float32, copy=True, order="C")


def _render(images_u8, verts, image_index, K, faces, colors, alpha, Rt, nviews, smooth, cull_back, return_debug, intensity, metallic,
            roughness):
    """render_batch (nviews None: mhmr_render_meshes, Rt [B, 3, 4] or None) and render_views (mhmr_render_views, Rt [B, nviews, 3, 4]
    or None = identity in every view).  Outputs [B, H, W, ...] or [B, nviews, H, W, ...]."""
    if not (torch.is_tensor(images_u8) and images_u8.is_cuda and images_u8.dtype == torch.uint8 and images_u8.dim() == 4
            and images_u8.shape[-1] == 3):
        raise ValueError("images_u8 must be a cuda uint8 tensor [B, H, W, 3]")
    dev = images_u8.device
    images = images_u8.contiguous()
    B, H, W, _ = images.shape
    if not (torch.is_tensor(verts) and verts.dim() == 3 and verts.shape[-1] == 3):
        raise ValueError("verts must be a tensor [P, V, 3]")
    verts = verts.to(device=dev, dtype=torch.float32)
    P, V = int(verts.shape[0]), int(verts.shape[1])
    if P and (verts.stride(2) != 1 or verts.stride(1) != 3 or (P > 1 and verts.stride(0) < 3 * V)):
        verts = verts.contiguous()
    idx = torch.as_tensor(image_index).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if idx.numel() != P:
        raise ValueError(f"image_index has {idx.numel()} entries for {P} meshes")
    Kt = torch.as_tensor(K, dtype=torch.float32).to(dev).reshape(B, 3, 3).contiguous()
    views = () if nviews is None else (nviews,)
    Rtt = None if Rt is None else torch.as_tensor(Rt, dtype=torch.float32).to(dev).reshape((B,) + views + (3, 4)).contiguous()
    if P:
        f_dev, off_dev, adj_dev = _faces_on(faces, V, dev)
        F = int(f_dev.shape[0])
    else:
        f_dev = off_dev = adj_dev = None
        F = int(np.asarray(faces).shape[0]) if faces is not None else 0
    col = torch.from_numpy(_colors(colors, P)).to(dev)
    out = torch.empty((B,) + views + (H, W, 3), dtype=torch.uint8, device=dev)
    key = torch.empty((B,) + views + (H, W), dtype=torch.int64, device=dev) if return_debug else None
    rgb = torch.empty((B,) + views + (H, W, 3), dtype=torch.uint8, device=dev) if return_debug else None

    d = _lib.RenderDesc()
    d.B, d.H, d.W, d.P, d.V, d.F = B, H, W, P, V, F
    d.verts, d.vstride = _lib.ptr(verts) if P else None, int(verts.stride(0)) if P > 1 else 3 * V
    d.faces, d.adj_off, d.adj = _lib.ptr(f_dev), _lib.ptr(off_dev), _lib.ptr(adj_dev)
    d.image_index, d.K, d.colors = _lib.ptr(idx), _lib.ptr(Kt), _lib.ptr(col)
    d.Rt = _lib.ptr(Rtt) if nviews is None else None
    d.alpha, d.intensity, d.ambient, d.metallic, d.roughness = float(alpha), float(intensity), AMBIENT, float(metallic), float(roughness)
    d.znear, d.zfar, d.smooth, d.cull_back = ZNEAR, ZFAR, int(bool(smooth)), int(bool(cull_back))
    d.img_in, d.img_out = _lib.ptr(images), _lib.ptr(out)
    d.key_out, d.rgb_out = _lib.ptr(key), _lib.ptr(rgb)
    L = _lib.lib()
    if nviews is None:
        nbytes = _lib.workspace_bytes("mhmr_render_workspace_bytes", C.byref(d))
    else:
        nbytes = _lib.workspace_bytes("mhmr_render_views_workspace_bytes", C.byref(d), nviews)
    with torch.cuda.device(dev):
        ws = _workspace(nbytes, dev)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        stream = torch.cuda.current_stream(dev).cuda_stream
        if nviews is None:
            _lib.check(L.mhmr_render_meshes(C.byref(d), stream), "mhmr_render_meshes")
        else:
            _lib.check(L.mhmr_render_views(C.byref(d), nviews, _lib.ptr(Rtt), stream), "mhmr_render_views")
    return (out, key, rgb) if return_debug else out


def render_batch(images_u8, verts, image_index, K, faces, colors=None, alpha=0.8, Rt=None, smooth=True, cull_back=True,
                 return_debug=False, intensity=3.0, metallic=0.0, roughness=0.5):
    """Draw P meshes sharing one face array into B images, on the images' device.

    images_u8 [B, H, W, 3] uint8 cuda; verts [P, V, 3] float32 cuda (rows of one person contiguous; any person stride, so a slice of
    the forward's ``v3d`` block is read in place); image_index [P] (image of each mesh); K [B, 3, 3]; faces [F, 3]; colors [P, 3] in
    [0, 1] (None: ``PALETTE``); Rt [B, 3, 4] = [R | t] or None.  Returns the blended images [B, H, W, 3] uint8 (a new tensor) and, with
    return_debug=True, also the winning keys [B, H, W] (int64 holding the uint64 bits; -1 = nothing drawn) and the pre-blend rgb
    [B, H, W, 3] uint8."""
    return _render(images_u8, verts, image_index, K, faces, colors, alpha, Rt, None, smooth, cull_back, return_debug, intensity,
                   metallic, roughness)


def render_views(images_u8, verts, image_index, K, faces, Rt, colors=None, alpha=0.8, smooth=True, cull_back=True, return_debug=False,
                 intensity=3.0, metallic=0.0, roughness=0.5):
    """Draw every image from NV cameras in one call: view (b, v) sees image b's meshes through K[b] and Rt[b, v] = [R | t], blended
    over images_u8[b].  Arguments as ``render_batch``, with Rt [B, NV, 3, 4] (NV >= 1).  Returns [B, NV, H, W, 3] uint8 and, with
    return_debug=True, the keys [B, NV, H, W] and the pre-blend rgb [B, NV, H, W, 3].  View v of the result is byte-identical to
    ``render_batch(..., Rt=Rt[:, v])``; the vertex normals are computed once per mesh, not once per view (csrc/render.hip)."""
    Rt = torch.as_tensor(Rt, dtype=torch.float32)
    if Rt.dim() != 4 or Rt.shape[2:] != (3, 4) or Rt.shape[1] < 1:
        raise ValueError(f"Rt must be [B, NV, 3, 4] with NV >= 1, got {tuple(Rt.shape)}")
    return _render(images_u8, verts, image_index, K, faces, colors, alpha, Rt, int(Rt.shape[1]), smooth, cull_back, return_debug,
                   intensity, metallic, roughness)


def render_meshes(img, l_mesh, l_face, cam_param, color=None, alpha=1.0, show_camera=False, intensity=3.0, metallicFactor=0.,
                  roughnessFactor=0.5, smooth=True):
    """Reference utils/render.py:175-315 on the GPU: img np.uint8 [H, W, 3]; l_mesh list of [V, 3] vertex arrays (numpy or cuda
    tensors); l_face list of [F, 3] face arrays, all equal (ValueError otherwise); cam_param {'focal', 'princpt'[, 'R', 't']}.
    Returns np.uint8 [H, W, 3].  color: list (one per mesh), tuple (all meshes) or None (``PALETTE``, where the reference draws
    unseeded random colours).  show_camera=True (the camera gizmo) is not implemented."""
    if show_camera:
        raise NotImplementedError("render_meshes(show_camera=True): the camera gizmo is not rendered")
    if len(l_face) != len(l_mesh):
        raise ValueError("l_mesh and l_face differ in length")
    faces0 = None
    for f in l_face:
        fa = f.detach().cpu().numpy() if torch.is_tensor(f) else np.asarray(f)
        if faces0 is None:
            faces0 = fa
        elif fa is not faces0 and not np.array_equal(fa, faces0):
            raise ValueError("render_meshes: every mesh of one call must share one face array")
    if isinstance(color, list):
        cols = [color[i] for i in range(len(l_mesh))]
    elif isinstance(color, tuple):
        cols = [color] * len(l_mesh)
    elif color is None:
        cols = None
    else:
        raise NotImplementedError("color must be a list, a tuple or None")
    img = np.asarray(img)
    if len(l_mesh) == 0:
        return img.astype(np.uint8)
    dev = next((m.device for m in l_mesh if torch.is_tensor(m) and m.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    verts = torch.stack([torch.as_tensor(np.asarray(m, np.float32)) if not torch.is_tensor(m) else m.detach().float()
                         for m in l_mesh]).to(dev)
    fx, fy = (float(v) for v in np.asarray(cam_param["focal"]).reshape(-1)[:2])
    cx, cy = (float(v) for v in np.asarray(cam_param["princpt"]).reshape(-1)[:2])
    K = torch.tensor([[[fx, 0, cx], [0, fy, cy], [0, 0, 1]]], dtype=torch.float32)
    Rt = None
    if "R" in cam_param or "t" in cam_param:
        Rt = torch.zeros(1, 3, 4)
        Rt[0, :, :3] = torch.as_tensor(np.asarray(cam_param.get("R", np.eye(3)), np.float32))
        Rt[0, :, 3] = torch.as_tensor(np.asarray(cam_param.get("t", np.zeros(3)), np.float32)).reshape(3)
    images = torch.from_numpy(np.array(img[..., :3], np.uint8))[None].to(dev)
    out = render_batch(images, verts, torch.zeros(len(l_mesh), dtype=torch.int32), K, faces0, colors=cols, alpha=alpha, Rt=Rt,
                       smooth=smooth, intensity=intensity, metallic=metallicFactor, roughness=roughnessFactor)
    return out[0].cpu().numpy()
