"""The 3D result as files: the drop-in for the reference's ``utils/render.py:62-173 create_scene`` (a trimesh scene exported as GLB
there; ``demo.py:371-384``, ``app.py:151``), its batched form ``export_batch``, and the distance labels of
``utils/render.py:365-405`` (``print_distance_on_image``, ``get_bbox``).

The vertices, the smooth vertex normals and the bounds of every person are laid out in the file's own byte layout by one launch of
``csrc/scene.hip`` (include/mhmr.h ``mhmr_scene_pack``, which holds the numeric contract) on the device where the vertices already
are, and leave it in one copy; there is no CPU path for that step.  The container is written here with ``struct`` and ``json``.

File layout (glTF 2.0 binary, little endian, one buffer; every chunk and buffer view 4-byte aligned, the JSON padded with spaces,
the binary with zeros):

* one ``uint32`` index buffer view (target 34963) shared by every person's primitive;
* per person a node ``person_<i>``, a mesh with one ``TRIANGLES`` primitive -- ``POSITION`` (with ``min`` / ``max``) and, with
  ``normals=True``, ``NORMAL``, views of target 34962 into the packed fp32 block -- and a material: ``baseColorFactor`` (r, g, b, 1),
  the metallic / roughness factors, ``alphaMode`` ``OPAQUE``.  Nodes carry no transform: the positions in the file are the packed
  bytes, already moved by the scene transform (default ``diag(-1, -1, 1)``: OpenCV camera axes to glTF's);
* with a photograph: node ``image``, a double-sided quad textured with it (embedded PNG, ``TEXCOORD_0``) where the camera sees it:
  corners ``K^-1 (u, v, 1) z0`` for the four image corners, ``z0 = 0.3 fx / W`` (a screen 0.3 m wide), so that from the origin the
  photograph lines up with the bodies; without ``K``: ``fx = fy = focal``, principal point at the image centre.  And node ``camera``:
  the four edges from the origin to those corners and the quad's outline, one red ``LINES`` primitive.
"""
from __future__ import annotations

import ctypes as C
import io
import json
import struct

import numpy as np

#: what the reference's create_scene applies to its whole scene (utils/render.py:167-171): [R | t], a half turn about z
DEFAULT_TRANSFORM = np.array([[-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 1, 0]], np.float32)
SCREEN_WIDTH = 0.3                                  # metres, the reference's screen_width

_MAGIC, _JSON, _BIN = 0x46546C67, 0x4E4F534A, 0x004E4942
_F32, _U32 = 5126, 5125
_ARRAY, _ELEMENT = 34962, 34963
_NCOMP = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4}
_DTYPE = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}


# ------------------------------------------------------------------------------------------------------------------ device
def pack_meshes(verts, faces, transform=None):
    """P meshes sharing one face array -> (packed [P, 2, V, 3], bounds [P, 2, 3]), float32 on the vertices' device, by one
    ``mhmr_scene_pack`` launch on the current stream: packed[p, 0] = R x + t, packed[p, 1] = the rotated smooth unit normals
    ((0, 0, 1) where a vertex has none), bounds[p] = min, max of packed[p, 0].

    verts [P, V, 3] float32 cuda (rows of one person contiguous; any person stride, so a slice of the forward's ``v3d`` block is
    read in place); faces [F, 3]; transform [3, 4] = [R | t] with R a rotation, None = ``DEFAULT_TRANSFORM``."""
    import torch
    from . import _lib
    from .render import _faces_on
    if not (torch.is_tensor(verts) and verts.is_cuda and verts.dim() == 3 and verts.shape[-1] == 3):
        raise ValueError("verts must be a cuda tensor [P, V, 3]")
    dev = verts.device
    verts = verts.detach().to(torch.float32)
    P, V = int(verts.shape[0]), int(verts.shape[1])
    if V < 1:
        raise ValueError("verts must hold at least one vertex per mesh")
    if P and (verts.stride(2) != 1 or verts.stride(1) != 3 or (P > 1 and verts.stride(0) < 3 * V)):
        verts = verts.contiguous()
    f_dev, off_dev, adj_dev = _faces_on(faces, V, dev)
    M = None if transform is None else torch.as_tensor(np.asarray(transform, np.float32).reshape(3, 4)).to(dev).contiguous()
    flat = torch.empty(P * (6 * V + 6), dtype=torch.float32, device=dev)   # one allocation, so that both leave in one copy
    out, bounds = flat[:P * 6 * V].view(P, 2, V, 3), flat[P * 6 * V:].view(P, 2, 3)
    if P == 0:
        return out, bounds
    d = _lib.SceneDesc()
    d.P, d.V, d.F = P, V, int(f_dev.shape[0])
    d.verts, d.vstride = _lib.ptr(verts), int(verts.stride(0)) if P > 1 else 3 * V
    d.faces, d.adj_off, d.adj = _lib.ptr(f_dev), _lib.ptr(off_dev), _lib.ptr(adj_dev)
    d.transform, d.out, d.bounds = _lib.ptr(M), _lib.ptr(out), _lib.ptr(bounds)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mhmr_scene_pack(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "mhmr_scene_pack")
    return out, bounds


# --------------------------------------------------------------------------------------------------------------- container
_pinned: dict = {}


def _to_host(packed, bounds, reuse=False):
    """Both results of one ``pack_meshes`` call as numpy arrays after ONE device -> host copy (they are two views of one allocation).
    reuse=True copies into a page-locked buffer kept for the next call (about three times the rate of a pageable copy for a
    batch's 60 MB): for callers that are done with the arrays before anybody calls again (one buffer per process, no lock)."""
    import torch
    P, V = int(packed.shape[0]), int(packed.shape[2])
    n = P * (6 * V + 6)
    flat = torch.as_strided(packed, (n,), (1,))
    assert packed.is_contiguous() and bounds.data_ptr() == packed.data_ptr() + 4 * P * 6 * V
    if reuse:
        buf = _pinned.get("buf")
        if buf is None or buf.numel() < n:
            buf = _pinned["buf"] = torch.empty(max(n, 1), dtype=torch.float32, pin_memory=True)
        host = buf[:n]
        host.copy_(flat, non_blocking=True)
        torch.cuda.current_stream(packed.device).synchronize()
    else:
        host = flat.cpu()
    host = host.numpy()
    return host[:P * 6 * V].reshape(P, 2, V, 3), host[P * 6 * V:].reshape(P, 2, 3)


def screen_quad(size, K=None, focal=600., transform=None):
    """The photograph's quad: corners [4, 3] float32 (top-left, top-right, bottom-right, bottom-left of an image of ``size`` =
    (W, H)) at depth ``z0 = 0.3 fx / W`` on the rays ``K^-1 (u, v, 1)``, moved by the scene transform (fp64, rounded once)."""
    W, H = int(size[0]), int(size[1])
    if K is None:
        fx = fy = float(focal)
        cx, cy = W / 2.0, H / 2.0
    else:
        K = np.asarray(K, np.float64).reshape(3, 3)
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    z0 = SCREEN_WIDTH * fx / W
    uv = np.array([[0, 0], [W, 0], [W, H], [0, H]], np.float64)
    X = np.stack([(uv[:, 0] - cx) / fx * z0, (uv[:, 1] - cy) / fy * z0, np.full(4, z0)], 1)
    M = np.asarray(DEFAULT_TRANSFORM if transform is None else transform, np.float64).reshape(3, 4)
    return (X @ M[:, :3].T + M[:, 3]).astype(np.float32)


def _png_bytes(image):
    from PIL import Image
    img = image if isinstance(image, Image.Image) else Image.fromarray(np.asarray(image, np.uint8))
    buf = io.BytesIO()
    img.convert("RGB").save(buf, format="PNG")
    return buf.getvalue(), img.size


def _colour_rows(colors, P):
    c = np.asarray(colors, np.float64).reshape(-1, 3) if P else np.zeros((0, 3))
    if c.shape[0] == 1 and P > 1:
        c = np.repeat(c, P, 0)
    if c.shape != (P, 3):
        raise ValueError(f"colors must give one RGB triple per mesh ({P}), got {c.shape}")
    return c


def glb_parts(block, bounds, faces, colors, image=None, K=None, focal=600., normals=True, metallic=0., roughness=0.5, transform=None):
    """The file as a list of bytes-like parts (header + JSON chunk, then the binary chunk piece by piece; the person block is passed
    through as a view of ``block``, not copied) from host arrays: block [P, 2, V, 3] float32 (positions, normals, already
    transformed), bounds [P, 2, 3] float32, faces [F, 3], colors [P, 3] in [0, 1]; image (PIL image or uint8 [H, W, 3]) and its
    camera K [3, 3] (None: ``focal``, centred) add the photograph's quad and the camera; ``transform`` places those two (None =
    ``DEFAULT_TRANSFORM``, the transform the block was packed with)."""
    block = np.asarray(block)
    bounds = np.asarray(bounds)
    if block.dtype != np.float32 or block.ndim != 4 or block.shape[1] != 2 or block.shape[3] != 3:
        raise ValueError("block must be float32 [P, 2, V, 3]")
    P, V = int(block.shape[0]), int(block.shape[2])
    if bounds.dtype != np.float32 or bounds.shape != (P, 2, 3):
        raise ValueError(f"bounds must be float32 [{P}, 2, 3]")
    block = np.ascontiguousarray(block)
    cols = _colour_rows(colors, P)
    views, accessors, meshes, materials, nodes, parts = [], [], [], [], [], []
    g = {"asset": {"version": "2.0", "generator": "multi_hmr_amd.scene"}, "scene": 0}
    offset = 0

    def add_view(data, target=None):
        nonlocal offset
        mv = memoryview(data).cast("B")
        view = {"buffer": 0, "byteOffset": offset, "byteLength": mv.nbytes}
        if target is not None:
            view["target"] = target
        views.append(view)
        parts.append(mv)
        pad = -mv.nbytes % 4
        if pad:
            parts.append(b"\0" * pad)
        offset += mv.nbytes + pad
        return len(views) - 1

    def add_accessor(view, ctype, count, kind, lo=None, hi=None):
        acc = {"bufferView": view, "componentType": ctype, "count": int(count), "type": kind}
        if lo is not None:
            acc["min"], acc["max"] = [float(v) for v in lo], [float(v) for v in hi]
        accessors.append(acc)
        return len(accessors) - 1

    def add_node(name, primitive):
        meshes.append({"name": name, "primitives": [primitive]})
        nodes.append({"name": name, "mesh": len(meshes) - 1})

    if P:
        f = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), dtype="<u4")
        if f.size == 0 or int(f.max()) >= V:
            raise ValueError(f"faces must be a non-empty [F, 3] array of indices in [0, {V})")
        idx_acc = add_accessor(add_view(f, _ELEMENT), _U32, f.size, "SCALAR")
        person_views = []
        if normals:                                   # the block as it is: one contiguous range, two views per person
            for p in range(P):
                person_views.append((add_view(block[p, 0], _ARRAY), add_view(block[p, 1], _ARRAY)))
        else:
            for p in range(P):
                person_views.append((add_view(block[p, 0], _ARRAY), None))
        for p, (vpos, vnrm) in enumerate(person_views):
            attrs = {"POSITION": add_accessor(vpos, _F32, V, "VEC3", bounds[p, 0], bounds[p, 1])}
            if vnrm is not None:
                attrs["NORMAL"] = add_accessor(vnrm, _F32, V, "VEC3")
            materials.append({"name": f"person_{p}", "alphaMode": "OPAQUE",
                              "pbrMetallicRoughness": {"baseColorFactor": [float(cols[p, 0]), float(cols[p, 1]), float(cols[p, 2]), 1.0],
                                                       "metallicFactor": float(metallic), "roughnessFactor": float(roughness)}})
            add_node(f"person_{p}", {"attributes": attrs, "indices": idx_acc, "material": len(materials) - 1, "mode": 4})
    if image is not None:
        png, size = _png_bytes(image)
        quad = screen_quad(size, K, focal, transform)
        qpos = add_accessor(add_view(quad, _ARRAY), _F32, 4, "VEC3", quad.min(0), quad.max(0))
        quv = add_accessor(add_view(np.array([[0, 0], [1, 0], [1, 1], [0, 1]], "<f4"), _ARRAY), _F32, 4, "VEC2")
        qidx = add_accessor(add_view(np.array([0, 1, 2, 0, 2, 3], "<u4"), _ELEMENT), _U32, 6, "SCALAR")
        materials.append({"name": "image", "doubleSided": True, "alphaMode": "OPAQUE",
                          "pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 1.0}})
        add_node("image", {"attributes": {"POSITION": qpos, "TEXCOORD_0": quv}, "indices": qidx, "material": len(materials) - 1,
                           "mode": 4})
        M = np.asarray(DEFAULT_TRANSFORM if transform is None else transform, np.float32).reshape(3, 4)
        cam = np.concatenate([M[None, :, 3], quad]).astype("<f4")                 # the optical centre, then the corners
        cpos = add_accessor(add_view(cam, _ARRAY), _F32, 5, "VEC3", cam.min(0), cam.max(0))
        lines = np.array([0, 1, 0, 2, 0, 3, 0, 4, 1, 2, 2, 3, 3, 4, 4, 1], "<u4")
        cidx = add_accessor(add_view(lines, _ELEMENT), _U32, lines.size, "SCALAR")
        materials.append({"name": "camera", "alphaMode": "OPAQUE",
                          "pbrMetallicRoughness": {"baseColorFactor": [1.0, 0.0, 0.0, 1.0], "metallicFactor": 0.0, "roughnessFactor": 1.0}})
        add_node("camera", {"attributes": {"POSITION": cpos}, "indices": cidx, "material": len(materials) - 1, "mode": 1})
        g["images"] = [{"bufferView": add_view(png), "mimeType": "image/png"}]
        g["samplers"] = [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]
        g["textures"] = [{"sampler": 0, "source": 0}]
    g["scenes"] = [{"nodes": list(range(len(nodes)))}] if nodes else [{}]
    if nodes:
        g.update(nodes=nodes, meshes=meshes, materials=materials, accessors=accessors, bufferViews=views,
                 buffers=[{"byteLength": offset}])
    js = json.dumps(g, separators=(",", ":")).encode("ascii")
    js += b" " * (-len(js) % 4)
    total = 12 + 8 + len(js) + ((8 + offset) if offset else 0)
    head = struct.pack("<IIIII", _MAGIC, 2, total, len(js), _JSON) + js
    if offset:
        head += struct.pack("<II", offset, _BIN)
    return [head] + parts


class GlbScene:
    """What ``create_scene`` returns: ``.export(path)`` writes the file, ``.to_glb()`` returns its bytes."""

    def __init__(self, parts):
        self._parts = parts

    def to_glb(self) -> bytes:
        return b"".join(self._parts)

    def export(self, path):
        if not str(path).lower().endswith(".glb"):
            raise ValueError("only the binary glTF container (.glb) is written")
        with open(path, "wb") as f:
            for p in self._parts:
                f.write(p)
        return path


def read_glb(src) -> dict:
    """A reader for what this module writes, nothing more: ``src`` a path or the bytes -> {'json': the document, 'accessors': every
    accessor as a numpy array ([count] or [count, components]), 'nodes': {node name: {'attributes': {name: array}, 'indices': array,
    'mode': int, 'material': dict}}, 'images': [encoded bytes]}."""
    data = src if isinstance(src, (bytes, bytearray, memoryview)) else open(src, "rb").read()
    data = bytes(data)
    magic, version, total = struct.unpack_from("<III", data, 0)
    if magic != _MAGIC or version != 2 or total != len(data):
        raise ValueError("not a glTF 2.0 binary file of the stated length")
    n, kind = struct.unpack_from("<II", data, 12)
    if kind != _JSON:
        raise ValueError("the first chunk must be JSON")
    g = json.loads(data[20:20 + n].decode("utf-8"))
    binary = b""
    if 20 + n < total:
        m, kind = struct.unpack_from("<II", data, 20 + n)
        if kind != _BIN:
            raise ValueError("the second chunk must be BIN")
        binary = data[28 + n:28 + n + m]

    def view_bytes(i):
        v = g["bufferViews"][i]
        if "byteStride" in v:
            raise ValueError("strided buffer views are not read")
        return binary[v.get("byteOffset", 0):v.get("byteOffset", 0) + v["byteLength"]]

    accessors = []
    for a in g.get("accessors", []):
        ncomp, dt = _NCOMP[a["type"]], np.dtype(_DTYPE[a["componentType"]]).newbyteorder("<")
        arr = np.frombuffer(view_bytes(a["bufferView"]), dt, a["count"] * ncomp, a.get("byteOffset", 0))
        accessors.append(arr if ncomp == 1 else arr.reshape(a["count"], ncomp))
    nodes = {}
    for node in g.get("nodes", []):
        prim = g["meshes"][node["mesh"]]["primitives"][0]
        nodes[node["name"]] = {"attributes": {k: accessors[i] for k, i in prim["attributes"].items()},
                               "indices": accessors[prim["indices"]], "mode": prim.get("mode", 4),
                               "material": g["materials"][prim["material"]]}
    images = [view_bytes(im["bufferView"]) for im in g.get("images", [])]
    return {"json": g, "accessors": accessors, "nodes": nodes, "images": images}


# ------------------------------------------------------------------------------------------------------------------ scenes
def _one_face_array(l_face):
    import torch
    faces0 = None
    for f in l_face:
        fa = f.detach().cpu().numpy() if torch.is_tensor(f) else np.asarray(f)
        if faces0 is None:
            faces0 = fa
        elif fa is not faces0 and not np.array_equal(fa, faces0):
            raise ValueError("create_scene: every mesh of one scene must share one face array")
    return faces0


def _K33(K):
    import torch
    if K is None:
        return None
    K = K.detach().float().cpu().numpy() if torch.is_tensor(K) else np.asarray(K, np.float32)
    return K.reshape(-1, 3, 3)[0]


def create_scene(img_pil, l_mesh, l_face, color=None, metallicFactor=0., roughnessFactor=0.5, focal=600, K=None):
    """Reference utils/render.py:62-173: the persons' meshes, the photograph on a quad in front of the camera and the camera itself,
    as an object with ``.export(path)`` (GLB) and ``.to_glb()``.  l_mesh: [V, 3] vertex arrays (cuda tensors or numpy) in camera
    coordinates; l_face: [F, 3] face arrays, all equal (ValueError otherwise).  color: a list (one per mesh), a tuple (all meshes) or
    None (``render.PALETTE`` in order, where the reference draws unseeded random colours).  Extension: K [3, 3] or [1, 3, 3], the
    camera of ``img_pil`` (None: ``focal``, principal point at the centre).  img_pil None: no photograph and no camera."""
    import torch
    from .render import PALETTE
    n = len(l_mesh)
    if len(l_face) != n:
        raise ValueError("l_mesh and l_face differ in length")
    faces0 = _one_face_array(l_face)
    if isinstance(color, list):
        cols = [color[i] for i in range(n)]
    elif isinstance(color, tuple):
        cols = [color] * n
    elif color is None:
        cols = [PALETTE[i % len(PALETTE)] for i in range(n)]
    else:
        raise NotImplementedError("color must be a list, a tuple or None")
    if n:
        from .demo import _stacked
        packed, bounds = pack_meshes(_stacked([m.detach() if torch.is_tensor(m) else m for m in l_mesh]), faces0)
        block, bnd = _to_host(packed, bounds)                             # one copy off the device
    else:
        block, bnd, faces0 = np.zeros((0, 2, 1, 3), np.float32), np.zeros((0, 2, 3), np.float32), np.zeros((0, 3), np.int32)
    return GlbScene(glb_parts(block, bnd, faces0, cols, image=img_pil, K=_K33(K), focal=focal, metallic=metallicFactor,
                              roughness=roughnessFactor))


def export_batch(verts, image_index, faces, paths, colors=None, images=None, K=None, normals=True, metallic=0., roughness=0.5):
    """The batched form, the counterpart of ``render.render_batch``: one file per image of a batch.  verts [P, V, 3] cuda and
    image_index [P] (ascending) as ``model(x, K=K, return_batched=True)`` returns them; paths: one ``.glb`` name per image;
    colors [P, 3] (None: ``render.PALETTE`` restarting with every image, as the demo colours its persons); images: one photograph per
    image (PIL or uint8 array) or None; K [B, 3, 3] the photographs' cameras or None.  One ``pack_meshes`` launch and one device ->
    host copy for the whole batch, then the B files, each writing its persons' byte range of that one host buffer; an image without
    persons still gets a file.  Returns ``paths``."""
    import torch
    from .render import PALETTE
    B = len(paths)
    idx = torch.as_tensor(image_index).detach().cpu().numpy().astype(np.int64).reshape(-1)
    P = int(idx.shape[0])
    if P != int(verts.shape[0]):
        raise ValueError(f"image_index has {P} entries for {int(verts.shape[0])} meshes")
    if P and (np.any(np.diff(idx) < 0) or idx[0] < 0 or idx[-1] >= B):
        raise ValueError("image_index must ascend within [0, len(paths))")
    if images is not None and len(images) != B:
        raise ValueError("images must give one photograph per path")
    Ks = None if K is None else (K.detach().float().cpu().numpy() if torch.is_tensor(K) else np.asarray(K, np.float32)).reshape(B, 3, 3)
    start = np.searchsorted(idx, np.arange(B + 1))
    if colors is None:
        cols = np.array([PALETTE[(p - start[idx[p]]) % len(PALETTE)] for p in range(P)], np.float64).reshape(P, 3)
    else:
        cols = _colour_rows(colors.detach().cpu().numpy() if torch.is_tensor(colors) else colors, P)
    if P:
        packed, bounds = pack_meshes(verts, faces)
        block, bnd = _to_host(packed, bounds, reuse=True)                 # consumed by the loop below, before the next call
    else:
        block, bnd = np.zeros((0, 2, 1, 3), np.float32), np.zeros((0, 2, 3), np.float32)
    for b in range(B):
        p0, p1 = int(start[b]), int(start[b + 1])
        parts = glb_parts(block[p0:p1], bnd[p0:p1], faces if p1 > p0 else np.zeros((0, 3), np.int32), cols[p0:p1],
                          image=None if images is None else images[b], K=None if Ks is None else Ks[b], normals=normals,
                          metallic=metallic, roughness=roughness)
        GlbScene(parts).export(paths[b])
    return list(paths)


# ------------------------------------------------------------------------------------------------------------------ labels
def get_bbox(points, factor=1., output_format='xywh'):
    """Reference utils/render.py:384-405: the box of points [k, 2] scaled by ``factor`` about its centre, truncated to integers:
    [x1, y1, w, h] ('xywh') or [x1, y1, x2, y2] ('x1y1x2y2')."""
    assert len(points.shape) == 2, f"Wrong shape, expected two-dimensional array. Got shape {points.shape}"
    assert points.shape[1] == 2
    x1, x2 = points[:, 0].min(), points[:, 0].max()
    y1, y2 = points[:, 1].min(), points[:, 1].max()
    cx, cy = (x2 + x1) / 2., (y2 + y1) / 2.
    sx, sy = int(factor * np.abs(x2 - x1)), int(factor * np.abs(y2 - y1))
    x1, y1 = int(cx - sx / 2.), int(cy - sy / 2.)
    x2, y2 = int(cx + sx / 2.), int(cy + sy / 2.)
    if output_format == 'xywh':
        return [x1, y1, sx, sy]
    if output_format == 'x1y1x2y2':
        return [x1, y1, x2, y2]
    raise NotImplementedError


def _host(t):
    return t.detach().float().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def distance_labels(humans, _color, K=None, font=None):
    """One label per person, as ``print_distance_on_image`` draws it: {'text': f"{d:.2f}m" with d = sqrt(x^2 + z^2) of
    ``transl_pelvis``, 'fill': the person's colour as integers, 'point': the top centre of the box (factor 1.35) of the person's 2D
    joints, 'anchor': where the text starts (the point moved left by half the text's length), 'bbox': that box}.  The 2D joints are
    ``j2d_smplx`` if present, else ``j2d``; with K [3, 3] / [1, 3, 3] they are ``j3d`` projected with K instead."""
    from PIL import ImageFont
    font = font or ImageFont.load_default()
    K = _K33(K)
    labels = []
    for i_hum, hum in enumerate(humans):
        transl = _host(hum['transl_pelvis']).reshape(3)
        dist_cam = np.sqrt(((transl[[0, 2]]) ** 2).sum())                         # discarding the Y axis
        if K is None:
            j2d = _host(hum['j2d_smplx'] if 'j2d_smplx' in hum else hum['j2d'])
        else:
            j3d = _host(hum['j3d']).astype(np.float64)
            j2d = np.stack([K[0, 0] * j3d[:, 0] / j3d[:, 2] + K[0, 2], K[1, 1] * j3d[:, 1] / j3d[:, 2] + K[1, 2]], 1)
        bbox = get_bbox(j2d, factor=1.35, output_format='x1y1x2y2')
        point = [(bbox[0] + bbox[2]) / 2., bbox[1]]
        txt = f"{dist_cam:.2f}m"
        anchor = (point[0] - font.getlength(txt) // 2, point[1])
        fill = tuple((np.asarray(_color[i_hum]) * 255).astype(np.int32).tolist())
        labels.append({"text": txt, "fill": fill, "point": tuple(point), "anchor": anchor, "bbox": bbox})
    return labels


def print_distance_on_image(pred_rend_array, humans, _color, K=None):
    """Reference utils/render.py:365-382: every person's distance from the camera written above the person, in the person's colour
    and PIL's default font -> np.uint8 [H, W, 3].  Extension: K, see ``distance_labels`` (the persons' own ``j2d`` is in the
    network's input resolution; an overlay at the photograph's resolution needs the photograph's camera)."""
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default()
    rend_pil = Image.fromarray(pred_rend_array)
    draw = ImageDraw.Draw(rend_pil)
    for lab in distance_labels(humans, _color, K=K, font=font):
        draw.text(lab["anchor"], lab["text"], fill=lab["fill"], font=font)
    return np.asarray(rend_pil)
