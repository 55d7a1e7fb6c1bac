"""The 3D export without a GPU: the GLB container written by ``scene.glb_parts`` from host arrays (read back by ``scene.read_glb``
and by an independent parse made here from ``struct`` and ``json`` alone), ``create_scene``'s argument checks, the distance labels
against the reference's own functions (tests/golden/distance_labels.npz), and the C entry ``mhmr_scene_pack``: declared, exported,
its descriptor laid out as the header lays it out, its argument checks made before any launch."""
import ctypes
import io
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from multi_hmr_amd import _lib, scene
import render_oracle as ro
import scene_oracle as so

PIL = pytest.importorskip("PIL")
from PIL import Image, ImageDraw, ImageFont  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden", "distance_labels.npz")
FIELDS = ["P", "V", "F", "verts", "vstride", "faces", "adj_off", "adj", "transform", "out", "bounds"]
BAD_ARG, BAD_SHAPE = -1, -2
COLORS = [(0.1, 0.5, 0.9), (1.0, 0.25, 0.0), (0.2, 0.2, 0.2)]
K = np.array([[612.5, 0, 322.25], [0, 608.75, 236.5], [0, 0, 1]], np.float32)
W, H = 640, 480


def _three_spheres():
    v, f = ro.icosphere(3)
    verts = np.stack([v * 0.4 + np.array(c, np.float32) for c in ((-1.0, 0.1, 3.0), (0.0, -0.2, 4.0), (1.1, 0.0, 3.5))]).astype(np.float32)
    block, bounds, none, _ = so.pack(verts, f)
    assert not none.any()
    return verts, f, block, bounds


def _photo():
    rng = np.random.default_rng(5)
    return Image.fromarray(rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8))


def _independent_parse(data):
    """struct + json only: (document, binary chunk), with the container's own invariants asserted on the way."""
    magic, version, total = struct.unpack_from("<III", data, 0)
    assert magic == 0x46546C67 and version == 2 and total == len(data)
    n0, t0 = struct.unpack_from("<II", data, 12)
    assert t0 == 0x4E4F534A and n0 % 4 == 0
    doc = json.loads(data[20:20 + n0].decode("utf-8"))
    assert data[20:20 + n0].rstrip(b" ") == data[20:20 + n0].rstrip()      # padded with spaces only
    if 20 + n0 == total:
        return doc, b""
    n1, t1 = struct.unpack_from("<II", data, 20 + n0)
    assert t1 == 0x004E4942 and n1 % 4 == 0 and 28 + n0 + n1 == total       # exactly two chunks
    return doc, data[28 + n0:]


def _accessor(doc, binary, i):
    a = doc["accessors"][i]
    v = doc["bufferViews"][a["bufferView"]]
    ncomp = {"SCALAR": 1, "VEC2": 2, "VEC3": 3}[a["type"]]
    code, size = {5126: ("f", 4), 5125: ("I", 4)}[a["componentType"]]
    assert a["count"] * ncomp * size == v["byteLength"]
    vals = struct.unpack_from(f"<{a['count'] * ncomp}{code}", binary, v["byteOffset"])
    return np.array(vals, np.float32 if code == "f" else np.uint32).reshape(a["count"], ncomp)


@pytest.mark.parametrize("with_photo", [False, True])
@pytest.mark.parametrize("normals", [False, True])
def test_writer_against_an_independent_parse_and_the_reader(with_photo, normals, tmp_path):
    verts, f, block, bounds = _three_spheres()
    P, V = block.shape[0], block.shape[2]
    photo = _photo() if with_photo else None
    parts = scene.glb_parts(block, bounds, f, COLORS, image=photo, K=K if with_photo else None, normals=normals, metallic=0.25,
                            roughness=0.75)
    path = tmp_path / "scene.glb"
    scene.GlbScene(parts).export(str(path))
    data = path.read_bytes()
    assert data == scene.GlbScene(parts).to_glb() and len(data) == os.path.getsize(path)

    doc, binary = _independent_parse(data)
    assert doc["asset"]["version"] == "2.0" and len(doc["buffers"]) == 1 and doc["buffers"][0]["byteLength"] == len(binary)
    spans = sorted((v["byteOffset"], v["byteOffset"] + v["byteLength"]) for v in doc["bufferViews"])
    assert all(v["buffer"] == 0 and v["byteOffset"] % 4 == 0 and v["byteLength"] > 0 for v in doc["bufferViews"])
    assert spans[0][0] >= 0 and spans[-1][1] <= len(binary)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))              # inside the buffer, no overlap
    covered = np.zeros(len(binary), bool)
    for a, b in spans:
        covered[a:b] = True
    assert not np.frombuffer(binary, np.uint8)[~covered].any()              # what pads the views is zero

    names = [n["name"] for n in doc["nodes"]]
    assert names == [f"person_{p}" for p in range(P)] + (["image", "camera"] if with_photo else [])
    assert doc["scenes"][doc["scene"]]["nodes"] == list(range(len(names)))
    assert all(set(n) == {"name", "mesh"} for n in doc["nodes"])            # no node transform
    idx_views = set()
    for p in range(P):
        prim = doc["meshes"][doc["nodes"][p]["mesh"]]["primitives"]
        assert len(prim) == 1 and prim[0]["mode"] == 4
        prim = prim[0]
        assert set(prim["attributes"]) == ({"POSITION", "NORMAL"} if normals else {"POSITION"})
        ia = doc["accessors"][prim["indices"]]
        assert ia["componentType"] == 5125 and ia["type"] == "SCALAR" and ia["count"] == f.size
        assert doc["bufferViews"][ia["bufferView"]]["target"] == 34963
        idx_views.add(ia["bufferView"])
        idx = _accessor(doc, binary, prim["indices"])
        assert idx.max() < V and np.array_equal(idx.reshape(-1, 3), f.astype(np.uint32))
        pa = doc["accessors"][prim["attributes"]["POSITION"]]
        assert pa["componentType"] == 5126 and pa["type"] == "VEC3" and pa["count"] == V
        assert doc["bufferViews"][pa["bufferView"]]["target"] == 34962
        pos = _accessor(doc, binary, prim["attributes"]["POSITION"])
        assert pos.tobytes() == block[p, 0].tobytes()
        assert np.array_equal(np.float32(pa["min"]), pos.min(0)) and np.array_equal(np.float32(pa["max"]), pos.max(0))
        assert np.array_equal(np.float32(pa["min"]), bounds[p, 0]) and np.array_equal(np.float32(pa["max"]), bounds[p, 1])
        if normals:
            na = doc["accessors"][prim["attributes"]["NORMAL"]]
            assert na["componentType"] == 5126 and na["type"] == "VEC3" and na["count"] == V
            assert doc["bufferViews"][na["bufferView"]]["target"] == 34962
            assert _accessor(doc, binary, prim["attributes"]["NORMAL"]).tobytes() == block[p, 1].tobytes()
        mat = doc["materials"][prim["material"]]
        assert mat["alphaMode"] == "OPAQUE"
        assert mat["pbrMetallicRoughness"] == {"baseColorFactor": list(COLORS[p]) + [1.0], "metallicFactor": 0.25, "roughnessFactor": 0.75}
    assert len(idx_views) == 1                                              # one index buffer view for every person
    if normals:                                                             # the block is in the file as it is, in one piece
        assert block.tobytes() in binary

    back = scene.read_glb(str(path))
    assert back["json"] == doc and scene.read_glb(data)["json"] == doc
    for p in range(P):
        node = back["nodes"][f"person_{p}"]
        assert node["attributes"]["POSITION"].tobytes() == block[p, 0].tobytes()
        assert np.array_equal(node["indices"].reshape(-1, 3), f) and node["mode"] == 4
        assert ("NORMAL" in node["attributes"]) == normals
        if normals:
            assert node["attributes"]["NORMAL"].tobytes() == block[p, 1].tobytes()
    for i in range(len(doc["accessors"])):
        assert np.array_equal(back["accessors"][i].reshape(-1), _accessor(doc, binary, i).reshape(-1))

    if not with_photo:
        assert "images" not in doc and back["images"] == []
        return
    # the photograph: an embedded PNG that decodes to it, on a double-sided quad whose corners the camera K sees at the image corners
    assert doc["images"][0]["mimeType"] == "image/png" and "uri" not in doc["images"][0]
    v = doc["bufferViews"][doc["images"][0]["bufferView"]]
    png = binary[v["byteOffset"]:v["byteOffset"] + v["byteLength"]]
    assert png == back["images"][0]
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(png)).convert("RGB")), np.asarray(photo))
    prim = doc["meshes"][doc["nodes"][P]["mesh"]]["primitives"][0]
    mat = doc["materials"][prim["material"]]
    assert mat["doubleSided"] is True and mat["pbrMetallicRoughness"]["baseColorTexture"]["index"] == 0
    assert doc["textures"][0]["source"] == 0 and prim["mode"] == 4
    quad = _accessor(doc, binary, prim["attributes"]["POSITION"]).astype(np.float64)
    qa = doc["accessors"][prim["attributes"]["POSITION"]]
    assert np.array_equal(np.float32(qa["min"]), quad.min(0)) and np.array_equal(np.float32(qa["max"]), quad.max(0))
    uv = _accessor(doc, binary, prim["attributes"]["TEXCOORD_0"])
    assert np.array_equal(uv, np.float32([[0, 0], [1, 0], [1, 1], [0, 1]]))
    qidx = _accessor(doc, binary, prim["indices"]).reshape(-1)
    assert qidx.max() < 4 and sorted(set(qidx.tolist())) == [0, 1, 2, 3] and len(qidx) == 6
    cam_space = quad * np.array([-1.0, -1.0, 1.0])                          # the default scene transform is its own inverse
    Kd = K.astype(np.float64)
    proj = np.stack([Kd[0, 0] * cam_space[:, 0] / cam_space[:, 2] + Kd[0, 2], Kd[1, 1] * cam_space[:, 1] / cam_space[:, 2] + Kd[1, 2]], 1)
    assert np.abs(proj - np.array([[0, 0], [W, 0], [W, H], [0, H]])).max() <= 1e-3
    assert np.allclose(cam_space[:, 2], 0.3 * Kd[0, 0] / W, rtol=1e-6, atol=0)
    # the camera: the origin and the four corners, eight segments, red
    prim = doc["meshes"][doc["nodes"][P + 1]["mesh"]]["primitives"][0]
    assert prim["mode"] == 1
    cam = _accessor(doc, binary, prim["attributes"]["POSITION"])
    assert np.array_equal(cam[0], np.zeros(3, np.float32)) and np.array_equal(cam[1:], quad.astype(np.float32))
    seg = {tuple(sorted(s)) for s in _accessor(doc, binary, prim["indices"]).reshape(-1, 2).tolist()}
    assert seg == {(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 3), (3, 4), (1, 4)}
    assert doc["materials"][prim["material"]]["pbrMetallicRoughness"]["baseColorFactor"] == [1.0, 0.0, 0.0, 1.0]


def test_quad_without_K_uses_focal_and_the_image_centre():
    quad = scene.screen_quad((W, H), None, focal=600).astype(np.float64) * np.array([-1.0, -1.0, 1.0])
    proj = np.stack([600 * quad[:, 0] / quad[:, 2] + W / 2, 600 * quad[:, 1] / quad[:, 2] + H / 2], 1)
    assert np.abs(proj - np.array([[0, 0], [W, 0], [W, H], [0, H]])).max() <= 1e-3


def test_create_scene_argument_checks_and_the_empty_scenes(tmp_path):
    v, f = ro.icosphere(1)
    with pytest.raises(ValueError):
        scene.create_scene(_photo(), [v, v + 1], [f, f[::-1].copy()]).export(str(tmp_path / "a.glb"))
    with pytest.raises(ValueError):
        scene.create_scene(_photo(), [v, v + 1], [f])
    with pytest.raises(NotImplementedError):
        scene.create_scene(_photo(), [v], [f], color="red").export(str(tmp_path / "a.glb"))
    with pytest.raises(NotImplementedError):
        scene.create_scene(_photo(), [v], [f], color=np.zeros(3))
    assert not os.path.exists(tmp_path / "a.glb")

    nobody = scene.create_scene(_photo(), [], [], K=K[None])                # zero persons: the photograph and the camera
    path = nobody.export(str(tmp_path / "nobody.glb"))
    doc, binary = _independent_parse(open(path, "rb").read())
    assert [n["name"] for n in doc["nodes"]] == ["image", "camera"] and doc["buffers"][0]["byteLength"] == len(binary)
    assert sorted(scene.read_glb(path)["nodes"]) == ["camera", "image"]
    empty = scene.create_scene(None, [], []).to_glb()                       # nothing at all: still a valid file
    doc, binary = _independent_parse(empty)
    assert doc["scenes"] == [{}] and doc["scene"] == 0 and binary == b"" and "buffers" not in doc and "nodes" not in doc
    assert scene.read_glb(empty)["nodes"] == {}
    with pytest.raises(ValueError):
        nobody.export(str(tmp_path / "nobody.gltf"))


def test_writer_rejects_inputs_it_cannot_lay_out():
    _, f, block, bounds = _three_spheres()
    with pytest.raises(ValueError):
        scene.glb_parts(block.astype(np.float64), bounds, f, COLORS)
    with pytest.raises(ValueError):
        scene.glb_parts(block, bounds[:2], f, COLORS)
    with pytest.raises(ValueError):
        scene.glb_parts(block, bounds, f, COLORS[:2])
    with pytest.raises(ValueError):
        scene.glb_parts(block, bounds, f + block.shape[2], COLORS)          # an index >= V
    with pytest.raises(ValueError):
        scene.read_glb(scene.GlbScene(scene.glb_parts(block, bounds, f, COLORS)).to_glb()[:-4])


# ------------------------------------------------------------------------------------------------------------------ labels
def test_get_bbox_and_the_labels_equal_the_references():
    g = np.load(GOLD)
    j2d, transl, colors = g["j2d"], g["transl_pelvis"], g["colors"]
    n = len(j2d)
    for i in range(n):
        assert scene.get_bbox(j2d[i], factor=1.35, output_format="xywh") == g["bbox_xywh"][i].tolist()
        assert scene.get_bbox(j2d[i], factor=1.35, output_format="x1y1x2y2") == g["bbox_x1y1x2y2"][i].tolist()
        assert scene.get_bbox(j2d[i]) == g["bbox_default"][i].tolist()
    with pytest.raises(NotImplementedError):
        scene.get_bbox(j2d[0], output_format="cxcywh")
    with pytest.raises(AssertionError):
        scene.get_bbox(j2d[0].reshape(-1))

    humans = [{"transl_pelvis": transl[i], "j2d": j2d[i]} for i in range(n)]
    cols = [tuple(c) for c in colors]
    labels = scene.distance_labels(humans, cols)
    font = ImageFont.load_default()
    Wg, Hg = (int(v) for v in g["image_size"])
    image = np.random.default_rng(1).integers(0, 256, size=(Hg, Wg, 3)).astype(np.uint8)
    want = Image.fromarray(image)
    draw = ImageDraw.Draw(want)
    for i, lab in enumerate(labels):
        assert lab["text"] == str(g["texts"][i]) and lab["fill"] == tuple(g["fills"][i].tolist())
        assert lab["point"] == tuple(g["points"][i].tolist()) and lab["bbox"] == g["bbox_x1y1x2y2"][i].tolist()
        anchor = (g["points"][i][0] - font.getlength(lab["text"]) // 2, g["points"][i][1])   # derived with this machine's Pillow
        assert lab["anchor"] == anchor
        draw.text(anchor, str(g["texts"][i]), fill=tuple(g["fills"][i].tolist()), font=font)
    got = scene.print_distance_on_image(image.copy(), humans, cols)
    assert got.dtype == np.uint8 and np.array_equal(got, np.asarray(want)) and not np.array_equal(got, image)
    # the reference's key wins when both are present
    both = [dict(h, j2d_smplx=h["j2d"], j2d=h["j2d"] + 1000) for h in humans]
    assert np.array_equal(scene.print_distance_on_image(image.copy(), both, cols), got)
    # K: the 2D joints are j3d projected with it
    z = 2.0 + np.arange(127, dtype=np.float32)[None, :, None] * 0.01
    Kl = np.array([[500.0, 0, 10.0], [0, 400.0, 20.0], [0, 0, 1]], np.float32)
    j3d = np.concatenate([(j2d - Kl[:2, 2]) / np.array([500.0, 400.0], np.float32) * z, np.broadcast_to(z, (n, 127, 1))], 2)
    proj = scene.distance_labels([dict(h, j3d=j3d[i].astype(np.float32)) for i, h in enumerate(humans)], cols, K=Kl[None])
    for lab, ref in zip(proj, labels):
        assert lab["text"] == ref["text"] and np.abs(np.array(lab["bbox"]) - np.array(ref["bbox"])).max() <= 1


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_scene_entry_is_declared_exported_and_built_like_the_renderer():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    assert "mhmr_scene_pack" in declared and "mhmr_scene_pack" in _lib.EXPORTS
    args, res = _lib._SIGS["mhmr_scene_pack"]
    assert args == [ctypes.POINTER(_lib.SceneDesc), ctypes.c_void_p] and res is ctypes.c_int
    assert "int mhmr_scene_pack(const mhmr_scene_desc* d, void* stream);" in header
    assert "#define MHMR_VERSION 106 " in header and _lib.VERSION == 106
    assert "scene.hip" in _lib.SOURCES and "-ffp-contract=off" in _lib.EXTRA_FLAGS["scene.hip"]


def test_scene_descriptor_has_the_field_order_of_the_header():
    assert [n for n, _ in _lib.SceneDesc._fields_] == FIELDS
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    body = header[header.index("typedef struct {\n    int P, V, F;"):header.index("} mhmr_scene_desc;")]
    pos = [body.index(tok) for tok in ("P,", "V,", "F;", "verts;", "vstride;", "faces;", "adj_off;", "adj;", "transform;", "out;",
                                       "bounds;")]
    assert pos == sorted(pos)
    assert ctypes.sizeof(_lib.SceneDesc) == 3 * 4 + 4 + 8 * 8              # three ints, padding, eight 8-byte fields


def test_scene_descriptor_matches_compiled_sizeof_and_offsetof(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler to compare the compiled layout with")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mhmr.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(mhmr_scene_desc));\n' +
                   "".join(f'  printf(" %zu", offsetof(mhmr_scene_desc, {n}));\n' for n in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.SceneDesc)] + [getattr(_lib.SceneDesc, n).offset for n in FIELDS]


def _desc(**kw):
    """A descriptor that passes every check, with made-up pointers: every call below must fail a check (or have nothing to do); a
    call that passed them all would launch on those pointers."""
    d = _lib.SceneDesc()
    d.P, d.V, d.F, d.vstride = 3, 100, 196, 300
    d.verts = d.faces = d.adj_off = d.adj = d.out = d.bounds = 4096
    d.transform = None
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_scene_pack_checks_its_arguments_before_any_launch():
    _lib.build()
    lib = _lib.lib()
    call = lambda **kw: lib.mhmr_scene_pack(ctypes.byref(_desc(**kw)), None)
    assert lib.mhmr_scene_pack(None, None) == BAD_ARG
    assert call(V=0) == BAD_SHAPE and call(V=-5) == BAD_SHAPE
    assert call(F=-1) == BAD_SHAPE
    assert call(P=-1) == BAD_SHAPE
    assert call(vstride=299) == BAD_SHAPE and call(vstride=0) == BAD_SHAPE
    assert call(out=None) == BAD_SHAPE
    assert call(P=2 ** 31 - 1, V=2 ** 31 - 1, vstride=2 ** 40) == BAD_SHAPE     # a grid that does not fit
    assert call(verts=None) == BAD_ARG and call(bounds=None) == BAD_ARG
    assert call(faces=None) == BAD_ARG and call(adj_off=None) == BAD_ARG and call(adj=None) == BAD_ARG
    assert call(P=0) == 0 and call(P=0, out=None, verts=None, bounds=None) == 0  # nothing to do: no launch
    assert call(P=0, V=0) == BAD_SHAPE                                           # the shape checks come first
