"""-m "not gpu": the host side of the per-pixel maps (multi_hmr_amd/maps.py, include/mhmr.h mhmr_render_maps, mhmr_render_point_visibility,
mhmr_render_amodal): ``part_labels``' tie, majority and ``groups`` rules, the SMPL-X part table, the numpy oracle (tests/maps_oracle.py)
on scenes whose answers are counted by hand, and the entry points: declared, exported, refusing bad input before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import maps_oracle as mo
import render_exact as rx
from multi_hmr_amd import _lib, maps
from multi_hmr_amd.constants import SMPLX_BODY_PARTS, SMPLX_JOINT_NAMES, SMPLX_NUM_JOINTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("mhmr_render_maps", "mhmr_render_point_visibility", "mhmr_render_amodal_workspace_bytes", "mhmr_render_amodal")
QUAD = np.array([[0, 2, 1], [0, 3, 2]], np.int32)


# ------------------------------------------------------------------------------------------------------------ part_labels
def test_part_labels_tie_majority_and_groups():
    w = np.array([[0.5, 0.5, 0.0],       # vertex 0: a tie -> the lowest joint, 0
                  [0.1, 0.2, 0.7],       # 1 -> 2
                  [0.0, 1.0, 0.0],       # 2 -> 1
                  [0.3, 0.3, 0.4],       # 3 -> 2
                  [0.0, 0.5, 0.5]])      # 4: a tie -> 1
    faces = np.array([[0, 1, 3],         # labels 0, 2, 2: the majority of the last two corners
                      [1, 0, 3],         # 2, 0, 2: first and third
                      [1, 3, 0],         # 2, 2, 0: first and second
                      [0, 1, 2],         # 0, 2, 1: all differ -> the first corner's
                      [2, 4, 4],         # 1, 1, 1
                      [3, 2, 0]])        # 2, 1, 0: all differ -> 2
    got = maps.part_labels(w, faces)
    assert got.dtype == np.uint8 and got.tolist() == [2, 2, 2, 0, 1, 2]
    # groups: joints 0 and 2 are one part (5), joint 1 another (9): the vertex labels become 5, 5, 9, 5, 9
    assert maps.part_labels(w, faces, groups=[5, 9, 5]).tolist() == [5, 5, 5, 5, 9, 5]
    assert maps.part_labels(w, np.zeros((0, 3), np.int64)).shape == (0,)
    with pytest.raises(ValueError):
        maps.part_labels(w, faces, groups=[0, 1])                   # one entry per joint
    with pytest.raises(ValueError):
        maps.part_labels(w, faces, groups=[0, 255, 1])              # 255 is the background
    with pytest.raises(ValueError):
        maps.part_labels(w, np.array([[0, 1, 5]]))


def test_part_table_covers_every_joint_and_is_symmetric():
    names, table = SMPLX_BODY_PARTS.names, SMPLX_BODY_PARTS.joint_part
    assert len(table) == SMPLX_NUM_JOINTS == 55 and all(0 <= t < len(names) for t in table)
    assert set(table) == set(range(len(names))) and len(set(names)) == len(names)          # every part is used, every name once
    swap = lambda s: "right" + s[4:] if s.startswith("left") else "left" + s[5:] if s.startswith("right") else s
    joints = SMPLX_JOINT_NAMES[:55]
    for j, t in zip(joints, table):
        assert swap(j) in joints and names[table[joints.index(swap(j))]] == swap(names[t]), j
    assert {names[t] for j, t in zip(joints, table) if not j.startswith(("left", "right"))} == {"torso", "head"}


def test_model_face_part_labels_is_part_labels_of_its_own_layer(smplx_data, mean_params):
    from multi_hmr_amd import Model
    m = Model(backbone="dinov2_vits14", img_size=224, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=1)
    lab = m.face_part_labels()
    faces = np.asarray(smplx_data["f"])
    assert lab.dtype == np.uint8 and lab.shape == (len(faces),) and lab.max() < len(SMPLX_BODY_PARTS.names)
    assert np.array_equal(lab, maps.part_labels(smplx_data["weights"], faces, SMPLX_BODY_PARTS.joint_part)) and m.face_part_labels() is lab


# ------------------------------------------------------------------------------------------------ the oracle, counted by hand
H, W, CX, CY = 24, 32, 16, 12


def _rect(u0, v0, u1, v1, Z):
    return np.stack([rx.vertex(u0, v0, Z, CX, CY), rx.vertex(u1, v0, Z, CX, CY), rx.vertex(u1, v1, Z, CX, CY), rx.vertex(u0, v1, Z, CX, CY)])


def two_rectangles():
    """Person 0: u 4.5 .. 20.5, v 4.5 .. 12.5 at Z = 2 (columns 4 .. 19, rows 4 .. 11: 128 pixels).  Person 1: u 12.5 .. 28.5,
    v 8.5 .. 16.5 at Z = 1 (columns 12 .. 27, rows 8 .. 15: 128 pixels), in front of person 0's lower right corner (columns 12 .. 19, rows
    8 .. 11: 32 pixels).  Person 2 has no image."""
    verts = np.stack([_rect(4.5, 4.5, 20.5, 12.5, 2.0), _rect(12.5, 8.5, 28.5, 16.5, 1.0), _rect(4.5, 4.5, 20.5, 12.5, 1.0)])
    return verts, np.array([0, 0, 7]), rx.cam(CX, CY)[None]


def test_oracle_two_rectangles_counted_by_hand():
    verts, idx, K = two_rectangles()
    keys = mo.scene_keys(verts, idx, K, QUAD, H, W)
    assert keys.shape == (1, 1, H, W)
    m = mo.maps(keys, 3, 2, idx, face_label=np.array([0, 3], np.uint8))
    am = mo.amodal(verts, idx, K, QUAD, H, W)
    assert m["visible_px"][:, 0].tolist() == [96, 128, 0] and am[:, 0].tolist() == [128, 128, 0]
    assert m["bbox"][:, 0].tolist() == [[4, 4, 19, 11], [12, 8, 27, 15], [W, H, -1, -1]]
    assert m["zmin"][:, 0].tolist() == [2.0, 1.0, np.inf]
    assert mo.occlusion(m["visible_px"], am)[:, 0].tolist() == [0.25, 0.0, 0.0]
    person = m["person"][0, 0]
    assert (person[8:12, 12:20] == 1).all() and (person[4:8, 4:20] == 0).all() and person[0, 0] == -1 and (person >= 0).sum() == 224
    assert m["depth"][0, 0, 5, 5] == 2.0 and m["depth"][0, 0, 9, 13] == 1.0 and m["depth"][0, 0, 0, 0] == 0.0
    assert m["face"][0, 0, 0, 0] == -1 and set(np.unique(m["face"])) == {-1, 0, 1}
    assert m["label"][0, 0, 0, 0] == 255 and (m["label_px"].sum(-1) == m["visible_px"]).all()
    # the diagonal u - 12.5 = 2 (v - 8.5) passes through the centre of column 12 + 2 k in row 8 + k: 15 - 2 k centres to its right (64 in
    # all), 2 k to its left (56), and the 8 on it go to the upper right face (0, label 0), for which it is a left edge
    assert np.array_equal(m["label_px"][1, 0], [72, 0, 0, 56])


def test_oracle_point_codes_counted_by_hand():
    verts, idx, K = two_rectangles()
    keys = mo.scene_keys(verts, idx, K, QUAD, H, W)
    pt = lambda u, v, Z: rx.vertex(u, v, Z, CX, CY)
    nan = np.float32(np.nan)
    pts = np.stack([pt(14.5, 9.5, 4.0),           # behind person 1 (depth 1): occluded
                    pt(14.5, 9.5, 0.5),           # in front of it: visible
                    pt(2.5, 20.5, 4.0),           # beside both, on a pixel nobody draws: visible
                    pt(-5.5, 9.5, 1.0),           # left of the image: outside
                    pt(14.5, 9.5, 1.0),           # on person 1's surface: visible for every tau >= 0
                    np.float32([0.0, 0.0, 0.01]),  # nearer than znear
                    np.float32([0.0, nan, 1.0]),
                    np.float32([0.0, 0.0, -1.0])])
    for tau in (0.0, 0.03):
        codes = mo.point_visibility(np.stack([pts, pts, pts]), idx, K, keys, tau=tau)
        assert codes.shape == (3, 1, 8)
        assert codes[0, 0].tolist() == codes[1, 0].tolist() == [0, 1, 1, 2, 1, 3, 3, 3], tau
        assert (codes[2] == 2).all()                                                  # a person of no image
    # the margin: 2 cm behind the surface is occluded at tau = 0 and visible at tau = 0.03
    just = np.float32([[[(14.5 - CX) * 1.02 / 64, (9.5 - CY) * 1.02 / 64, 1.02]]])
    assert mo.point_visibility(just, [0], K, keys, tau=0.0)[0, 0, 0] == 0 and mo.point_visibility(just, [0], K, keys, tau=0.03)[0, 0, 0] == 1


# --------------------------------------------------------------------------------------------------------- the entry points
def test_entries_declared_exported_and_in_the_build():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    _lib.build()
    L = _lib.lib()
    for sym in SYMS:
        assert sym in declared and sym in _lib.EXPORTS and getattr(L, sym) is not None, sym
    assert "mhmr_render_maps_desc" in header and "mhmr_point_visibility_desc" in header
    assert "render_maps.hip" in _lib.SOURCES and _lib.EXTRA_FLAGS["render_maps.hip"] == _lib.EXTRA_FLAGS["render.hip"] == ["-ffp-contract=off"]
    assert "render_shared.h" in _lib.HEADERS
    for name in ("render.hip", "render_maps.hip"):                      # one definition of the geometry, included by both
        src = open(os.path.join(_lib.CSRC, name)).read()
        assert '#include "render_shared.h"' in src and "tri_setup(const double" not in src, name
    assert re.search(r"#define MHMR_VERSION 106\b", header) and _lib.VERSION == 106                                # additive


def _maps_desc(**kw):
    d = _lib.RenderMapsDesc()
    d.B, d.NV, d.H, d.W, d.P, d.F, d.L = 2, 1, 48, 64, 3, 80, 0
    d.keys = d.image_index = d.person = 256
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entries_refuse_bad_input_before_launch():
    """Every call below returns before anything is launched: the pointers are never dereferenced."""
    _lib.build()
    L = _lib.lib()
    assert L.mhmr_render_maps(None, None) == -1
    for bad, rc in ((dict(B=0), -2), (dict(NV=0), -2), (dict(B=300, NV=300), -2), (dict(H=0), -2), (dict(W=0), -2), (dict(P=-1), -2),
                    (dict(F=0), -2), (dict(P=70000, F=70000), -2), (dict(L=256), -2), (dict(L=-1), -2), (dict(keys=None), -1),
                    (dict(image_index=None), -1), (dict(label=256), -1), (dict(label_px=256, L=4), -1),
                    (dict(label_px=256, face_label=256, L=0), -2)):
        assert L.mhmr_render_maps(C.byref(_maps_desc(**bad)), None) == rc, bad
    p = _lib.PointVisibilityDesc()
    p.B, p.NV, p.H, p.W, p.P, p.N, p.pstride, p.znear, p.tau = 2, 1, 48, 64, 3, 10, 30, 0.05, 0.03
    p.points = p.image_index = p.K = p.keys = p.out = 256
    assert L.mhmr_render_point_visibility(None, None) == -1
    for bad, rc in ((dict(B=0), -2), (dict(N=-1), -2), (dict(pstride=29), -2), (dict(P=70000, N=70000, pstride=210000), -2),
                    (dict(znear=0.0), -1), (dict(tau=-1.0), -1), (dict(tau=float("nan")), -1), (dict(out=None), -1), (dict(keys=None), -1)):
        q = _lib.PointVisibilityDesc.from_buffer_copy(p)
        for k, v in bad.items():
            setattr(q, k, v)
        assert L.mhmr_render_point_visibility(C.byref(q), None) == rc, bad
    q = _lib.PointVisibilityDesc.from_buffer_copy(p)
    q.N = 0
    assert L.mhmr_render_point_visibility(C.byref(q), None) == 0          # nothing to do, nothing launched

    def rd(**kw):
        d = _lib.RenderDesc()
        d.B, d.H, d.W, d.P, d.V, d.F, d.vstride = 2, 48, 64, 3, 42, 80, 126
        d.znear, d.zfar, d.cull_back = 0.05, 100.0, 1
        d.verts = d.faces = d.image_index = d.K = d.workspace = 256
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    one, two, nine = (L.mhmr_render_amodal_workspace_bytes(C.byref(rd()), 3, n) for n in (1, 2, 9))
    words = (48 * 64 + 31) // 32
    assert one >= 3 * words * 4 + 3 * 80 * 8 and two - one == one - 256 and nine - one == 8 * (one - 256)       # linear in the pass size
    assert L.mhmr_render_amodal_workspace_bytes(C.byref(rd(P=1000)), 3, 2) == two                               # and independent of P
    assert maps.amodal_pass_bytes((48, 64), 80, 3) == one
    for nv, n, bad, rc in ((0, 1, {}, -2), (3, 0, {}, -2), (40000, 1, {}, -2), (3, 1, dict(Rt=256), -1), (3, 1, dict(V=0), -2),
                           (3, 1, dict(vstride=100), -2), (3, 1, dict(P=70000, F=70000), -2)):
        assert L.mhmr_render_amodal_workspace_bytes(C.byref(rd(**bad)), nv, n) == rc, (nv, n, bad)
    assert L.mhmr_render_amodal_workspace_bytes(None, 1, 1) == -1 and L.mhmr_render_amodal(None, 1, None, 256, None) == -1
    assert L.mhmr_render_amodal(C.byref(rd(workspace_bytes=one - 1)), 3, None, 256, None) == -2                 # not even one person per pass
    assert L.mhmr_render_amodal(C.byref(rd(workspace_bytes=one)), 3, None, None, None) == -1
    assert L.mhmr_render_amodal(C.byref(rd(workspace_bytes=one, znear=0.0)), 3, None, 256, None) == -1
    assert L.mhmr_render_amodal(C.byref(rd(workspace_bytes=one, Rt=256)), 3, None, 256, None) == -1
    assert L.mhmr_render_amodal(C.byref(rd(P=0)), 3, None, None, None) == 0                                     # nobody: nothing launched
