"""-m "not gpu": the host side of the contacts between persons (multi_hmr_amd/contact.py, include/mhmr.h mhmr_contact): the numpy oracle
(tests/contact_oracle.py) on scenes whose answers are known by hand, the entry points (declared, exported, bound, the descriptor's layout,
every refusal before any launch) and ``penetration_loss``'s gradient."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import contact_oracle as co
from multi_hmr_amd import _lib, contact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("mhmr_contact_workspace_bytes", "mhmr_contact_check_faces", "mhmr_contact")
DESC_FIELDS = ["P", "V", "F", "verts", "vstride", "image_index", "faces", "max_dist", "tau", "workspace", "workspace_bytes", "sdf",
               "nearest_person", "nearest_face", "closest", "penetration_depth", "inside_count", "contact_count", "pair_distance",
               "pair_inside", "aabb", "valid"]
INF = np.inf


# ---------------------------------------------------------------------------------------------------------- the scene builders
def test_scene_builders_are_closed_outward_and_of_the_stated_sizes():
    for (v, f), nv, nf in ((co.icosphere(2), 162, 320), (co.icosphere(3), 642, 1280), (co.box(), 8, 12), (co.torus(24, 12), 288, 576)):
        assert v.shape == (nv, 3) and f.shape == (nf, 3) and co.signed_volume(v, f) > 0
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        fwd = {(int(a), int(b)) for a, b in e}
        assert len(fwd) == len(e) and all((b, a) in fwd for a, b in fwd)               # every edge once in each direction: closed, oriented
    v, f = co.icosphere(2)
    vo, fo = co.open_sphere(2)
    assert 0 < len(fo) < len(f) and co.signed_volume(v, co.inverted(f)) < 0
    fd = co.with_degenerate(f, 5)
    assert len(fd) == len(f) + 5 and np.array_equal(co.kept_faces(v.astype(np.float32), fd), np.arange(len(f)))


# ------------------------------------------------------------------------------------------------ the oracle, answers by hand
def test_oracle_unit_box_inside_a_box_of_side_three():
    v, f = co.box()
    verts = np.stack([v, 3 * v]).astype(np.float32)
    r = co.contacts(verts, [0, 0], f, 0.10, 0.01)
    # every corner of the unit box is 1 m from three faces of the large one and inside it; the large box's corners are 1 m + from the
    # small box's inflated box and are not evaluated
    assert np.array_equal(r["sdf"], np.stack([np.full(8, -1.0), np.full(8, INF)]))
    assert r["inside_count"].tolist() == [8, 0] and r["contact_count"].tolist() == [0, 0] and r["penetration_depth"].tolist() == [1.0, 0.0]
    assert r["pair_inside"].tolist() == [[0, 8], [0, 0]] and r["pair_distance"].tolist() == [[INF, -1.0], [INF, INF]]
    assert r["nearest_person"].tolist() == [[1] * 8, [-1] * 8] and (r["nearest_face"][1] == -1).all()
    # corner 0 = (-.5, -.5, -.5): its projection on the face x = -1.5 lies on the diagonal of faces 0 and 1: face 0, the lowest index
    assert r["nearest_face"][0, 0] == 0 and r["closest"][0, 0].tolist() == [-1.5, -0.5, -0.5]
    assert np.array_equal(r["closest"][1], verts[1]) and r["valid"].tolist() == [1, 1]
    assert r["aabb"].tolist() == [[-0.5] * 3 + [0.5] * 3, [-1.5] * 3 + [1.5] * 3]
    assert r["detail"]["pair"].tolist() == [[False, True], [True, False]] and not r["detail"]["evaluated"][1, 0].any()
    assert np.allclose(np.abs(r["detail"]["w"][0, 1]), 1.0, atol=1e-12)
    assert co.guard_set(r, 0.01).sum() == 0


def test_oracle_two_boxes_two_centimetres_apart():
    v, f = co.box()
    verts = np.stack([v, v + [1.02, 0, 0]]).astype(np.float32)
    gap = float(np.float32(1.02 - 0.5)) - 0.5                                           # the fp32 coordinate of the facing side
    for tau, contact in ((0.01, 0), (0.03, 4)):
        r = co.contacts(verts, [3, 3], f, 0.10, tau)
        near_a, near_b = v[:, 0] > 0, v[:, 0] < 0                                        # the four corners of each facing side
        assert np.allclose(r["sdf"][0, near_a], gap, atol=1e-12) and np.isinf(r["sdf"][0, ~near_a]).all()
        assert np.allclose(r["sdf"][1, near_b], gap, atol=1e-12) and np.isinf(r["sdf"][1, ~near_b]).all()
        assert r["inside_count"].tolist() == [0, 0] and r["contact_count"].tolist() == [contact] * 2
        assert r["penetration_depth"].tolist() == [0, 0] and (r["pair_inside"] == 0).all()
        pd = r["pair_distance"]
        assert np.allclose([pd[0, 1], pd[1, 0]], gap, atol=1e-12) and np.isinf(pd[0, 0]) and np.isinf(pd[1, 1])
        assert ((np.minimum(pd, pd.T) <= tau).sum() == 2) == (contact > 0)               # the docstring's `touching`
        c = r["closest"][0, near_a]
        assert np.allclose(c[:, 0], 0.5 + gap, atol=1e-12) and np.array_equal(c[:, 1:], verts[0, near_a][:, 1:])
    # 2 cm apart with max_dist = 1 cm: the inflated boxes still intersect (the pair is evaluated), no vertex is within reach
    r = co.contacts(verts, [3, 3], f, 0.01, 0.01)
    assert r["detail"]["pair"][0, 1] and not r["detail"]["evaluated"].any() and np.isinf(r["sdf"]).all() and np.isinf(r["pair_distance"]).all()


def test_oracle_boxes_in_different_images_and_an_invalid_person():
    v, f = co.box()
    verts = np.stack([v, v + [0.3, 0.2, 0.1], v + [0.3, 0.2, 0.1]]).astype(np.float32)
    r = co.contacts(verts, [0, 1, 0], f, 0.10, 0.01)
    assert not r["detail"]["pair"][0, 1] and not r["detail"]["pair"][1, 2] and r["detail"]["pair"][0, 2] and r["detail"]["pair"][2, 0]
    # person 0's corner (.5, .5, .5) is the only one inside person 2 = [-.2, .8] x [-.3, .7] x [-.4, .6], 0.1 m under its face z = .6;
    # person 2's corner (-.2, -.3, -.4) is inside person 0, 0.1 m from its face z = -.5; person 1 has the image to itself
    assert np.isinf(r["sdf"][1]).all() and r["inside_count"].tolist() == [1, 0, 1] and r["pair_inside"][0, 2] == 1 == r["pair_inside"][2, 0]
    assert r["nearest_person"][0, 7] == 2 and abs(r["sdf"][0, 7] + 0.1) < 1e-6 and r["nearest_person"][2, 0] == 0 and abs(r["sdf"][2, 0] + 0.1) < 1e-6
    assert set(r["nearest_person"][0].tolist()) <= {2, -1} and abs(r["penetration_depth"][0] - 0.1) < 1e-6
    verts[2, 5, 1] = np.nan
    r = co.contacts(verts, [0, 1, 0], f, 0.10, 0.01)
    assert r["valid"].tolist() == [1, 1, 0] and not r["detail"]["pair"].any() and np.isinf(r["sdf"]).all()
    assert r["aabb"][2].tolist() == [INF] * 3 + [-INF] * 3 and np.array_equal(r["closest"][2].astype(np.float32).view(np.uint32), verts[2].view(np.uint32))


def test_oracle_fp32_agrees_with_fp64_within_the_gate():
    v, f = co.icosphere(2)
    c0 = np.array([0.3, -0.2, 6.0])
    verts = np.stack([0.5 * v + c0, 0.5 * v + c0 + [0.6, 0.1, 0.2]]).astype(np.float32)
    r64, r32 = co.contacts(verts, [0, 0], f), co.contacts(verts, [0, 0], f, dtype=np.float32)
    assert r64["inside_count"].tolist() == [27, 27] == r32["inside_count"].tolist()
    fin = np.isfinite(r64["sdf"])
    assert np.array_equal(fin, np.isfinite(r32["sdf"])) and np.abs(r32["sdf"][fin] - r64["sdf"][fin]).max() < co.GATE < co.gate_ceiling(verts)


# --------------------------------------------------------------------------------------------------------- the entry points
def test_entries_declared_exported_and_in_the_build():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    _lib.build()
    L = _lib.lib()
    for sym in SYMS:
        assert sym in declared and sym in _lib.EXPORTS and getattr(L, sym) is not None, sym
    assert "mhmr_contact_desc" in header and "contact.hip" in _lib.SOURCES and "contact.hip" not in _lib.EXTRA_FLAGS
    src = open(os.path.join(_lib.CSRC, "contact.hip")).read()
    assert "#pragma clang fp contract(off)" in src                                      # the face normal's zero is part of the contract
    assert int(re.search(r"constexpr int TILE = (\d+);", src).group(1)) == _lib.CONTACT_FACE_TILE == contact.FACE_TILE
    assert re.search(r"#define MHMR_VERSION 106\b", header) and _lib.VERSION == 106     # additive
    import multi_hmr_amd
    for name in ("contacts", "penetration_loss", "Contacts"):
        assert name in multi_hmr_amd.__all__ and getattr(multi_hmr_amd, name) is getattr(contact, name)
    assert contact.Contacts._fields == contact.FIELDS == tuple(DESC_FIELDS[11:])


def test_descriptor_matches_compiled_sizeof_and_offsetof(tmp_path):
    assert [n for n, _ in _lib.ContactDesc._fields_] == DESC_FIELDS
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler to compare the compiled layout with")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mhmr.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(mhmr_contact_desc));\n' +
                   "".join(f'  printf(" %zu", offsetof(mhmr_contact_desc, {n}));\n' for n in DESC_FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.ContactDesc)] + [getattr(_lib.ContactDesc, n).offset for n in DESC_FIELDS]


def _desc(**kw):
    """A descriptor that passes every check, with made-up pointers: every call below must fail a check or have nothing to do."""
    d = _lib.ContactDesc()
    d.P, d.V, d.F, d.vstride, d.max_dist, d.tau = 3, 100, 196, 300, 0.10, 0.01
    d.verts = d.image_index = d.faces = d.workspace = d.sdf = 256
    d.workspace_bytes = 1 << 20
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entry_refuses_bad_input_before_launch():
    """Every call below returns before anything is launched: the pointers are never dereferenced."""
    _lib.build()
    L = _lib.lib()
    nan, inf = float("nan"), float("inf")
    assert L.mhmr_contact(None, None) == -1
    need = L.mhmr_contact_workspace_bytes(3, 100)
    assert need >= 3 * (32 + 4 + 4 * 100) and L.mhmr_contact_workspace_bytes(0, 0) > 0
    assert L.mhmr_contact_workspace_bytes(6, 100) >= need + 3 * 4 * 100                # the vertex lists grow with P V
    assert L.mhmr_contact_workspace_bytes(-1, 1) == -2 and L.mhmr_contact_workspace_bytes(50000, 1) == -2
    assert L.mhmr_contact_workspace_bytes(1, -1) == -2 and L.mhmr_contact_workspace_bytes(40000, 60000) == -2
    for bad, rc in ((dict(max_dist=-0.1), -1), (dict(max_dist=nan), -1), (dict(max_dist=inf), -1), (dict(tau=-0.01), -1), (dict(tau=nan), -1),
                    (dict(tau=0.2), -1), (dict(P=-1), -2), (dict(V=-1), -2), (dict(F=-1), -2), (dict(P=40000, V=60000, vstride=180000), -2),
                    (dict(P=50000, V=1, vstride=3), -2), (dict(vstride=299), -2), (dict(image_index=None), -1), (dict(workspace=None), -1),
                    (dict(verts=None), -1), (dict(faces=None), -1), (dict(workspace_bytes=need - 1), -2), (dict(workspace_bytes=0), -2)):
        assert L.mhmr_contact(C.byref(_desc(**bad)), None) == rc, bad
    assert L.mhmr_contact(C.byref(_desc(P=0, verts=None, image_index=None, workspace=None, workspace_bytes=0)), None) == 0   # nobody: nothing launched
    assert L.mhmr_contact(C.byref(_desc(P=0, tau=0.5)), None) == -1                     # the margins are checked even then
    f = np.array([[0, 1, 2], [2, 3, 99]], np.int32)
    assert L.mhmr_contact_check_faces(f.ctypes.data, 2, 100) == 0 and L.mhmr_contact_check_faces(f.ctypes.data, 2, 99) == -2
    f[0, 1] = -1
    assert L.mhmr_contact_check_faces(f.ctypes.data, 2, 100) == -2 and L.mhmr_contact_check_faces(None, 2, 100) == -1
    assert L.mhmr_contact_check_faces(None, 0, 100) == 0 and L.mhmr_contact_check_faces(f.ctypes.data, -1, 100) == -2


def test_contacts_refuses_on_the_host():
    with pytest.raises(ValueError):
        contact.contacts(torch.zeros(2, 8, 3), [0, 0], co.box()[1])                     # not a cuda tensor: there is no CPU path


# ---------------------------------------------------------------------------------------------------------- penetration_loss
def test_penetration_loss_gradient_is_twice_the_offset_on_the_inside_vertices():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(2, 9, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    closest = torch.randn(2, 9, 3, generator=g, dtype=torch.float64)
    sdf = torch.randn(2, 9, generator=g, dtype=torch.float64)
    sdf[0, 0], sdf[1, 8] = float("inf"), 0.0                                            # empty and exactly on the surface: not inside
    c = contact.Contacts(*[dict(sdf=sdf, closest=closest).get(n) for n in contact.FIELDS])
    loss = contact.penetration_loss(v, c)
    loss.backward()
    mask = (sdf < 0).unsqueeze(-1)
    want = torch.where(mask, 2 * (v.detach() - closest), torch.zeros_like(closest))
    assert mask.any() and not mask.all() and torch.equal(v.grad, want)
    assert torch.equal(loss.detach(), ((v.detach() - closest) ** 2 * mask).sum())
    with pytest.raises(ValueError):
        contact.penetration_loss(v, contact.Contacts(*[None] * len(contact.FIELDS)))
