"""-m "not gpu": the host side of the differentiable rasteriser (multi_hmr_amd/raster.py, include/mhmr.h mhmr_raster_desc): the three
forms of tests/raster_oracle.py against each other and against the keys, gradcheck of the fp64 forward with fixed keys, the stale rule,
the entry points (declared, exported, bound, the descriptor's layout, every refusal before any launch) and ``depth_loss`` by hand."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import maps_oracle as mo
import raster_oracle as rso
import render_oracle as ro
from multi_hmr_amd import _lib, raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("mhmr_raster_workspace_bytes", "mhmr_raster_interpolate", "mhmr_raster_backward")
DESC_FIELDS = ["B", "NV", "H", "W", "P", "V", "F", "C", "verts", "vstride", "faces", "adj_off", "adj", "image_index", "K", "view_Rt", "keys", "attr",
               "astride", "znear", "cull_back", "depth", "bary", "out_attr", "g_depth", "g_bary", "g_out_attr", "g_verts", "g_attr", "workspace",
               "workspace_bytes"]
H, W = 29, 37


def spheres(NV=1):
    """Two overlapping icosphere(1) meshes in image 0 of two, a third person of no image; optionally three views."""
    sv, faces = ro.icosphere(1)
    centres = np.float32([[-0.3, 0.1, 3.0], [0.25, -0.1, 3.6], [0.0, 0.0, 3.0]])
    verts = (sv[None] * np.float32([0.75, 0.9, 0.8])[:, None, None] + centres[:, None]).astype(np.float32)
    idx = np.array([0, 0, 5], np.int32)
    K = np.float32([[[0.9 * W, 0, W / 2 + 0.3], [0, 0.9 * W, H / 2 - 0.2], [0, 0, 1]], [[W, 0, W / 2], [0, W, H / 2], [0, 0, 1]]])
    Rt = None
    if NV > 1:
        from multi_hmr_amd import demo
        o = demo.orbit_extrinsics(centres[:2].mean(0), "y", [0.0, 25.0, -40.0][:NV]).astype(np.float32)
        Rt = np.stack([o, o[::-1]])
    return verts, idx, K, faces, Rt


def cotangents(shape, C_, seed):
    g = np.random.default_rng(seed)
    return g.standard_normal(shape), g.standard_normal(shape + (3,)), g.standard_normal(shape + (C_,))


@pytest.mark.parametrize("NV", [1, 3])
def test_the_three_oracle_forms_agree(NV):
    verts, idx, K, faces, Rt = spheres(NV)
    keys = mo.scene_keys(verts, idx, K, faces, H, W, Rt)
    attr = np.random.default_rng(0).standard_normal((3, 42, 3)).astype(np.float32)
    fwd = rso.forward_np(verts, idx, K, faces, H, W, keys, Rt, attr)
    drawn = keys != ro.KEY_NONE
    assert drawn.any() and np.array_equal(fwd["owned"], drawn) and not fwd["owned"][1].any()
    # the depth is the key's high word, bit for bit; the barycentrics are a partition of one
    assert np.array_equal(fwd["depth"].view(np.uint32)[drawn], (keys[drawn] >> np.uint64(32)).astype(np.uint32))
    assert (fwd["depth"][~drawn] == 0).all() and (fwd["bary"][~drawn] == 0).all() and (fwd["attr"][~drawn] == 0).all()
    assert np.abs(fwd["bary64"][drawn].sum(-1) - 1).max() < 1e-12 and (fwd["bary64"][drawn] >= 0).all()
    assert np.array_equal(fwd["person"], np.where(drawn, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64) // 80, -1))
    # torch fp64, the same route
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float32).astype(np.float64))
    depth, bary, out = rso.forward_torch(t64(verts), t64(attr), fwd, K, faces, Rt)
    for got, want in ((depth, fwd["depth64"]), (bary, fwd["bary64"]), (out, fwd["attr64"])):
        assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # the closed form against autograd of the edge-function route, each cotangent alone and all together
    gd, gb, ga = cotangents(keys.shape, 3, 1)
    gd[~drawn] = np.nan
    for kw in (dict(g_depth=gd), dict(g_bary=gb), dict(g_attr=ga), dict(g_depth=gd, g_bary=gb, g_attr=ga)):
        gv_c, ga_c = rso.backward_closed(verts, attr, fwd, K, faces, Rt, **kw)
        gv_a, ga_a = rso.backward_autograd(verts, attr, fwd, K, faces, Rt, **kw)
        assert np.isfinite(gv_c).all() and np.abs(gv_a).max() > 0
        assert np.abs(gv_c - gv_a).max() <= 1e-9 * np.abs(gv_a).max(), kw.keys()
        assert np.abs(ga_c - ga_a).max() <= 1e-9 * max(np.abs(ga_a).max(), 1e-300), kw.keys()
        assert (gv_c[2] == 0).all() and (ga_c[2] == 0).all()                                    # the person of no image
    # one table for every person: its gradient is the sum over the persons of the per-person gradient of the same table
    shared = attr[0]
    fs = rso.forward_np(verts, idx, K, faces, H, W, keys, Rt, shared)
    _, ga_s = rso.backward_autograd(verts, shared, fs, K, faces, Rt, g_attr=ga)
    _, ga_p = rso.backward_autograd(verts, np.broadcast_to(shared, attr.shape), fs, K, faces, Rt, g_attr=ga)
    assert ga_s.shape == (42, 3) and np.abs(ga_s - ga_p.sum(0)).max() <= 1e-12 * np.abs(ga_s).max()


def test_gradcheck_of_the_fp64_forward_with_fixed_keys_on_one_face():
    verts = np.float32([[[-0.6, -0.5, 2.0], [0.7, -0.4, 2.6], [0.1, 0.8, 3.1]]])
    faces = np.array([[0, 2, 1]], np.int32)
    K = np.float32([[[30, 0, 18.5], [0, 30, 14.5], [0, 0, 1]]])
    Rt = np.float32([[[0.96, 0.0, 0.28, 0.1], [0.0, 1.0, 0.0, -0.05], [-0.28, 0.0, 0.96, 0.2]]])
    keys = mo.scene_keys(verts, [0], K, faces, H, W, Rt, cull=False)
    attr = np.float32([[[0.5, -1.0], [1.5, 0.25], [-0.75, 2.0]]])
    fwd = rso.forward_np(verts, [0], K, faces, H, W, keys, Rt, attr, cull=False)
    assert fwd["owned"].sum() > 20
    v0 = torch.from_numpy(verts.astype(np.float64)).requires_grad_(True)
    a0 = torch.from_numpy(attr.astype(np.float64)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v, a: rso.forward_torch(v, a, fwd, K, faces, Rt), (v0, a0), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_stale_keys_are_background_and_give_no_gradient():
    verts, idx, K, faces, _ = spheres()
    keys = mo.scene_keys(verts, idx, K, faces, H, W)
    attr = np.random.default_rng(2).standard_normal((42, 2)).astype(np.float32)
    gd, gb, ga = cotangents(keys.shape, 2, 3)
    # the mesh moved out of the picture: every key is stale
    gone = verts + np.float32([40.0, 0.0, 0.0])
    fwd = rso.forward_np(gone, idx, K, faces, H, W, keys, None, attr)
    assert not fwd["owned"].any() and (fwd["depth"] == 0).all() and (fwd["bary"] == 0).all() and (fwd["attr"] == 0).all()
    for back in (rso.backward_closed, rso.backward_autograd):
        gv, gat = back(gone, attr, fwd, K, faces, None, g_depth=gd, g_bary=gb, g_attr=ga)
        assert (gv == 0).all() and (gat == 0).all()
    # moved by a pixel or so: some keys still fit, some are stale, none is an error
    near = verts + np.float32([0.06, 0.0, 0.0])
    fwd = rso.forward_np(near, idx, K, faces, H, W, keys, None, attr)
    drawn = keys != ro.KEY_NONE
    assert fwd["owned"].any() and (drawn & ~fwd["owned"]).any() and not (fwd["owned"] & ~drawn).any()
    assert np.isfinite(fwd["depth64"]).all() and (fwd["depth"][~fwd["owned"]] == 0).all()
    # a face index outside [0, V) and vertices that are NaN: stale, not dereferenced, no NaN
    bad = faces.copy()
    bad[:40, 1] = 42
    assert not rso.forward_np(verts, idx, K, bad, H, W, keys)["owned"].all()
    nanv = verts.copy()
    nanv[1] = np.nan
    fwd = rso.forward_np(nanv, idx, K, faces, H, W, keys, None, attr)
    assert fwd["owned"].any() and (fwd["person"] != 1).all() and np.isfinite(fwd["attr"]).all()


def test_entries_declared_exported_and_in_the_build():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    _lib.build()
    L = _lib.lib()
    for sym in SYMS:
        assert sym in declared and sym in _lib.EXPORTS and getattr(L, sym) is not None, sym
    assert "mhmr_raster_desc" in header and "raster_grad.hip" in _lib.SOURCES
    assert _lib.EXTRA_FLAGS["raster_grad.hip"] == _lib.EXTRA_FLAGS["render.hip"] == ["-ffp-contract=off"]
    src = open(os.path.join(_lib.CSRC, "raster_grad.hip")).read()
    assert '#include "render_shared.h"' in src and "tri_setup(const double" not in src                # one definition of the geometry
    assert not re.search(r"atomicAdd\s*\(\s*[^)]*(?:float|double)", src) and "unsafeAtomicAdd" not in src
    assert re.search(r"#define MHMR_VERSION 106\b", header) and _lib.VERSION == 106                  # additive
    import multi_hmr_amd
    for name in ("rasterize", "depth_loss", "Raster"):
        assert name in multi_hmr_amd.__all__ and getattr(multi_hmr_amd, name) is getattr(raster, name)


def test_descriptor_matches_compiled_sizeof_and_offsetof(tmp_path):
    assert [n for n, _ in _lib.RasterDesc._fields_] == DESC_FIELDS
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler to compare the compiled layout with")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mhmr.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(mhmr_raster_desc));\n' +
                   "".join(f'  printf(" %zu", offsetof(mhmr_raster_desc, {n}));\n' for n in DESC_FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.RasterDesc)] + [getattr(_lib.RasterDesc, n).offset for n in DESC_FIELDS]


def _desc(**kw):
    """A descriptor that passes every check of both entries (C = 0, a depth output, a depth cotangent), with made-up pointers."""
    d = _lib.RasterDesc()
    d.B, d.NV, d.H, d.W, d.P, d.V, d.F, d.C, d.vstride, d.znear, d.cull_back = 2, 3, 48, 64, 3, 42, 80, 0, 126, 0.05, 1
    d.verts = d.faces = d.adj_off = d.adj = d.image_index = d.K = d.keys = d.depth = d.g_depth = d.g_verts = d.workspace = 256
    d.workspace_bytes = 1 << 30
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entries_refuse_bad_input_before_launch():
    """Every call below returns before anything is launched: the pointers are never dereferenced."""
    _lib.build()
    L = _lib.lib()
    fwd, bwd, wsb = L.mhmr_raster_interpolate, L.mhmr_raster_backward, L.mhmr_raster_workspace_bytes
    assert fwd(None, None) == -1 and bwd(None, None) == -1 and wsb(None, 1) == -1
    shapes = (dict(B=0), dict(NV=0), dict(B=300, NV=300), dict(H=0), dict(W=0), dict(P=-1), dict(V=0), dict(F=0), dict(vstride=125),
              dict(P=70000, F=70000), dict(P=30000, F=60000), dict(P=70000, V=70000, vstride=210000), dict(C=-1), dict(C=17),
              dict(C=3, astride=125))
    for bad in shapes:
        assert fwd(C.byref(_desc(**bad)), None) == -2 and bwd(C.byref(_desc(**bad)), None) == -2 and wsb(C.byref(_desc(**bad)), 1) == -2, bad
    for bad in (dict(znear=0.0), dict(znear=float("nan")), dict(keys=None), dict(verts=None), dict(faces=None), dict(image_index=None),
                dict(K=None)):
        assert fwd(C.byref(_desc(**bad)), None) == -1 and bwd(C.byref(_desc(**bad)), None) == -1, bad
    # attributes: present iff an attribute output (forward) or an attribute cotangent / gradient (backward) is asked for
    assert fwd(C.byref(_desc(C=3, attr=256)), None) == -1 and fwd(C.byref(_desc(C=3, out_attr=256)), None) == -1
    assert fwd(C.byref(_desc(C=0, attr=256, out_attr=256)), None) == -2
    assert bwd(C.byref(_desc(C=3, attr=256)), None) == -1 and bwd(C.byref(_desc(C=3, g_out_attr=256)), None) == -1
    assert bwd(C.byref(_desc(C=3, g_attr=256)), None) == -1 and bwd(C.byref(_desc(C=0, attr=256, g_attr=256)), None) == -2
    # the backward's own pointers and its workspace
    for bad in (dict(g_verts=None), dict(adj_off=None), dict(adj=None), dict(workspace=None)):
        assert bwd(C.byref(_desc(**bad)), None) == -1, bad
    one, two, nine = (wsb(C.byref(_desc()), n) for n in (1, 2, 9))
    assert one >= 3 * 80 * (9 * 8 + 4) and two - one == one - 256 and nine - one == 8 * (one - 256)              # linear in the pass size
    assert wsb(C.byref(_desc(P=1000)), 2) == two and wsb(C.byref(_desc()), 0) == -2                             # and independent of P
    three = wsb(C.byref(_desc(C=3)), 1)
    assert three >= 3 * 80 * ((9 + 3 * 3) * 8 + 4) and raster.pass_bytes((48, 64), 80, 3) == one and raster.pass_bytes((48, 64), 80, 3, 3) == three
    assert bwd(C.byref(_desc(workspace_bytes=one - 1)), None) == -2 and bwd(C.byref(_desc(workspace_bytes=0)), None) == -2
    # nobody: the backward has nothing to write and launches nothing; the forward with no output asked for launches nothing
    assert bwd(C.byref(_desc(P=0, verts=None, faces=None, image_index=None, g_verts=None, workspace=None)), None) == 0
    assert fwd(C.byref(_desc(depth=None)), None) == 0


def test_depth_loss_value_and_gradient_by_hand():
    depth = torch.tensor([[[2.0, 0.0, 3.0], [1.5, 2.5, 0.0]]], requires_grad=True)
    mask = depth.detach() > 0
    r = raster.Raster(depth, None, None, None, None, mask, None)
    target = torch.tensor([[[2.2, 9.0, float("nan")], [1.0, 2.5, 1.0]]])
    valid = torch.tensor([[[True, True, True], [True, False, True]]])
    # in the sum: (0, 0) d = -0.2 and (1, 0) d = 0.5; (0, 1) and (1, 2) are background, (0, 2) has no target, (1, 1) is not valid
    sig = 0.25
    s = np.array([0.2, 0.5]) ** 2 / sig ** 2
    for robust, val, dvds in (("l2", s.sum(), np.ones(2)), ("gmof", (s / (1 + s)).sum(), 1 / (1 + s) ** 2)):
        depth.grad = None
        loss = raster.depth_loss(r, target, valid, sigma=sig, robust=robust)
        loss.backward()
        assert abs(float(loss.detach()) - val) <= 1e-6 * val
        want = np.zeros((1, 2, 3))
        want[0, 0, 0], want[0, 1, 0] = dvds[0] * 2 * -0.2 / sig ** 2, dvds[1] * 2 * 0.5 / sig ** 2
        assert np.abs(depth.grad.numpy() - want).max() <= 1e-5 * np.abs(want).max() and bool(torch.isfinite(depth.grad).all())
    assert float(raster.depth_loss(r, target.nan_to_num(1.0), sigma=sig, robust="l2")) > float(raster.depth_loss(r, target, valid, sigma=sig, robust="l2"))
    with pytest.raises(ValueError):
        raster.depth_loss(r, target, robust="huber")
    with pytest.raises(ValueError):
        raster.depth_loss(r, target[:, :1])
