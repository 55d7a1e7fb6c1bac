"""-m "not gpu": the host side of the silhouette term (multi_hmr_amd/silhouette.py, include/mhmr.h mhmr_distance_transform_desc and
mhmr_silhouette_desc): the forms of tests/silhouette_oracle.py against each other (brute-force and separable transform, closed-form and
autograd gradient, moment and pixel form of the uncovered term), gradcheck of the fp64 outside term, the entry points (declared,
exported, bound, the descriptors' layouts, every refusal before any launch, the workspace rule) and ``assign_instance_masks`` by hand."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import render_oracle as ro
import silhouette_oracle as so
from multi_hmr_amd import _lib, silhouette

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("mhmr_distance_transform_workspace_bytes", "mhmr_distance_transform", "mhmr_silhouette_workspace_bytes", "mhmr_silhouette")
DT_FIELDS = ["N", "H", "W", "src", "max_dist", "dist2", "nearest", "workspace", "workspace_bytes"]
SIL_FIELDS = ["B", "H", "W", "P", "V", "F", "verts", "vstride", "faces", "image_index", "K", "Rt", "znear", "zfar", "cull_back", "mask", "allowed",
              "sigma", "robust", "max_dist", "terms", "counts", "g_verts", "splat", "moments", "workspace", "workspace_bytes"]
H, W = 29, 37


@pytest.mark.parametrize("size", [(1, 1), (1, 37), (37, 1), (29, 37), (12, 16)])
def test_brute_force_transform_equals_the_separable_form(size):
    for name, m in so.maps_of_every_kind(*size).items():
        for R in (0, 1, 5):
            d_b, n_b = so.transform_brute(m, R)
            d_s, n_s = so.transform_separable(m, R)
            assert np.array_equal(d_b, d_s) and np.array_equal(n_b, n_s), (name, R)
            assert d_b.dtype == np.int32 and n_b.dtype == np.int32
            if not m.any():
                assert (d_b == (R * R + 1 if R else so.DIST_NONE)).all() and (n_b == -1).all()
            else:
                ok = n_b >= 0
                assert (d_b[m] == 0).all() and ((R > 0) or ok.all()) and m.reshape(-1)[n_b[ok]].all()
                yy, xx = np.nonzero(ok)
                assert np.array_equal((yy - n_b[ok] // size[1]) ** 2 + (xx - n_b[ok] % size[1]) ** 2, d_b[ok])
    # the tie rule by hand: (1, 1) is equally far from four pixels; the smallest linear index wins, not the column pass's first find
    m = np.zeros((3, 3), bool)
    m[0, 1] = m[1, 0] = m[1, 2] = m[2, 1] = True
    d, n = so.transform_brute(m)
    assert d[1, 1] == 1 and n[1, 1] == 1
    m = np.zeros((7, 7), bool)
    m[6, 3] = m[3, 6] = True                                          # from (3, 3): three below, three to the right; the upper row wins
    assert so.transform_brute(m)[1][3, 3] == 3 * 7 + 6 and so.transform_separable(m)[1][3, 3] == 3 * 7 + 6


def test_transform_equals_scipy_where_there_is_one():
    ndi = pytest.importorskip("scipy.ndimage")
    for name, m in so.maps_of_every_kind(29, 37, seed=3).items():
        if m.any():
            want = np.rint(ndi.distance_transform_edt(~m) ** 2).astype(np.int64)
            assert np.array_equal(so.transform_brute(m)[0], want), name


def scene():
    """Two icosphere(1) meshes in image 0 and one in image 1, a fourth person of no image; masks = the cover of the spheres moved by
    a few pixels; one NaN vertex and one vertex behind znear."""
    sv, faces = ro.icosphere(1)
    centres = np.float32([[-0.3, 0.1, 3.0], [0.25, -0.1, 3.6], [0.1, 0.0, 3.2], [0.0, 0.0, 3.0]])
    verts = (sv[None] * np.float32([0.55, 0.6, 0.5, 0.5])[:, None, None] + centres[:, None]).astype(np.float32)
    idx = np.array([0, 0, 1, 7], np.int32)
    K = np.float32([[[0.9 * W, 0, W / 2 + 0.3], [0, 0.9 * W, H / 2 - 0.2], [0, 0, 1]], [[W, 0, W / 2], [0, W, H / 2], [0, 0, 1]]])
    Rt = np.float32([[[0.96, 0.0, 0.28, -0.8], [0.0, 1.0, 0.0, -0.05], [-0.28, 0.0, 0.96, 0.2]], [[1, 0, 0, 0.02], [0, 1, 0, 0], [0, 0, 1, 0]]])
    mask = so.cover(verts + np.float32([0.25, -0.12, 0.0]), idx, K, faces, H, W, Rt)
    verts[0, 5] = np.nan
    verts[1, 7, 2] = 0.01
    return verts, idx, K, faces, Rt, mask


@pytest.mark.parametrize("robust", [so.L2, so.GMOF])
def test_closed_form_gradient_equals_autograd_and_moments_equal_pixels(robust):
    verts, idx, K, faces, Rt, mask = scene()
    fwd = so.forward(verts, idx, K, faces, mask, so.others_allowed(mask, idx, 2), sigma=3.0, robust=robust, R=9, Rt=Rt)
    assert (fwd["counts"][:3] > 0).all() and (fwd["counts"][3] == 0).all() and (fwd["terms"][:3] > 0).all() and (fwd["terms"][3] == 0).all()
    assert not fwd["ok"][0, 5] and not fwd["ok"][1, 7] and fwd["ok"][:3].sum() > 100
    # the torch restatement gives the numpy values; the moment form equals the pixel-by-pixel sum
    t = so.terms_torch(torch.from_numpy(verts.astype(np.float64)), idx, K, fwd, Rt).numpy()
    assert np.abs(t - fwd["terms"]).max() <= 1e-12 * fwd["terms"].max()
    m = so.term1_from_moments(verts, idx, K, fwd, Rt)
    assert np.abs(m - fwd["terms"][:, 1]).max() <= 1e-10 * fwd["terms"][:, 1].max()
    assert np.array_equal(fwd["moments"][..., 0].sum(1), fwd["counts"][:, 1])
    # every splat is owned by the smallest vertex index that falls into it
    for p in range(3):
        ok, _, _, r, c = so.project(verts[p], K, int(idx[p]), Rt, H, W)
        for n in np.nonzero(ok)[0]:
            assert fwd["splat"][p, r[n], c[n]] <= n
    g_c, g_a = so.backward_closed(verts, idx, K, fwd, Rt), so.backward_autograd(verts, idx, K, fwd, Rt)
    for k in range(2):
        assert np.isfinite(g_c[k]).all() and np.abs(g_a[k]).max() > 0
        assert np.abs(g_c[k] - g_a[k]).max() <= 1e-9 * np.abs(g_a[k]).max(), k
    assert (g_c[:, 3] == 0).all() and (g_c[:, 0, 5] == 0).all() and (g_c[:, 1, 7] == 0).all()


def test_gradcheck_of_the_fp64_outside_term_away_from_cell_borders():
    verts, idx, K, faces, Rt, mask = scene()
    verts, idx, mask = verts[2:3], idx[2:3], mask[2:3]
    fwd = so.forward(verts, idx, K, faces, mask, None, sigma=3.0, robust=so.GMOF, R=9, Rt=Rt)
    cell = fwd["cell"][0]
    frac = np.stack([cell["su"] - cell["x0"], cell["sv"] - cell["y0"]])
    keep = fwd["ok"][0] & (np.abs(frac - 0.5) < 0.45).all(0) & cell["free_u"] & cell["free_v"] & (fwd["phi"][0] > 0)
    assert keep.sum() >= 5
    fwd["ok"][0] = keep                                               # the other vertices are left out of the sum
    v0 = torch.from_numpy(verts.astype(np.float64)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: so.terms_torch(v, idx, K, fwd, Rt)[:, 0], (v0,), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_entries_declared_exported_and_in_the_build():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    _lib.build()
    L = _lib.lib()
    for sym in SYMS:
        assert sym in declared and sym in _lib.EXPORTS and getattr(L, sym) is not None, sym
    assert "mhmr_silhouette_desc" in header and "mhmr_distance_transform_desc" in header and "silhouette.hip" in _lib.SOURCES
    assert _lib.EXTRA_FLAGS["silhouette.hip"] == _lib.EXTRA_FLAGS["render.hip"] == ["-ffp-contract=off"]
    src = open(os.path.join(_lib.CSRC, "silhouette.hip")).read()
    assert '#include "render_shared.h"' in src and "tri_setup(const double" not in src                # one definition of the geometry
    assert not re.search(r"atomicAdd\s*\(\s*[^)]*(?:float|double)", src) and "unsafeAtomicAdd" not in src
    assert re.search(r"#define MHMR_VERSION 106\b", header) and _lib.VERSION == 106                  # additive
    import multi_hmr_amd
    for name in ("silhouette_loss", "distance_transform", "assign_instance_masks", "Silhouette"):
        assert name in multi_hmr_amd.__all__ and getattr(multi_hmr_amd, name) is getattr(silhouette, name)


def test_descriptors_match_compiled_sizeof_and_offsetof(tmp_path):
    assert [n for n, _ in _lib.DistanceTransformDesc._fields_] == DT_FIELDS and [n for n, _ in _lib.SilhouetteDesc._fields_] == SIL_FIELDS
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler to compare the compiled layout with")
    for struct, cls, fields in (("mhmr_distance_transform_desc", _lib.DistanceTransformDesc, DT_FIELDS), ("mhmr_silhouette_desc", _lib.SilhouetteDesc, SIL_FIELDS)):
        src = tmp_path / f"{struct}.c"
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mhmr.h"\nint main(void) {\n'
                       f'  printf("%zu", sizeof({struct}));\n' +
                       "".join(f'  printf(" %zu", offsetof({struct}, {n}));\n' for n in fields) + "  return 0;\n}\n")
        exe = tmp_path / struct
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
        got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
        assert got == [C.sizeof(cls)] + [getattr(cls, n).offset for n in fields], struct


def _dt(**kw):
    d = _lib.DistanceTransformDesc()
    d.N, d.H, d.W, d.max_dist, d.workspace_bytes = 3, 48, 64, 5, 1 << 30
    d.src = d.dist2 = d.nearest = d.workspace = 256
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _sil(**kw):
    """A descriptor that passes every check, with made-up pointers."""
    d = _lib.SilhouetteDesc()
    d.B, d.H, d.W, d.P, d.V, d.F, d.vstride, d.znear, d.zfar, d.cull_back = 2, 48, 64, 3, 42, 80, 126, 0.05, 100.0, 1
    d.sigma, d.robust, d.max_dist, d.workspace_bytes = 8.0, 1, 64, 1 << 30
    d.verts = d.faces = d.image_index = d.K = d.mask = d.terms = d.counts = d.g_verts = d.workspace = 256
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entries_refuse_bad_input_before_launch():
    """Every call below returns before anything is launched: the pointers are never dereferenced."""
    _lib.build()
    L = _lib.lib()
    dt, dtw, sil, silw = L.mhmr_distance_transform, L.mhmr_distance_transform_workspace_bytes, L.mhmr_silhouette, L.mhmr_silhouette_workspace_bytes
    assert dt(None, None) == -1 and dtw(None) == -1 and sil(None, None) == -1 and silw(None, 1) == -1
    for bad in (dict(N=-1), dict(H=0), dict(W=0), dict(H=4097), dict(W=4097), dict(N=1 << 30, H=16)):
        assert dt(C.byref(_dt(**bad)), None) == -2 and dtw(C.byref(_dt(**bad))) == -2, bad
    for bad in (dict(max_dist=-1), dict(max_dist=46341), dict(src=None), dict(workspace=None)):
        assert dt(C.byref(_dt(**bad)), None) == -1, bad
    need = dtw(C.byref(_dt()))
    assert need >= 3 * 48 * 64 * 4 and dt(C.byref(_dt(workspace_bytes=need - 1)), None) == -2
    assert dt(C.byref(_dt(N=0, src=None, workspace=None)), None) == 0 and dt(C.byref(_dt(dist2=None, nearest=None)), None) == 0
    shapes = (dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(H=4097), dict(W=4097), dict(P=-1), dict(V=0), dict(F=0), dict(vstride=125),
              dict(P=70000, F=70000), dict(P=70000, V=70000, vstride=210000))
    for bad in shapes:
        assert sil(C.byref(_sil(**bad)), None) == -2 and silw(C.byref(_sil(**bad)), 1) == -2, bad
    args = (dict(znear=0.0), dict(znear=float("nan")), dict(zfar=0.01), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
            dict(robust=2), dict(robust=-1), dict(max_dist=0), dict(max_dist=46341), dict(verts=None), dict(faces=None), dict(image_index=None),
            dict(K=None), dict(mask=None), dict(workspace=None))
    for bad in args:
        assert sil(C.byref(_sil(**bad)), None) == -1, bad
    one, two, nine = (silw(C.byref(_sil()), n) for n in (1, 2, 9))
    assert one >= 4 * 48 * 64 * 4 + 48 * 64 // 8 + 80 * 4 + 42 * 32                                              # four maps, bits, faces, moments
    assert two - one == one - 256 and nine - one == 8 * (one - 256)                                              # linear in the pass size
    assert silw(C.byref(_sil(P=1000)), 2) == two and silw(C.byref(_sil()), 0) == -2                              # and independent of P
    assert silhouette.pass_bytes((48, 64), 42, 80) == one
    assert sil(C.byref(_sil(workspace_bytes=one - 1)), None) == -2 and sil(C.byref(_sil(workspace_bytes=0)), None) == -2
    assert sil(C.byref(_sil(P=0, verts=None, faces=None, image_index=None, mask=None, workspace=None)), None) == 0   # nobody: nothing launched


def test_assign_instance_masks_by_hand():
    person = torch.full((2, 4, 6), -1, dtype=torch.int32)
    person[0, :2, :3] = 0                                             # person 0: 6 px, top left of image 0
    person[0, 2:, 3:] = 1                                             # person 1: 6 px, bottom right of image 0
    person[1, :, :2] = 2                                              # person 2: 8 px of image 1
    inst = torch.zeros((2, 3, 4, 6), dtype=torch.bool)
    inst[0, 0, 2:, 3:] = True                                         # exactly person 1: IoU 1
    inst[0, 1, :2, :2] = True                                         # 4 of person 0's 6 px: IoU 4 / 6
    inst[0, 2, :2, :3] = True                                         # exactly person 0: IoU 1 (ties with (1, 0): the lower pair first)
    inst[1, 0, :, 4:] = True                                          # touches nobody: IoU 0
    masks, matched = silhouette.assign_instance_masks(person, [0, 0, 1, 0, 5], inst)
    assert matched.tolist() == [2, 0, -1, -1, -1]                     # person 3 is drawn nowhere, person 4 has no image
    assert torch.equal(masks[0], inst[0, 2]) and torch.equal(masks[1], inst[0, 0]) and not bool(masks[2:].any())
    # a tie between two instances for one person goes to the lower instance; a person that is drawn nowhere matches nothing
    inst2 = torch.zeros((1, 2, 4, 6), dtype=torch.bool)
    inst2[0, 0, :2, :3] = inst2[0, 1, :2, :3] = True
    person2 = person[:1].clone()
    person2[0, 2:, 3:] = -1
    person2[0, :2, :3] = 0
    masks, matched = silhouette.assign_instance_masks(person2, [0, 0], inst2)
    assert matched.tolist() == [0, -1] and torch.equal(masks[0], inst2[0, 0]) and not bool(masks[1].any())
    half = torch.zeros((1, 1, 4, 6), dtype=torch.bool)
    half[0, 0, :2, 1:5] = True                                        # persons 0 (cols 0-2) and 1 (cols 3-5) both have IoU 4 / 10: the lower person
    person3 = torch.full((1, 4, 6), -1, dtype=torch.int32)
    person3[0, :2, :3], person3[0, :2, 3:] = 0, 1
    masks, matched = silhouette.assign_instance_masks(person3, [0, 0], half)
    assert matched.tolist() == [0, -1]
    masks, matched = silhouette.assign_instance_masks(person3, [], half)
    assert tuple(masks.shape) == (0, 4, 6) and tuple(matched.shape) == (0,)
    with pytest.raises(ValueError):
        silhouette.assign_instance_masks(person3, [0], half[0])
