"""-m "not gpu": the host side of the differentiable prediction decode (csrc/heads_bwd.hip, multi_hmr_amd/heads.py)
-- header / binding / version agree, every entry validates before any launch (so every case runs without a GPU), the 53 <-> 55 pose
mapping, and the oracle of tests/heads_oracle.py pinned against central finite differences in fp64."""
import ctypes as C
import os
import re

import pytest
import torch

import gt_oracle as go
import heads_oracle as ho
from multi_hmr_amd import _lib, heads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE = -1, -2
ENTRIES = {"mhmr_heads_decode", "mhmr_heads_place_workspace_bytes", "mhmr_heads_place_backward", "mhmr_heads_decode_backward"}
STRUCTS = {"mhmr_heads_decode_desc": _lib.HeadsDecodeDesc, "mhmr_heads_place_desc": _lib.HeadsPlaceDesc,
           "mhmr_heads_decode_backward_desc": _lib.HeadsDecodeBackwardDesc}


def _struct_fields(header, name):
    end = header.index("} " + name + ";")
    body = header[header.rindex("typedef struct {", 0, end):end]
    return re.findall(r"[\*\s,]([A-Za-z_0-9]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_entries_are_declared_bound_and_additive():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    assert ENTRIES <= declared and ENTRIES <= set(_lib._SIGS)
    assert declared == set(_lib.EXPORTS)
    assert "#define MHMR_VERSION 106" in header and _lib.VERSION == 106            # additive entries: the version stays
    assert "heads_bwd.hip" in _lib.SOURCES
    for name, cls in STRUCTS.items():
        assert _struct_fields(header, name) == [f[0] for f in cls._fields_], name
    _lib.build()
    lib = _lib.lib()
    assert lib.mhmr_version() == 106
    assert all(hasattr(lib, n) for n in ENTRIES)


def _fill(d, **over):
    """Every pointer non-null but never dereferenced: validation comes before any launch."""
    for n, t in d._fields_:
        if t is _lib._vp:
            setattr(d, n, 64)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _decode(**over):
    d = _lib.HeadsDecodeDesc()
    d.P, d.nb, d.ldr, d.patch, d.nearness, d.fn = 3, 10, 341, 14, 1, 387.0
    return _fill(d, **over)


def _decode_bwd(**over):
    d = _lib.HeadsDecodeBackwardDesc()
    d.P, d.nb, d.ldr, d.patch, d.nearness, d.fn = 3, 10, 341, 14, 1, 387.0
    return _fill(d, **over)


def _place(**over):
    d = _lib.HeadsPlaceDesc()
    d.P, d.V, d.NJ, d.center_joint = 3, 10475, 127, 15
    d.workspace_bytes = 3 * (11 + 1) * 24
    return _fill(d, **over)


DECODE_REQUIRED = ("readout", "offset", "K", "det_b", "det_y", "det_x", "loc", "rotmat", "rotvec", "shape", "expression", "dist_postprocessed", "dist")
DECODE_BWD_REQUIRED = ("readout", "offset", "K", "det_b", "det_y", "det_x", "g_readout", "g_offset")
PLACE_REQUIRED = ("verts_u", "joints_u", "transl", "gx_v", "gx_j", "g_transl_total", "workspace")
SHAPES = [dict(nb=-1), dict(nb=65, ldr=400), dict(ldr=340), dict(nb=11, ldr=341)]


@pytest.mark.parametrize("name", DECODE_REQUIRED + ("P",))
def test_decode_rejects_bad_arguments_before_any_launch(name):
    _lib.build()
    over = {"P": -1} if name == "P" else {name: None}
    assert _lib.lib().mhmr_heads_decode(C.byref(_decode(**over)), None) == BAD_ARG


@pytest.mark.parametrize("name", DECODE_BWD_REQUIRED + ("P",))
def test_decode_backward_rejects_bad_arguments_before_any_launch(name):
    _lib.build()
    over = {"P": -1} if name == "P" else {name: None}
    assert _lib.lib().mhmr_heads_decode_backward(C.byref(_decode_bwd(**over)), None) == BAD_ARG


@pytest.mark.parametrize("over", SHAPES, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_the_decodes_limit_on_nb_and_the_row_pitch(over):
    _lib.build()
    lib = _lib.lib()
    assert lib.mhmr_heads_decode(C.byref(_decode(**over)), None) == BAD_SHAPE
    assert lib.mhmr_heads_decode_backward(C.byref(_decode_bwd(**over)), None) == BAD_SHAPE


PLACE_BAD = [{n: None} for n in PLACE_REQUIRED] + [dict(P=-1), dict(K=None), dict(K=None, g_v2d=None), dict(K=None, g_j2d=None), dict(workspace_bytes=24),
                                                  dict(center_joint=127), dict(V=0), dict(NJ=0)]


@pytest.mark.parametrize("over", PLACE_BAD, ids=lambda o: ",".join(o))
def test_place_backward_rejects_bad_arguments_before_any_launch(over):
    _lib.build()
    assert _lib.lib().mhmr_heads_place_backward(C.byref(_place(**over)), None) == BAD_ARG


def test_null_descriptors_nobody_and_the_workspace_size():
    _lib.build()
    lib = _lib.lib()
    assert lib.mhmr_heads_decode(None, None) == BAD_ARG
    assert lib.mhmr_heads_place_backward(None, None) == BAD_ARG
    assert lib.mhmr_heads_decode_backward(None, None) == BAD_ARG
    # P == 0 launches nothing, whatever the pointers are
    assert lib.mhmr_heads_decode(C.byref(_decode(P=0, readout=None, rotmat=None)), None) == 0
    assert lib.mhmr_heads_decode_backward(C.byref(_decode_bwd(P=0, readout=None, g_readout=None)), None) == 0
    assert lib.mhmr_heads_place_backward(C.byref(_place(P=0, verts_u=None, workspace=None, workspace_bytes=0)), None) == 0
    # too many persons for one grid: a shape, not an argument
    assert lib.mhmr_heads_place_backward(C.byref(_place(P=65536, workspace_bytes=1 << 40)), None) == BAD_SHAPE
    # 2D cotangents absent: K is not needed
    d = _place(K=None, g_v2d=None, g_j2d=None, P=0)
    assert lib.mhmr_heads_place_backward(C.byref(d), None) == 0
    # three doubles per (person, tile of 1024 points), the joints in tiles of their own
    assert lib.mhmr_heads_place_workspace_bytes(10475, 127, 3) == 3 * (11 + 1) * 24
    assert lib.mhmr_heads_place_workspace_bytes(1024, 1025, 1) == (1 + 2) * 24
    assert lib.mhmr_heads_place_workspace_bytes(10475, 127, 0) == 0
    assert lib.mhmr_heads_place_workspace_bytes(0, 127, 1) == BAD_ARG and lib.mhmr_heads_place_workspace_bytes(5, 127, -1) == BAD_ARG


def test_pose_mapping_and_its_transpose():
    g = torch.Generator().manual_seed(1)
    r = torch.randn(2, 53, 3, generator=g)
    full = heads.pose53_to_55(r)
    assert tuple(full.shape) == (2, 55, 3)
    assert torch.equal(full[:, 0], r[:, 0]) and torch.equal(full[:, 1:22], r[:, 1:22]) and torch.equal(full[:, 22], r[:, 52])
    assert torch.equal(full[:, 23:25], torch.zeros(2, 2, 3))
    assert torch.equal(full[:, 25:40], r[:, 22:37]) and torch.equal(full[:, 40:55], r[:, 37:52])
    assert torch.equal(full, ho.pose53_to_55(r))                                   # the oracle's own statement, by index
    assert torch.equal(heads.pose55_to_53(full), r)
    # the transpose: <A r, c> == <r, A^T c>; a selection, so the same 318 products, summed in another order (fp64: 1e-13)
    c = torch.randn(2, 55, 3, generator=g).double()
    assert abs(float((full.double() * c).sum() - (r.double() * heads.pose55_to_53(c)).sum())) <= 1e-12
    assert torch.equal(heads.pose55_to_53(heads.pose53_to_55(r)), r)
    assert heads.readout_width(10) == 341 and heads.readout_width(11) == 342


def test_decode_readout_has_no_cpu_path(smplx_data, mean_params):
    from multi_hmr_amd import Model
    model = Model(backbone="dinov2_vits14", img_size=224, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=1, precision="f16")
    with pytest.raises(_lib.MhmrError):
        model.decode_readout(torch.zeros(1, 341, requires_grad=True), torch.zeros(1, 2), (torch.zeros(1, dtype=torch.long),) * 3, torch.eye(3)[None])


@pytest.mark.parametrize("center,nearness", [(15, True), (None, False)])
def test_the_oracles_gradient_against_central_differences(smplx_data, mean_params, center, nearness):
    """Pins the oracle itself: fp64 autograd against (f(r + h d) - f(r - h d)) / 2h along seeded unit directions, one person, all
    fourteen cotangents.  The function is smooth here (the report says which branches it took; a central difference across a branch
    of the quaternion is still a difference of the same smooth function), so the truncation error is O(h^2 |f'''|) and the rounding
    error O(eps |f| / h): h = 1e-5 leaves both far below the 1e-6 relative gate."""
    S, nb = 224, 10
    body = go.OracleBody(smplx_data, "smplx", nb, dtype=torch.float64)
    init = torch.cat([torch.eye(3)[:, :2].reshape(1, 3, 2).repeat(53, 1, 1).flatten(), torch.zeros(nb + 13)])
    init[:144] = torch.as_tensor(mean_params["pose"], dtype=torch.float32).flatten()
    readout, offset, idx, K = ho.make_inputs(init, 1, 1, S // 14, S, seed=5, nearness=nearness, general_K=True)
    cot = ho.make_cotangents(1, 10475, S, seed=6, nb=nb)
    kw = dict(nb=nb, img_size=S, nearness=nearness, center=center)
    g_r, g_o, report = ho.grads(readout, offset, idx, K, body, cot, torch.float64, **kw)
    assert report["in_front"] and int(report["clamp"].abs().sum()) == 0
    print("branches", report["branch"].flatten().bincount(minlength=4).tolist(), "flips", int(report["flip"].sum()))

    def f(r, o):
        out, _ = ho.decode(r, o, idx, K, body, dtype=torch.float64, **kw)
        return float(sum((out[k] * c.double()).sum() for k, c in cot.items()))

    g = torch.Generator().manual_seed(7)
    h = 1e-5
    for i in range(4):
        dr, do = torch.randn(readout.shape, generator=g, dtype=torch.float64), torch.randn(offset.shape, generator=g, dtype=torch.float64)
        n = float(torch.sqrt((dr ** 2).sum() + (do ** 2).sum()))
        dr, do = dr / n, do / n
        fd = (f(readout.double() + h * dr, offset.double() + h * do) - f(readout.double() - h * dr, offset.double() - h * do)) / (2 * h)
        an = float((g_r * dr).sum() + (g_o * do).sum())
        print(f"direction {i}: finite difference {fd:.12g} autograd {an:.12g} rel {abs(fd - an) / abs(an):.3g}")
        assert abs(fd - an) <= 1e-6 * abs(an)
    assert float(g_r[:, 318 + nb + 1:318 + nb + 3].abs().max()) == 0.0
