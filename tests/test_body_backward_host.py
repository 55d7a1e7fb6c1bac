"""-m "not gpu": the host side of the body model's backward (csrc/bodymodel_bwd.hip) -- header / binding /
version agree, the entry validates everything before any launch (so every case runs without a GPU), and the per-vertex inverted list
that carries the picked-vertex joints' and landmarks' cotangents back expands to the model's own tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import synthetic
from multi_hmr_amd import BodyModel, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE = -1, -2


def _struct_fields(header, first_line, name):
    body = header[header.index(first_line):header.index("} " + name + ";")]
    return re.findall(r"[\*\s,]([A-Za-z_0-9]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_backward_entries_are_declared_bound_and_additive():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    ours = {"mhmr_body_backward", "mhmr_body_backward_workspace_bytes"}
    assert ours <= declared and ours <= set(_lib._SIGS)
    assert declared == set(_lib.EXPORTS)                                           # nothing declared and unbound, or the reverse
    assert "#define MHMR_VERSION 106" in header and _lib.VERSION == 106            # additive entries: the version stays
    assert "bodymodel_bwd.hip" in _lib.SOURCES
    assert _struct_fields(header, "typedef struct {\n    int n; ", "mhmr_body_bwd_consts") == [f[0] for f in _lib.BodyBwdConsts._fields_]
    assert _struct_fields(header, "typedef struct {\n    const mhmr_body_consts* c;", "mhmr_body_backward_desc") == \
        [f[0] for f in _lib.BodyBackwardDesc._fields_]
    _lib.build()
    assert _lib.lib().mhmr_version() == 106


def _consts(**over):
    """SMPL-X shapes; the pointers are non-null but never dereferenced: validation comes before any launch."""
    c = _lib.BodyConsts()
    c.V, c.Vp, c.J, c.nc, c.K, c.E, c.L = 10475, 10496, 55, 21, 21 + 9 * 54, 21, 51
    for n in ("vtemp", "basis", "J0", "JS", "parents", "weights", "extra_idx", "lmk_idx", "lmk_bary"):
        setattr(c, n, 64)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _desc(c=None, G=3, bc_over=None, **over):
    lib = _lib.lib()
    c = c if c is not None else _consts()
    bc = _lib.BodyBwdConsts()
    bc.n, bc.inv_ptr, bc.inv_joint, bc.inv_w = c.E + 3 * c.L, 64, 64, 64
    for k, v in (bc_over or {}).items():
        setattr(bc, k, v)
    d = _lib.BodyBackwardDesc()
    d.c, d.bc, d.G = C.pointer(c), C.pointer(bc), G
    for n in ("pose", "coef", "transl", "K", "ws_F", "ws_A", "vertices", "joints", "g_vertices", "g_joints", "g_v2d", "g_j2d", "g_pose", "g_coef",
              "g_transl", "workspace"):
        setattr(d, n, 64)
    d.workspace_bytes = max(0, lib.mhmr_body_backward_workspace_bytes(C.byref(c), max(G, 0)))
    for k, v in over.items():
        setattr(d, k, v)
    d._keep = (c, bc)
    return d


BAD_ARGS = [dict(pose=None), dict(coef=None), dict(ws_F=None), dict(ws_A=None), dict(vertices=None), dict(joints=None), dict(workspace=None),
            dict(G=-1), dict(K=None), dict(K=None, g_v2d=None), dict(K=None, g_j2d=None), dict(transl=None), dict(workspace_bytes=8),
            dict(bc_over=dict(n=3)), dict(bc_over=dict(inv_ptr=None)), dict(bc_over=dict(inv_w=None)), dict(c=_consts(basis=None)),
            dict(c=_consts(weights=None))]
BAD_SHAPES = [dict(J=65, K=21 + 9 * 64), dict(K=500), dict(Vp=10475), dict(Vp=10432), dict(V=0), dict(nc=1500, K=1500 + 9 * 54), dict(J=0), dict(E=-1)]


@pytest.mark.parametrize("over", BAD_ARGS, ids=lambda o: ",".join(o))
def test_backward_rejects_bad_arguments_before_any_launch(over):
    _lib.build()
    assert _lib.lib().mhmr_body_backward(C.byref(_desc(**over)), None) == BAD_ARG


@pytest.mark.parametrize("over", BAD_SHAPES, ids=lambda o: ",".join(o))
def test_backward_rejects_the_forwards_shape_limits_before_any_launch(over):
    _lib.build()
    lib = _lib.lib()
    c = _consts(**over)
    assert lib.mhmr_body_backward(C.byref(_desc(c=c)), None) == BAD_SHAPE
    assert lib.mhmr_body_backward_workspace_bytes(C.byref(c), 3) == BAD_SHAPE


def test_backward_null_descriptor_nobody_and_the_workspace_size():
    _lib.build()
    lib = _lib.lib()
    assert lib.mhmr_body_backward(None, None) == BAD_ARG
    d = _desc()
    d.c = None
    assert lib.mhmr_body_backward(C.byref(d), None) == BAD_ARG
    assert lib.mhmr_body_backward_workspace_bytes(None, 3) == BAD_ARG
    c = _consts()
    assert lib.mhmr_body_backward_workspace_bytes(C.byref(c), -1) == BAD_ARG
    # G == 0 launches nothing, whatever the pointers are
    d0 = _desc(G=0, pose=None, ws_F=None, workspace=None, workspace_bytes=0)
    assert lib.mhmr_body_backward(C.byref(d0), None) == 0
    assert lib.mhmr_body_backward_workspace_bytes(C.byref(c), 0) == 0
    # the partial-sum block: one slice of K + 12 J + 3 doubles per (tile range, person); with few groups of 8 there are more ranges
    slice_bytes = (c.K + 12 * c.J + 3) * 8
    sizes = {G: lib.mhmr_body_backward_workspace_bytes(C.byref(c), G) for G in (1, 8, 9, 256, 4096)}
    assert all(s > 0 and s % (G * slice_bytes) == 0 for G, s in sizes.items())
    ranges = {G: s // (G * slice_bytes) for G, s in sizes.items()}
    assert ranges[1] == ranges[8] == c.Vp // 64 and ranges[1] >= ranges[9] >= ranges[256] > ranges[4096] == 1


def _expand(model):
    """The inverted list expanded back to (vertex, joint, weight) triples."""
    ptr, joint, w = model.inverted_list()
    assert ptr.dtype == np.int32 and joint.dtype == np.int32 and w.dtype == np.float32
    assert ptr[0] == 0 and ptr[-1] == joint.size == w.size and np.all(np.diff(ptr) >= 0) and ptr.size == model.num_vertices + 1
    vert = np.repeat(np.arange(model.num_vertices), np.diff(ptr))
    for v in np.nonzero(np.diff(ptr) > 1)[0]:
        assert np.all(np.diff(joint[ptr[v]:ptr[v + 1]]) >= 0), v                   # sorted by joint inside a vertex
    return vert, joint, w


@pytest.mark.parametrize("kind", ["smplx", "smplx_1000", "smpl"])
def test_inverted_list_expands_back_to_the_models_tables(kind, smplx_data):
    if kind == "smplx":
        model = BodyModel(smplx_data, "smplx", num_betas=11)
    elif kind == "smplx_1000":
        d = dict(synthetic.make_smplx_data(3, num_verts=1000, num_faces=2000))
        d["extra_joint_verts"] = np.arange(21) * 47 + 5
        model = BodyModel(d, "smplx", num_betas=11)
    else:
        model = BodyModel(synthetic.make_smpl_data(0, "male"), "smpl", num_betas=10)
    vert, joint, w = _expand(model)
    J, E, L = model.num_joints, len(model.extra_joint_verts), len(model.lmk_vidx)
    assert joint.size == E + 3 * L == (174 if kind != "smpl" else 21)
    assert joint.min() >= J and joint.max() < model.num_out_joints
    # picked vertices: joint J + e <- vertex extra_joint_verts[e], weight exactly 1
    pick = joint < J + E
    got = np.full(E, -1)
    got[joint[pick] - J] = vert[pick]
    assert np.array_equal(got, model.extra_joint_verts) and np.all(w[pick] == 1.0) and pick.sum() == E
    # landmarks: as a dense [L, V] matrix both ways (a face may name a vertex twice: the weights add)
    dense = np.zeros((L, model.num_vertices))
    np.add.at(dense, (joint[~pick] - J - E, vert[~pick]), w[~pick].astype(np.float64))
    want = np.zeros_like(dense)
    np.add.at(want, (np.repeat(np.arange(L), 3), model.lmk_vidx.reshape(-1)), model.lmk_bary.reshape(-1).astype(np.float64))
    assert np.array_equal(dense, want)


def test_inverted_list_is_range_checked():
    d = dict(synthetic.make_smplx_data(3, num_verts=1000, num_faces=2000))
    d["extra_joint_verts"] = np.arange(21) * 47 + 5
    model = BodyModel(d, "smplx", num_betas=11)
    model.lmk_vidx = model.lmk_vidx.copy()
    model.lmk_vidx[3, 1] = 1000
    with pytest.raises(ValueError):
        model.inverted_list()


def test_differentiable_has_no_cpu_path_and_call_keeps_no_grad(smplx_data):
    model = BodyModel(smplx_data, "smplx", num_betas=11)
    with pytest.raises(_lib.MhmrError):
        model.differentiable(global_orient=torch.zeros(2, 3, requires_grad=True), betas=torch.zeros(2, 11))
    with pytest.raises(ValueError):
        model.differentiable()
    import inspect
    assert list(inspect.signature(model.differentiable).parameters) == list(inspect.signature(model.__call__).parameters)
