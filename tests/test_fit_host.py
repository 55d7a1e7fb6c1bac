"""-m "not gpu": the host side of the keypoint fit (csrc/fit.hip, multi_hmr_amd/fit.py) -- header / binding / version
agree, mhmr_fit_keypoints validates everything before its first launch (so every case runs without a GPU), the tables of
``BodyModel.keypoint_model()``, the detector layouts, and the oracle of tests/fit_oracle.py pinned by ``torch.autograd.gradcheck``."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import fit_oracle as fo
import gt_oracle as go
import synthetic
from multi_hmr_amd import COCO17, OPENPOSE_BODY25, BodyModel, KeypointFitter, _lib, fit, keypoints_by_name
from multi_hmr_amd.constants import SMPLX_JOINT_NAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE = -1, -2
ENTRIES = {"mhmr_fit_keypoints_workspace_bytes", "mhmr_fit_keypoints"}
F64 = torch.float64
S, NB = 224, 10


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
    assert "fit.hip" in _lib.SOURCES and "adam_element.h" in _lib.HEADERS
    assert _lib.EXTRA_FLAGS["fit.hip"] == _lib.EXTRA_FLAGS["optim.hip"] == ["-ffp-contract=off"]      # one Adam element, rounded one way
    assert _struct_fields(header, "mhmr_fit_desc") == [f[0] for f in _lib.FitDesc._fields_]
    assert "#define MHMR_FIT_L2 0" in header and "#define MHMR_FIT_GMOF 1" in header and _lib.FIT_ROBUST == {"l2": 0, "gmof": 1}
    _lib.build()
    lib = _lib.lib()
    assert lib.mhmr_version() == 106
    assert all(hasattr(lib, n) for n in ENTRIES)
    # the element function exists once: optim.hip and fit.hip include it, neither restates it
    csrc = os.path.join(ROOT, "multi_hmr_amd", "csrc")
    for name in ("optim.hip", "fit.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "adam_element.h"' in text and "void adam_element(" not in text, name


# ---------------------------------------------------------------------------------------------------- validation
def _consts(**over):
    """The keypoint model's shapes with pointers that are never dereferenced."""
    c = _lib.BodyConsts()
    c.V, c.Vp, c.J, c.nc, c.K, c.E, c.L = 172, 192, 55, 20, 20 + 9 * 54, 21, 51
    for n, t in c._fields_:
        if t is _lib._vp:
            setattr(c, n, 64)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _bwd_consts(**over):
    b = _lib.BodyBwdConsts()
    b.n, b.inv_ptr, b.inv_joint, b.inv_w = 21 + 3 * 51, 64, 64, 64
    for k, v in over.items():
        setattr(b, k, v)
    return b


def _desc(c=None, bc=None, **over):
    _lib.build()
    c, bc = c if c is not None else _consts(), bc if bc is not None else _bwd_consts()
    d = _lib.FitDesc()
    d._keep = (c, bc)
    d.c, d.bc = C.pointer(c), C.pointer(bc)
    d.P, d.nb, d.ldr, d.patch, d.nearness, d.center_joint, d.fn = 3, 10, 341, 14, 1, 15, 387.0
    for n, t in d._fields_:
        if t is _lib._vp:
            setattr(d, n, 64)
    d.sigma, d.robust = 50.0, 1
    d.lambda_pose = d.lambda_shape = d.lambda_depth = d.lambda_expr = d.lambda_loc = 0.1
    d.steps, d.step0, d.lr, d.beta1, d.beta2, d.eps = 2, 0, 0.01, 0.9, 0.999, 1e-8
    P = over.get("P", 3)
    d.workspace_bytes = max(int(_lib.lib().mhmr_fit_keypoints_workspace_bytes(C.byref(c), P if 0 <= P <= 65535 else 1)), 0)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _run(d):
    return _lib.lib().mhmr_fit_keypoints(C.byref(d) if d is not None else None, None)


REQUIRED = ("readout", "offset", "readout0", "offset0", "det_b", "det_y", "det_x", "K", "keypoints", "confidence", "mask", "exp_avg", "exp_avg_sq",
            "workspace")
BAD_ARGS = ([{n: None} for n in REQUIRED] +
            [dict(P=-1), dict(steps=-1), dict(step0=-1), dict(sigma=0.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(robust=2),
             dict(robust=-1), dict(lambda_pose=-1.0), dict(lambda_shape=float("nan")), dict(lambda_depth=float("inf")), dict(lambda_expr=-0.5),
             dict(lambda_loc=-1e-3), dict(fn=0.0), dict(fn=float("nan")), dict(lr=0.0), dict(lr=float("inf")), dict(beta1=1.0), dict(beta2=-0.1),
             dict(eps=-1.0), dict(center_joint=127), dict(patch=0), dict(workspace_bytes=1024), dict(step0=2 ** 31 - 1)])


@pytest.mark.parametrize("over", BAD_ARGS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_bad_arguments_are_refused_before_any_launch(over):
    assert _run(_desc(**over)) == BAD_ARG


def test_bad_models_are_refused_before_any_launch():
    assert _run(None) == BAD_ARG
    d = _desc()
    d.c = None
    assert _run(d) == BAD_ARG
    d = _desc()
    d.bc = None
    assert _run(d) == BAD_ARG
    assert _run(_desc(bc=_bwd_consts(n=173))) == BAD_ARG                         # not E + 3 L entries
    assert _run(_desc(bc=_bwd_consts(inv_ptr=None))) == BAD_ARG
    for field in ("vtemp", "basis", "J0", "JS", "parents", "weights", "extra_idx", "lmk_idx", "lmk_bary"):
        assert _run(_desc(c=_consts(**{field: None}))) == BAD_ARG, field


SHAPES = [dict(nb=11), dict(nb=11, ldr=342), dict(ldr=340), dict(P=65536)]


@pytest.mark.parametrize("over", SHAPES, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_bad_shapes_are_refused_before_any_launch(over):
    assert _run(_desc(**over)) == BAD_SHAPE


def test_the_model_must_be_an_smplx_chain_within_the_body_kernels_limits():
    _lib.build()
    lib = _lib.lib()
    smpl = _consts(J=24, K=10 + 9 * 23, nc=10, L=0)                              # SMPL: 24 joints, no expression
    for c in (smpl, _consts(Vp=100), _consts(K=100), _consts(nc=5, K=5 + 9 * 54), _consts(nc=80, K=80 + 9 * 54), _consts(L=9000), _consts(V=0)):
        assert lib.mhmr_fit_keypoints_workspace_bytes(C.byref(c), 3) == BAD_SHAPE
        assert _run(_desc(c=c)) == BAD_SHAPE
    assert lib.mhmr_fit_keypoints_workspace_bytes(None, 3) == BAD_ARG and lib.mhmr_fit_keypoints_workspace_bytes(C.byref(_consts()), -1) == BAD_ARG


def test_nobody_launches_nothing_and_the_workspace_grows_with_the_persons():
    _lib.build()
    lib = _lib.lib()
    assert _run(_desc(P=0, readout=None, keypoints=None, workspace=None, workspace_bytes=0)) == 0
    assert _run(_desc(P=0, steps=0, exp_avg=None, exp_avg_sq=None)) == 0
    c = _consts()
    sizes = [int(lib.mhmr_fit_keypoints_workspace_bytes(C.byref(c), P)) for P in (0, 1, 3, 8, 9, 160)]
    assert sizes[0] >= 0 and all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    # value-and-gradient only needs no moments, but everything else
    assert _run(_desc(steps=0, exp_avg=None, exp_avg_sq=None, keypoints=None)) == BAD_ARG
    assert _run(_desc(P=0, sigma=-1.0)) == BAD_ARG                              # the scalars are checked whatever P is


# ---------------------------------------------------------------------------------------------------- the keypoint model
@functools.lru_cache(maxsize=None)
def bodies():
    data = synthetic.make_smplx_data(seed=0)
    full = BodyModel(data, "smplx", num_betas=NB)
    return data, full, full.keypoint_model()


def test_keypoint_model_tables():
    _, full, km = bodies()
    assert full.keypoint_model() is km and km.model_type == "smplx"
    ids = km.vertex_ids
    want = np.unique(np.concatenate([full.extra_joint_verts, full.lmk_vidx.reshape(-1)]))
    assert np.array_equal(ids, want) and np.all(np.diff(ids) > 0) and km.num_vertices == len(ids) <= 21 + 3 * 51
    assert km.num_joints == 55 and km.num_out_joints == 127
    # the renumbering is a bijection onto the picked set
    assert np.array_equal(ids[km.extra_joint_verts], full.extra_joint_verts) and np.array_equal(ids[km.lmk_vidx], full.lmk_vidx)
    used = np.unique(np.concatenate([km.extra_joint_verts, km.lmk_vidx.reshape(-1)]))
    assert np.array_equal(used, np.arange(len(ids)))
    # gathered columns, shared chain
    for name in ("v_template", "shapedirs", "posedirs", "lbs_weights"):
        assert np.array_equal(getattr(km, name), getattr(full, name)[ids]), name
    assert km.lmk_bary is full.lmk_bary and km.parents is full.parents
    cpu = torch.device("cpu")
    pk, pf = km._consts(cpu), full._consts(cpu)
    assert pk["struct"].V == len(ids) and pk["struct"].Vp == 192 and pf["struct"].Vp == 10496 and pk["struct"].K == pf["struct"].K
    assert torch.equal(pk["J0"], pf["J0"]) and torch.equal(pk["JS"], pf["JS"]) and torch.equal(pk["parents"], pf["parents"])
    idt = torch.from_numpy(ids)
    for name, axis in (("vtemp", 1), ("basis", 2), ("weights", 1)):
        assert torch.equal(pk[name].narrow(axis, 0, len(ids)), pf[name].index_select(axis, idt)), name
        assert float(pk[name].narrow(axis, len(ids), 192 - len(ids)).abs().max()) == 0.0, name          # zero padding
    # the inverted list claims every entry once
    ptr, joint, w = km.inverted_list()
    n = 21 + 3 * 51
    assert ptr.shape == (len(ids) + 1,) and ptr[0] == 0 and ptr[-1] == n and joint.shape == w.shape == (n,) and np.all(np.diff(ptr) >= 1)
    vert = np.repeat(np.arange(len(ids)), np.diff(ptr))
    got = sorted(zip(joint.tolist(), vert.tolist(), w.tolist()))
    exp = sorted([(55 + e, int(v), 1.0) for e, v in enumerate(km.extra_joint_verts)] +
                 [(76 + l, int(km.lmk_vidx[l, f]), float(km.lmk_bary[l, f])) for l in range(51) for f in range(3)])
    assert got == exp


def test_keypoint_model_joints_equal_the_full_models_through_the_oracle():
    """The full model's vertices (gt_oracle, fp64), gathered with numpy and read through the keypoint model's own renumbered tables, give
    the full model's picked-vertex joints and landmarks."""
    data, full, km = bodies()
    body = go.OracleBody(data, "smplx", NB, dtype=F64)
    g = torch.Generator().manual_seed(3)
    pose, coef = go.random_pose(g, 2, 55), torch.randn(2, NB + 10, generator=g)
    v, j = body(pose, coef, None)
    vk = v.numpy()[:, km.vertex_ids]
    picked = vk[:, km.extra_joint_verts]
    lmk = np.einsum("lf,plfc->plc", km.lmk_bary.astype(np.float64), vk[:, km.lmk_vidx])
    assert np.array_equal(picked, j.numpy()[:, 55:76])
    assert float(np.abs(lmk - j.numpy()[:, 76:]).max()) <= 1e-15


# ---------------------------------------------------------------------------------------------------- detector layouts
def test_keypoints_by_name_and_the_two_tables():
    assert len(COCO17) == 17 and len(OPENPOSE_BODY25) == 25 and COCO17 == fo.COCO17
    for table in (COCO17, OPENPOSE_BODY25):
        assert len(set(table)) == len(table) and all(n in SMPLX_JOINT_NAMES for n in table)
    assert fit.joint_indices(COCO17)[:5] == [55, 57, 56, 59, 58] and fit.joint_indices(COCO17)[5:7] == [16, 17]
    assert fit.joint_indices(OPENPOSE_BODY25)[1] == 12 and fit.joint_indices(OPENPOSE_BODY25)[8] == 0
    g = torch.Generator().manual_seed(0)
    xy, conf = torch.rand(3, 17, 2, generator=g) * 200, torch.rand(3, 17, generator=g)
    kp, c = keypoints_by_name(COCO17, xy, conf)
    assert tuple(kp.shape) == (3, 127, 2) and tuple(c.shape) == (3, 127) and kp.dtype == c.dtype == torch.float32
    rows = fit.joint_indices(COCO17)
    assert torch.equal(kp[:, rows], xy) and torch.equal(c[:, rows], conf)
    rest = [i for i in range(127) if i not in rows]
    assert float(c[:, rest].abs().max()) == 0.0 and float(kp[:, rest].abs().max()) == 0.0
    with pytest.raises(ValueError):
        keypoints_by_name(("nose", "left_elbow_typo"), xy[:, :2], conf[:, :2])
    with pytest.raises(ValueError):
        keypoints_by_name(("nose", "nose"), xy[:, :2], conf[:, :2])
    with pytest.raises(ValueError):
        keypoints_by_name(COCO17, xy[:, :16], conf)


def test_the_fitters_arguments_and_mask(smplx_data, mean_params):
    from multi_hmr_amd import Model
    model = Model(backbone="dinov2_vits14", img_size=S, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=1, precision="f16")
    f = KeypointFitter(model, optimize=("pose", "depth"))
    m = f.column_mask(NB)
    assert torch.equal(m, fo.column_mask(NB, ("pose", "depth"))) and int(m.sum()) == 319 and float(m[318 + NB + 1:318 + NB + 3].sum()) == 0.0
    assert int(KeypointFitter(model, optimize=fit.GROUPS).column_mask(11).sum()) == 318 + 11 + 1 + 10 + 2
    for bad in (dict(robust="huber"), dict(weights=dict(hands=1.0)), dict(optimize=("pose", "feet")), dict(sigma=0.0)):
        with pytest.raises(ValueError):
            KeypointFitter(model, **bad)
    with pytest.raises(_lib.MhmrError):                                          # no CPU path
        z = torch.zeros(1, dtype=torch.long)
        f.fit(torch.zeros(1, 341), torch.zeros(1, 2), (z, z, z), torch.eye(3)[None], torch.zeros(1, 127, 2), torch.zeros(1, 127))


# ---------------------------------------------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def small_scene():
    data, mean = synthetic.make_smplx_data(seed=0), synthetic.make_mean_params(seed=0)
    init = torch.cat([torch.eye(3)[:, :2].reshape(1, 3, 2).repeat(53, 1, 1).flatten(), torch.zeros(NB + 13)])
    init[:144] = torch.as_tensor(np.asarray(mean["pose"], dtype=np.float32)).flatten()
    body = go.OracleBody(data, "smplx", NB, dtype=F64)
    return body, fo.scene(init, 2, 2, S // 14, S, 31, body, nb=NB)


@pytest.mark.parametrize("robust", ["l2", "gmof"])
def test_the_oracles_gradient_passes_gradcheck(robust):
    body, sc = small_scene()
    lam = dict(pose=0.3, shape=0.2, depth=0.1, expression=0.4, loc=0.5)
    g = torch.Generator().manual_seed(2)
    r0, o0 = sc["readout"].double(), sc["offset"].double()
    r = (r0 + 0.02 * torch.randn(r0.shape, generator=g, dtype=F64)).requires_grad_()
    o = (o0 + 0.02 * torch.randn(o0.shape, generator=g, dtype=F64)).requires_grad_()
    conf = torch.rand(2, 127, generator=g)
    conf[:, ::5] = 0.0
    fn = lambda rr, oo: fo.energy(rr, oo, r0, o0, sc["idx"], sc["K"], body, sc["keypoints"], conf, nb=NB, img_size=S, sigma=20.0, robust=robust,
                                  lam=lam, dtype=F64)[0]
    assert torch.autograd.gradcheck(fn, (r, o), eps=1e-6, atol=1e-7, rtol=1e-5, fast_mode=True)
    # the masked gradient of value_and_grad is that gradient, column by column
    mask = fo.column_mask(NB, ("pose", "depth", "loc"))
    E, gm = fo.value_and_grad(r, o, r0, o0, sc["idx"], sc["K"], body, sc["keypoints"], conf, mask, F64, nb=NB, img_size=S, sigma=20.0, robust=robust,
                              lam=lam)
    full = torch.cat(torch.autograd.grad(fn(r, o).sum(), [r, o]), 1)
    assert torch.equal(gm, full * mask.double()) and torch.equal(E, fn(r, o).detach())
    assert float(gm[:, 318:318 + NB].abs().max()) == 0.0 and float(gm[:, 318 + NB + 1:318 + NB + 3].abs().max()) == 0.0
    assert float(full[:, 318:318 + NB].abs().min()) > 0.0                        # ... which the mask, not the function, zeroed


@pytest.mark.parametrize("dtype", [F64, torch.float32])
def test_joints_that_are_not_given_may_hold_nan(dtype):
    body, sc = small_scene()
    body = body if dtype == F64 else go.OracleBody(synthetic.make_smplx_data(seed=0), "smplx", NB, dtype=dtype)
    conf = torch.ones(2, 127)
    conf[:, 40:] = 0.0
    kp_nan, kp_any = sc["keypoints"].clone(), sc["keypoints"].clone()
    kp_nan[:, 40:] = float("nan")
    kp_nan[0, 50] = float("inf")
    kp_any[:, 40:] = 123.0
    mask = fo.column_mask(NB, fo.GROUPS)
    kw = dict(nb=NB, img_size=S, sigma=30.0, robust="gmof", lam=dict(pose=0.1))
    r = sc["readout"] + 0.01
    a = fo.value_and_grad(r, sc["offset"], sc["readout"], sc["offset"], sc["idx"], sc["K"], body, kp_nan, conf, mask, dtype, **kw)
    b = fo.value_and_grad(r, sc["offset"], sc["readout"], sc["offset"], sc["idx"], sc["K"], body, kp_any, conf, mask, dtype, **kw)
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                   # a select: what the target holds changes no bit
    assert float(a[1].abs().max()) > 0


def test_the_oracles_loop_descends_and_matches_one_hand_written_adam_step():
    body, sc = small_scene()
    mask = fo.column_mask(NB, ("pose", "shape", "depth", "loc"))
    kw = dict(nb=NB, img_size=S, sigma=1.0, robust="l2", lam={})
    r, o, trace = fo.loop(sc["readout"], sc["offset"], sc["idx"], sc["K"], body, sc["keypoints"], sc["confidence"], mask, 3, F64, lr=0.01, **kw)
    assert tuple(trace.shape) == (4, 2) and bool((trace[-1] < trace[0]).all())
    _, g = fo.value_and_grad(sc["readout"], sc["offset"], sc["readout"], sc["offset"], sc["idx"], sc["K"], body, sc["keypoints"], sc["confidence"],
                             mask, F64, **kw)
    # step 1 of Adam from zero moments: p - lr * g / (|g| + eps) up to rounding; masked columns stay
    r1, _, _ = fo.loop(sc["readout"], sc["offset"], sc["idx"], sc["K"], body, sc["keypoints"], sc["confidence"], mask, 1, F64, lr=0.01, **kw)
    want = sc["readout"].double() - 0.01 * g[:, :341] / (g[:, :341].abs() + 1e-8)
    assert float((r1 - want).abs().max()) <= 1e-12
    assert torch.equal(r1[:, 318 + NB + 3:], sc["readout"].double()[:, 318 + NB + 3:])       # expression is not optimised
