"""-m "not gpu": the host side of the tracker (csrc/track.hip, multi_hmr_amd/track.py) -- header / binding / version
agree, mhmr_track_update validates everything before its first launch (so every case runs without a GPU), the size functions, the
``Tracker``'s argument errors, and the oracle of tests/track_oracle.py on the scenes the GPU tests share: its fp32 and fp64 forms give the
same ids, and those are the ids the scenes were built to give."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import track_oracle as to
from multi_hmr_amd import Tracker, _lib, track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE = -1, -2
ENTRIES = {"mhmr_track_state_bytes", "mhmr_track_workspace_bytes", "mhmr_track_update"}
S = 224


def _struct_fields(header, name):
    end = header.index("} " + name + ";")
    body = header[header.rindex("typedef struct {", 0, end):end]
    return re.findall(r"[\*\s,]([A-Za-z_0-9]+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_entries_are_declared_exported_bound_and_additive():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    assert ENTRIES <= declared and ENTRIES <= set(_lib._SIGS)
    assert declared == set(_lib.EXPORTS)
    assert "#define MHMR_VERSION 106" in header and _lib.VERSION == 106            # additive entries: the version stays
    assert "track.hip" in _lib.SOURCES and _lib.EXTRA_FLAGS["track.hip"] == _lib.EXTRA_FLAGS["fit.hip"] == ["-ffp-contract=off"]
    assert _struct_fields(header, "mhmr_track_desc") == [f[0] for f in _lib.TrackDesc._fields_]
    for bit, g in enumerate(_lib.TRACK_GROUPS):
        assert f"#define MHMR_TRACK_{g.upper()} {1 << bit}\n" in header
    assert f"#define MHMR_TRACK_MAX_CAPACITY {_lib.TRACK_MAX_CAPACITY}\n" in header
    _lib.build()
    lib = _lib.lib()
    assert lib.mhmr_version() == 106
    assert all(hasattr(lib, n) for n in ENTRIES)
    text = open(os.path.join(ROOT, "multi_hmr_amd", "csrc", "track.hip")).read()
    code = re.sub(r"//.*", "", text)
    assert not re.search(r"atomic|\basm\b|hipMalloc|Synchronize", code)


# ---------------------------------------------------------------------------------------------------- validation
def _desc(**over):
    """A valid descriptor with pointers that are never dereferenced."""
    _lib.build()
    lib = _lib.lib()
    d = _lib.TrackDesc()
    d.F, d.P, d.nb, d.capacity = 4, 3, 10, 16
    for n, t in d._fields_:
        if t is _lib._vp:
            setattr(d, n, 64)
    d.fps, d.max_dist, d.max_age, d.groups, d.dcutoff = 30.0, 1.0, 5, 31, 1.0
    for g in _lib.TRACK_GROUPS:
        setattr(d, "mincutoff_" + g, 1.0)
        setattr(d, "beta_" + g, 0.007)
    for k in ("F", "nb", "capacity"):
        if k in over:
            setattr(d, k, over[k])
    cap, F = (d.capacity if 1 <= d.capacity <= 1024 else 1), max(d.F, 1)
    d.state_bytes = lib.mhmr_track_state_bytes(cap, to.width(d.nb))
    d.workspace_bytes = lib.mhmr_track_workspace_bytes(F, cap)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _run(d):
    return _lib.lib().mhmr_track_update(C.byref(d) if d is not None else None, None)


POINTERS = ("img_id", "idx_y", "idx_x", "transl", "readout", "offset", "state", "workspace", "track_id", "hits", "readout_s", "offset_s", "status")
NAN, INF = float("nan"), float("inf")
BAD_ARGS = ([{n: None} for n in POINTERS] +
            [dict(F=0), dict(F=-1), dict(P=-1), dict(capacity=0), dict(capacity=1025), dict(capacity=-3), dict(max_age=-1), dict(fps=0.0),
             dict(fps=NAN), dict(fps=INF), dict(dcutoff=0.0), dict(dcutoff=NAN), dict(max_dist=-0.5), dict(max_dist=NAN), dict(max_dist=INF),
             dict(groups=32), dict(groups=-1), dict(mincutoff_pose=0.0), dict(mincutoff_loc=NAN), dict(mincutoff_shape=INF), dict(beta_depth=-1.0),
             dict(beta_expr=NAN), dict(state_bytes=1024), dict(workspace_bytes=64), dict(state=68), dict(workspace=70)])


@pytest.mark.parametrize("over", BAD_ARGS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_bad_arguments_are_refused_before_any_launch(over):
    assert _run(_desc(**over)) == BAD_ARG


@pytest.mark.parametrize("over", [dict(P=65536), dict(nb=9), dict(nb=12), dict(nb=0)], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_bad_shapes_are_refused_before_any_launch(over):
    assert _run(_desc(**over)) == BAD_SHAPE


def test_a_null_descriptor_and_the_small_print():
    assert _run(None) == BAD_ARG
    # a group that is not selected may hold anything; nobody in the batch still needs the table, the workspace and the status
    assert _run(_desc(groups=30, mincutoff_pose=NAN, beta_pose=-1.0, state=None)) == BAD_ARG      # ... refused for the state, not the group
    assert _run(_desc(groups=1, mincutoff_pose=NAN)) == BAD_ARG
    for n in ("state", "workspace", "status"):
        assert _run(_desc(P=0, img_id=None, readout=None, track_id=None, **{n: None})) == BAD_ARG
    assert _run(_desc(nb=11, state_bytes=int(_lib.lib().mhmr_track_state_bytes(16, to.width(10))))) == BAD_ARG      # the table of the narrower row


def test_the_size_functions_are_monotone_and_refuse():
    _lib.build()
    lib = _lib.lib()
    D = to.width(10)
    assert lib.mhmr_track_state_bytes(16, D) == 64 + 16 * 40 + 16 * D * 8              # the layout of include/mhmr.h, as table_views reads it
    st = [int(lib.mhmr_track_state_bytes(c, D)) for c in (1, 2, 63, 64, 65, 256, 1024)]
    assert all(a < b for a, b in zip(st, st[1:])) and all(s % 8 == 0 for s in st)
    assert lib.mhmr_track_state_bytes(16, to.width(11)) > lib.mhmr_track_state_bytes(16, D)
    for F in (1, 2, 9, 32, 33):
        ws = [int(lib.mhmr_track_workspace_bytes(F, c)) for c in (1, 2, 64, 256, 1024)]
        assert all(a <= b for a, b in zip(ws, ws[1:])) and ws[0] < ws[-1] and all(w % 256 == 0 and w >= 8 * F * c + 4 * (F + 1) for w, c in
                                                                                  zip(ws, (1, 2, 64, 256, 1024)))
    wf = [int(lib.mhmr_track_workspace_bytes(F, 256)) for F in (1, 2, 9, 32, 33, 4096)]
    assert all(a < b for a, b in zip(wf, wf[1:]))
    for bad in ((0, D), (1025, D), (-1, D), (16, 0)):
        assert lib.mhmr_track_state_bytes(*bad) == BAD_ARG
    for bad in ((0, 16), (-1, 16), (4, 0), (4, 1025)):
        assert lib.mhmr_track_workspace_bytes(*bad) == BAD_ARG


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_the_trackers_arguments(smplx_data, mean_params):
    from multi_hmr_amd import Model
    model = Model(backbone="dinov2_vits14", img_size=S, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=1, precision="f16")
    t = Tracker(model)
    assert t.groups == track.DEFAULT_SMOOTH == to.DEFAULT_SMOOTH and t.width == to.width(10) and t.capacity == 256
    assert t.groups["shape"][1] == 0.0 and all(t.groups[g] == (1.0, 0.007) for g in _lib.TRACK_GROUPS if g != "shape")
    assert Tracker(model, smooth=None).groups == {}
    assert sorted(Tracker(model, smooth=dict(pose=None, expression=(2.0, 0.0))).groups) == ["depth", "expr", "loc", "shape"]
    assert Tracker(model, smooth=dict(expression=(2.0, 0.0))).groups["expr"] == (2.0, 0.0)
    for bad in (dict(fps=0.0), dict(fps=float("nan")), dict(max_dist=-1.0), dict(max_age=-1), dict(max_age=1.5), dict(capacity=0), dict(capacity=1025),
                dict(dcutoff=0.0), dict(smooth=dict(hands=(1.0, 0.0))), dict(smooth=dict(pose=(0.0, 0.0))), dict(smooth=dict(pose=(1.0, -1.0))),
                dict(smooth=dict(pose=(1.0,))), dict(smooth=dict(expr=(1.0, 0.0), expression=(1.0, 0.0)))):
        with pytest.raises(ValueError):
            Tracker(model, **bad)
    z = torch.zeros(1, dtype=torch.long)
    cpu = dict(readout=torch.zeros(1, 341), offset=torch.zeros(1, 2), transl=torch.zeros(1, 3), idx=(z, z, z))
    with pytest.raises(_lib.MhmrError):                                          # no CPU path
        t.update(cpu, z, 1)
    with pytest.raises(ValueError):
        t.update(cpu, z, 0)
    with pytest.raises(ValueError):
        t.update(dict(readout=cpu["readout"]), z, 1)
    assert t.state_dict() == dict(table=None, capacity=256, width=341)
    with pytest.raises(ValueError):
        Tracker(model, capacity=8).load_state_dict(t.state_dict())
    t.reset()                                                                    # before any update: nothing to forget


# ---------------------------------------------------------------------------------------------------- the oracle
def oracle(sc, dtype, **over):
    return to.OracleTracker(sc["nb"], dtype=dtype, **{**sc["params"], **over})


@pytest.mark.parametrize("name", sorted(to.scenes()))
def test_the_oracles_two_forms_give_the_scenes_ids(name):
    sc, want = to.scenes()[name]
    o32, o64 = oracle(sc, np.float32), oracle(sc, np.float64)
    a, b = o32.update(**to.call_args(sc)), o64.update(**to.call_args(sc))
    assert a["status"] == b["status"] == 0
    assert to.ids_by_frame(sc, a["track_id"]) == want == to.ids_by_frame(sc, b["track_id"])
    assert np.array_equal(a["hits"], b["hits"]) and o32.next_id == o64.next_id
    for k in ("id", "missed", "hits"):
        assert np.array_equal(o32.table()[k], o64.table()[k]), k
    new = a["hits"] <= 1                                                         # a new track's rows, and a row without a slot, keep their bits
    assert np.array_equal(a["readout"][new], sc["readout"][new]) and np.array_equal(a["offset"][new], sc["offset"][new])
    assert np.array_equal(a["hits"] == 0, a["track_id"] == -1)


def test_the_crossing_needs_the_velocity_term():
    sc, want = to.scenes()["crossing"]
    still = oracle(sc, np.float32, predict=False).update(**to.call_args(sc))
    assert to.ids_by_frame(sc, still["track_id"]) == [[0, 1]] * 4 != want


def test_the_oracle_refuses_disordered_image_ids_and_lets_time_pass():
    sc, _ = to.scenes()["leave_and_return"]
    o = oracle(sc, np.float32)
    args = to.call_args(sc, (0, 2))
    bad = dict(args, img_id=args["img_id"][::-1].copy())
    out = o.update(**bad)
    assert out["status"] == 1 and np.all(out["track_id"] == -1) and np.all(out["hits"] == 0) and o.next_id == 0 and not o.hits.any()
    assert o.update(**dict(args, img_id=args["img_id"] + 1))["status"] == 1      # outside [0, F)
    o.update(**args)
    empty = dict(F=3, img_id=np.zeros(0, np.int64), idx_y=np.zeros(0, np.int64), idx_x=np.zeros(0, np.int64), transl=np.zeros((0, 3)),
                 readout=np.zeros((0, o.D)), offset=np.zeros((0, 2)))
    assert o.hits.sum() == 3 and o.update(**empty)["status"] == 0 and not o.hits.any()      # max_age 2: three empty frames free both


@pytest.mark.parametrize("nb", [10, 11])
def test_the_oracle_is_one_recursion_and_its_fp32_form_is_close(nb):
    sc = to.filter_scene(nb)
    whole32, whole64 = oracle(sc, np.float32), oracle(sc, np.float64)
    a, b = whole32.update(**to.call_args(sc)), whole64.update(**to.call_args(sc))
    assert np.array_equal(a["track_id"], b["track_id"]) and sorted(set(a["track_id"])) == [0, 1]
    halves = oracle(sc, np.float32)
    h = [halves.update(**to.call_args(sc, fr)) for fr in ((0, 4), (4, 8))]
    for k in ("track_id", "hits", "readout", "offset"):
        assert np.array_equal(np.concatenate([x[k] for x in h]), a[k]), k
    for k, v in whole32.table().items():
        assert np.array_equal(v, halves.table()[k]), k
    err = max(float(np.abs(a[k] - b[k]).max()) for k in ("readout", "offset"))
    moved = float(np.abs(a["readout"] - sc["readout"]).max())
    print(f"nb {nb}: fp32 oracle against fp64 {err:.3e}; the filter moved a column by up to {moved:.3f}")
    assert 0 < err < 1e-5 and moved > 0.5
    cam12 = slice(318 + nb + 1, 318 + nb + 3)                                    # cam[1:3] pass through
    assert np.array_equal(a["readout"][:, cam12], sc["readout"][:, cam12])
    # a group set to None is a select
    part = oracle(sc, np.float32, smooth=dict(to.DEFAULT_SMOOTH, pose=None, loc=None)).update(**to.call_args(sc))
    assert np.array_equal(part["readout"][:, :318], sc["readout"][:, :318]) and np.array_equal(part["offset"], sc["offset"])
    assert np.array_equal(part["readout"][:, 318:], a["readout"][:, 318:])
