"""-m "not gpu": host side of the ground-truth path -- CSR construction, model-file loading, the C ABI's new names and its argument
checks (which come before any launch), the synthetic SMPL assets, and the condition the GPU prepare tests rest on."""
import ctypes
import hashlib
import os
import pickle
import re
import sys
import types

import numpy as np
import pytest
import torch

from multi_hmr_amd import BodyModel, GroundTruth, SparseRegressor, _lib, constants
from multi_hmr_amd.bodymodel import load_body_data
from multi_hmr_amd.evaluate import csr_from_matrix
import gt_oracle as go
import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mhmr_body_forward", "mhmr_sparse_regress", "mhmr_gt_targets", "mhmr_rotvec_to_rotmat", "mhmr_project_points"}


def test_csr_from_dense_and_scipy_sparse_agree():
    import scipy.sparse as sp
    rng = np.random.RandomState(0)
    dense = np.where(rng.rand(17, 300) < 0.05, rng.randn(17, 300), 0.0).astype(np.float32)
    dense[5] = 0.0                                                       # a row without entries
    a, b = csr_from_matrix(dense), csr_from_matrix(sp.coo_matrix(dense))
    c = csr_from_matrix(torch.from_numpy(dense))
    for x, y_, z in zip(a[:3], b[:3], c[:3]):
        assert np.array_equal(x, y_) and np.array_equal(x, z)
    rowptr, col, val, shape = a
    assert shape == (17, 300) and rowptr.dtype == np.int32 and col.dtype == np.int32 and val.dtype == np.float32
    assert rowptr[5] == rowptr[6] and rowptr[-1] == np.count_nonzero(dense)
    back = np.zeros_like(dense)
    for r in range(17):
        cols = col[rowptr[r]:rowptr[r + 1]]
        assert np.all(np.diff(cols) > 0)                                 # ascending columns: the kernel's summation order
        back[r, cols] = val[rowptr[r]:rowptr[r + 1]]
    assert np.array_equal(back, dense)
    # duplicates of a COO matrix are summed, explicit zeros dropped
    m = sp.coo_matrix((np.array([1.0, 2.0, 0.0], dtype=np.float32), (np.array([0, 0, 1]), np.array([3, 3, 2]))), shape=(2, 5))
    rowptr, col, val, _ = csr_from_matrix(m)
    assert rowptr.tolist() == [0, 1, 1] and col.tolist() == [3] and val.tolist() == [3.0]
    reg = SparseRegressor(synthetic.make_smplx2smpl(0))
    assert reg.shape == (6890, 10475) and reg.nnz <= 3 * 6890
    assert int(np.diff(reg.rowptr).max()) <= 3 and reg.rowptr[1] - reg.rowptr[0] == 1
    with pytest.raises(_lib.MhmrError):
        reg(torch.zeros(1, 10475, 3))                                    # no CPU path


def test_body_data_loader_reads_npz_and_pickle_and_explains_a_chumpy_pickle(tmp_path):
    data = synthetic.make_smpl_data(0, "male")
    np.savez(tmp_path / "smpl.npz", **data)
    with open(tmp_path / "smpl.pkl", "wb") as f:
        pickle.dump(data, f, protocol=2)
    for name in ("smpl.npz", "smpl.pkl"):
        got = load_body_data(str(tmp_path / name))
        assert set(got) == set(data) and all(np.array_equal(got[k], data[k]) for k in data)
    # a pickle whose arrays are objects of a module named chumpy, which is not installed
    assert "chumpy" not in sys.modules
    mod = types.ModuleType("chumpy")

    class Ch:                                                            # noqa: B903
        def __init__(self, a):
            self.a = a
    Ch.__module__, Ch.__qualname__ = "chumpy", "Ch"
    mod.Ch = Ch
    sys.modules["chumpy"] = mod
    try:
        with open(tmp_path / "chumpy.pkl", "wb") as f:
            pickle.dump({"v_template": Ch(data["v_template"])}, f, protocol=2)
    finally:
        del sys.modules["chumpy"]
    with pytest.raises(_lib.MhmrError, match="chumpy"):
        load_body_data(str(tmp_path / "chumpy.pkl"))
    with pytest.raises(_lib.MhmrError, match="chumpy"):
        BodyModel(str(tmp_path / "chumpy.pkl"), "smpl")


def test_header_and_exports_agree_on_the_new_names_and_the_version_stays():
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    declared = set(re.findall(r"\b(?:int|long long|const char\*)\s+(mhmr_[a-z0-9_]+)\s*\(", header))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS) and declared == set(_lib.EXPORTS)
    assert "mhmr_body_consts" in header and "bodymodel.hip" in _lib.SOURCES
    assert re.search(r"#define\s+MHMR_VERSION\s+106\b", header) and _lib.VERSION == 106
    # the ctypes struct has the header's fields, in order
    body = re.search(r"typedef struct \{([^}]*)\} mhmr_body_consts;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") for n in re.sub(r"^\s*(const\s+)?(int|float)\s*\*?", "", decl.strip()).split(",") if n.strip()]
    assert names == [n for n, _ in _lib.BodyConsts._fields_]


def test_new_entry_points_check_their_arguments_before_any_launch():
    _lib.build()
    lib = _lib.lib()
    BAD_ARG, BAD_SHAPE = -1, -2
    c = _lib.BodyConsts()
    c.V, c.Vp, c.J, c.nc, c.K, c.E, c.L = 100, 128, 24, 10, 10 + 9 * 23, 0, 0
    call = lambda G=1: lib.mhmr_body_forward(ctypes.byref(c), *([None] * 4), G, *([None] * 7))
    assert call(0) == 0                                                  # nobody: nothing is launched, nothing is read
    assert call(1) == BAD_ARG and call(-1) == BAD_SHAPE
    for field, value in (("J", 65), ("Vp", 100), ("Vp", 64), ("K", 216), ("K", 2000), ("V", 0)):
        old = getattr(c, field)
        setattr(c, field, value)
        assert call(1) == BAD_SHAPE, (field, value)
        setattr(c, field, old)
    assert lib.mhmr_body_forward(None, *([None] * 4), 1, *([None] * 7)) == BAD_ARG
    assert lib.mhmr_sparse_regress(None, None, None, 5, 10, None, None, 0, None, None) == 0
    assert lib.mhmr_sparse_regress(None, None, None, 5, 10, None, None, 2, None, None) == BAD_ARG
    assert lib.mhmr_sparse_regress(None, None, None, 5, 0, None, None, 2, None, None) == BAD_SHAPE
    assert lib.mhmr_gt_targets(None, 45, 45, None, None, 1, 1, 16, 14, 1.0, 1, *([None] * 8)) == BAD_SHAPE     # centre joint outside
    assert lib.mhmr_gt_targets(None, 45, 15, None, None, 1, 0, 16, 14, 1.0, 1, *([None] * 8)) == BAD_SHAPE
    assert lib.mhmr_gt_targets(None, 45, 15, None, None, 1, 1, 16, 14, 1.0, 1, *([None] * 8)) == BAD_ARG
    assert lib.mhmr_rotvec_to_rotmat(None, 0, None, None) == 0 and lib.mhmr_rotvec_to_rotmat(None, 3, None, None) == BAD_ARG
    assert lib.mhmr_project_points(None, None, 0, 5, None, None) == 0 and lib.mhmr_project_points(None, None, 2, 5, None, None) == BAD_ARG


def test_synthetic_smpl_data_is_a_valid_model():
    for gender in ("male", "female"):
        d = synthetic.make_smpl_data(0, gender)
        assert d["v_template"].shape == (6890, 3) and d["shapedirs"].shape == (6890, 3, 10) and d["posedirs"].shape == (6890, 3, 207)
        assert d["weights"].shape == (6890, 24) and d["J_regressor"].shape == (24, 6890)
        assert np.abs(d["weights"].astype(np.float64).sum(1) - 1).max() < 1e-6 and d["weights"].min() >= 0
        assert np.abs(d["J_regressor"].astype(np.float64).sum(1) - 1).max() < 1e-5
        parents = d["kintree_table"][0].astype(np.int64)
        assert list(d["kintree_table"][1]) == list(range(24)) and parents[0] == 2 ** 32 - 1
        assert all(0 <= parents[i] < i for i in range(1, 24)) and list(parents[1:]) == constants.SMPL_PARENTS[1:]
        assert d["f"].min() >= 0 and d["f"].max() < 6890
        bm = BodyModel(d, "smpl")
        assert bm.num_vertices == 6890 and bm.num_out_joints == 45 and bm.faces.shape == (13776, 3) and bm.J_regressor.shape == (24, 6890)
    a, b = synthetic.make_smpl_data(0, "male"), synthetic.make_smpl_data(0, "female")
    assert not np.array_equal(a["v_template"], b["v_template"])
    assert all(np.array_equal(v, synthetic.make_smpl_data(0, "male")[k]) for k, v in a.items())          # seeded
    h = synthetic.make_h36m_regressor(0)
    assert h.shape == (17, 6890) and h.dtype == np.float32 and np.all((h != 0).sum(1) == 32)
    m = synthetic.make_smplx2smpl(0)
    assert m.shape == (6890, 10475) and np.abs(np.asarray(m.sum(1)).ravel() - 1).max() < 1e-6
    assert len(constants.SMPL_EXTRA_JOINT_VERTS) == 21 == len(set(constants.SMPL_EXTRA_JOINT_VERTS)) and max(constants.SMPL_EXTRA_JOINT_VERTS) < 6890
    assert constants.SMPL_EXTRA_JOINT_VERTS == go.SMPL_EXTRA and constants.H36M_TO_J14 == go.H36M_TO_J14


def test_existing_smplx_generator_is_byte_identical_to_the_parent_commit(smplx_data):
    """The benchmark draws from make_smplx_data: appending generators to synthetic.py must not move it.  The checksum was taken on the
    commit before the new generators were added."""
    h = hashlib.sha256()
    for k in sorted(smplx_data):
        a = np.ascontiguousarray(smplx_data[k])
        h.update(k.encode() + str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    want = open(os.path.join(ROOT, "tests", "golden", "synthetic_smplx_seed0.sha256")).read().strip()
    assert h.hexdigest() == want


def test_body_model_surface_and_no_cpu_path(smplx_data):
    bm = BodyModel(smplx_data, "smplx", num_betas=11)
    assert bm.num_vertices == 10475 and bm.num_out_joints == 127 and bm.faces.shape == (20908, 3) and bm.J_regressor.shape == (55, 10475)
    assert tuple(bm.expression.shape) == (1, 10) and float(bm.expression.abs().max()) == 0.0
    assert bm.basis_bytes == (21 + 486) * 3 * 10496 * 4
    with pytest.raises(_lib.MhmrError):
        bm(global_orient=torch.zeros(2, 3), betas=torch.zeros(2, 11))
    with pytest.raises(ValueError):
        BodyModel(smplx_data, "smpl")                                    # 55 joints are not an SMPL model
    bad = dict(synthetic.make_smpl_data(0, "male"))
    bad["kintree_table"] = bad["kintree_table"].copy()
    bad["kintree_table"][0, 3] = 7                                       # a parent behind its child
    with pytest.raises(ValueError):
        BodyModel(bad, "smpl")
    gt = GroundTruth(448, smplx_neutral=bm)
    assert gt.center_joint == 15 and abs(gt.focal_norm - 448 / (2 * np.tan(np.radians(30)))) < 1e-9
    with pytest.raises(_lib.MhmrError):
        gt.prepare(go.make_y("smplx", 0, 448, [1]))


def test_prepare_cases_meet_their_condition_on_the_fp64_oracle(smplx_data):
    """The GPU tests compare idx / scores / visibility EXACTLY; that is fair only where no centre sits within rounding of a cell border."""
    bodies = dict(smplx_neutral=go.OracleBody(smplx_data, "smplx", 11), smpl_male=go.OracleBody(synthetic.make_smpl_data(0, "male"), "smpl", 10),
                  smpl_female=go.OracleBody(synthetic.make_smpl_data(0, "female"), "smpl", 10))
    for name, case in go.PREPARE_CASES.items():
        gt = go.prepare_gt(go.make_y(img_size=go.IMG, **case), go.IMG, go.PATCH, True, "head", **bodies)
        away, inside = go.cell_condition(gt)
        assert away >= 1e-3 and inside, (name, away, inside)
        if "duplicate" in case:
            assert int((~gt["_visible"]).sum()) == 1 and float(gt["scores"].sum()) == int(gt["_visible"].sum())
    assert go.prepare_gt(go.make_y("smplx", 0, go.IMG, [0, 0]), go.IMG, go.PATCH, True, "head", **bodies) is None
