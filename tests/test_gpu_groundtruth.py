"""-m gpu: the ground-truth path on the device against the fp64 oracle of tests/gt_oracle.py.

Tolerances are not fixed in advance.  For every compared tensor the test evaluates the SAME oracle in fp32 on the CPU; the error of that
evaluation against fp64 is what an equally valid fp32 computation costs, and the kernel may be at most 4x worse (a different summation
order over ~500 terms).  Every figure is printed before it is asserted (run with -s to see them)."""
import numpy as np
import pytest
import torch

from multi_hmr_amd import BodyModel, Evaluator, GroundTruth, SparseRegressor, evaluate_dataset
import gt_oracle as go
import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def assets(smplx_data):
    data = {"smplx": (smplx_data, "smplx", 11), "smpl_male": (synthetic.make_smpl_data(0, "male"), "smpl", 10),
            "smpl_female": (synthetic.make_smpl_data(0, "female"), "smpl", 10)}
    out = {}
    for name, (d, kind, nb) in data.items():
        out[name] = dict(data=d, kind=kind, nb=nb, model=BodyModel(d, kind, num_betas=nb), o64=go.OracleBody(d, kind, nb, dtype=F64),
                         o32=go.OracleBody(d, kind, nb, dtype=F32))
    return out


def gate(name, got, ref64, ref32, unit="m"):
    """The 4x rule: |kernel - fp64| <= 4 |fp32 oracle - fp64| (maximum absolute errors)."""
    yard, err = go.max_err(ref32, ref64), go.max_err(got.cpu(), ref64)
    print(f"{name}: kernel {err:.3e} {unit}, fp32 oracle {yard:.3e} {unit}, gate {4 * yard:.3e} {unit}")
    assert tuple(got.shape) == tuple(ref64.shape), (name, tuple(got.shape), tuple(ref64.shape))
    assert err <= 4 * yard, (name, err, yard)
    return err, yard


def body_inputs(a, G, seed, zero_pose=False):
    g = torch.Generator().manual_seed(seed)
    J = a["model"].num_joints
    pose = torch.zeros(G, J, 3) if zero_pose else go.random_pose(g, G, J)
    coef = torch.randn(G, a["nb"], generator=g)
    if a["kind"] == "smplx":
        coef = torch.cat([coef, 0.5 * torch.randn(G, 10, generator=g)], 1)
    return pose, coef, go.random_transl(g, G)


def run_body(a, pose, coef, transl, K=None):
    G, nb = pose.shape[0], a["nb"]
    c = lambda t: None if t is None else t.to(DEV)
    if a["kind"] == "smplx":
        kw = dict(global_orient=pose[:, 0], body_pose=pose[:, 1:22].reshape(G, 63), jaw_pose=pose[:, 22], leye_pose=pose[:, 23], reye_pose=pose[:, 24],
                  left_hand_pose=pose[:, 25:40].reshape(G, 45), right_hand_pose=pose[:, 40:55].reshape(G, 45), betas=coef[:, :nb], expression=coef[:, nb:])
    else:
        kw = dict(global_orient=pose[:, 0], body_pose=pose[:, 1:].reshape(G, 69), betas=coef)
    return a["model"](transl=c(transl), K=c(K), **{k: v.to(DEV) for k, v in kw.items()})


@pytest.mark.parametrize("G", [1, 7, 8, 9, 33])
@pytest.mark.parametrize("name", ["smplx", "smpl_male", "smpl_female"])
def test_body_forward_within_4x_of_the_fp32_oracle(assets, name, G):
    """Global orientations of ~1.5 rad, translations of ~8 m: vertices at |x| up to ~11 m, where one fp32 ulp is 9.5e-7 m."""
    a = assets[name]
    pose, coef, transl = body_inputs(a, G, seed=100 * G + len(name))
    out = run_body(a, pose, coef, transl)
    v64, j64 = a["o64"](pose, coef, transl)
    v32, j32 = a["o32"](pose, coef, transl)
    assert out.v2d is None and out.j2d is None
    gate(f"{name} G={G} vertices", out.vertices, v64, v32)
    gate(f"{name} G={G} joints", out.joints, j64, j32)
    assert out.joints.shape[1] == {"smplx": 127, "smpl": 45}[a["kind"]]


def test_body_forward_projection_in_the_same_call(assets):
    a = assets["smplx"]
    pose, coef, transl = body_inputs(a, 5, seed=5)
    K = go.camera_K(448, 5, torch.Generator().manual_seed(6))
    out = run_body(a, pose, coef, transl, K)
    (v64, j64), (v32, j32) = a["o64"](pose, coef, transl), a["o32"](pose, coef, transl)
    gate("v2d", out.v2d, go.perspective_projection(v64, K.double()), go.perspective_projection(v32, K), "px")
    gate("j2d", out.j2d, go.perspective_projection(j64, K.double()), go.perspective_projection(j32, K), "px")


@pytest.mark.parametrize("name", ["smplx", "smpl_male"])
def test_body_forward_all_zero_pose_and_no_transl(assets, name):
    a = assets[name]
    pose, coef, transl = body_inputs(a, 3, seed=7, zero_pose=True)
    for tr in (transl, None):
        out = run_body(a, pose, coef, tr)
        (v64, j64), (v32, j32) = a["o64"](pose, coef, tr), a["o32"](pose, coef, tr)
        gate(f"{name} zero pose vertices", out.vertices, v64, v32)
        gate(f"{name} zero pose joints", out.joints, j64, j32)


def test_body_forward_vertex_count_off_the_tile_and_nobody(smplx_data):
    """1000 vertices (15 tiles of 64 + 40), picked vertices overridden through the data; then G = 0."""
    d = dict(synthetic.make_smplx_data(3, num_verts=1000, num_faces=2000))
    d["extra_joint_verts"] = np.arange(21) * 47 + 5
    a = dict(data=d, kind="smplx", nb=11, model=BodyModel(d, "smplx", num_betas=11),
             o64=go.OracleBody(d, "smplx", 11, dtype=F64, extra=list(d["extra_joint_verts"])),
             o32=go.OracleBody(d, "smplx", 11, dtype=F32, extra=list(d["extra_joint_verts"])))
    assert a["model"].num_vertices % 64 != 0
    pose, coef, transl = body_inputs(a, 9, seed=8)
    out = run_body(a, pose, coef, transl)
    (v64, j64), (v32, j32) = a["o64"](pose, coef, transl), a["o32"](pose, coef, transl)
    gate("V=1000 vertices", out.vertices, v64, v32)
    gate("V=1000 joints", out.joints, j64, j32)
    empty = run_body(a, pose[:0], coef[:0], transl[:0], go.camera_K(448, 0, torch.Generator().manual_seed(0)))
    assert tuple(empty.vertices.shape) == (0, 1000, 3) and tuple(empty.joints.shape) == (0, 127, 3)
    assert tuple(empty.v2d.shape) == (0, 1000, 2) and tuple(empty.j2d.shape) == (0, 127, 2) and empty.vertices.is_cuda


def dense_product(m, x, dtype, block=1024):
    """Dense matmul of a (possibly scipy-sparse) matrix with x [M, C, 3] in ``dtype``, densified a block of rows at a time."""
    dense = (lambda r0, r1: m[r0:r1].toarray()) if hasattr(m, "toarray") else (lambda r0, r1: np.asarray(m[r0:r1]))
    out = [torch.einsum("rc,mck->mrk", torch.from_numpy(dense(r0, min(r0 + block, m.shape[0])).astype(np.float32)).to(dtype), x.to(dtype))
           for r0 in range(0, m.shape[0], block)]
    return torch.cat(out, 1)


@pytest.mark.parametrize("which", ["smplx2smpl", "h36m"])
def test_sparse_regressor_within_4x_of_the_fp32_dense_product(which):
    m = synthetic.make_smplx2smpl(0) if which == "smplx2smpl" else synthetic.make_h36m_regressor(0)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, m.shape[1], 3, generator=g) * 0.4 + torch.randn(6, 1, 3, generator=g) * 3
    reg = SparseRegressor(m)
    got = reg(x.to(DEV))
    gate(which, got, dense_product(m, x, F64), dense_product(m, x, F32))
    again = reg(x.to(DEV))
    assert torch.equal(got, again)                                       # deterministic
    c = x[:, 0].clone()
    gate(which + " centred", reg(x.to(DEV), c.to(DEV)), dense_product(m, x - c[:, None], F64), dense_product(m, x - c[:, None], F32))


def test_sparse_regressor_row_without_entries_gives_zeros():
    m = synthetic.make_h36m_regressor(0).copy()
    m[5] = 0.0
    x = torch.randn(3, 6890, 3, generator=torch.Generator().manual_seed(4)) + 2.0
    got = SparseRegressor(m)(x.to(DEV)).cpu()
    assert float(got[:, 5].abs().max()) == 0.0 and float(got[:, 4].abs().min()) > 0.0
    assert tuple(SparseRegressor(m)(x[:0].to(DEV)).shape) == (0, 17, 3)


def check_prepare(name, y, assets, img=go.IMG, expect_dropped=0):
    o = lambda p: dict(smplx_neutral=assets["smplx"][p], smpl_male=assets["smpl_male"][p], smpl_female=assets["smpl_female"][p])
    ref = go.prepare_gt(y, img, go.PATCH, True, "head", dtype=F64, **o("o64"))
    yard = go.prepare_gt(y, img, go.PATCH, True, "head", dtype=F32, **o("o32"))
    away, inside = go.cell_condition(ref, img)
    print(f"{name}: nearest cell border {away:.4f} cells away, all centres inside: {inside}")
    assert away >= 1e-3 and inside                                       # the condition under which idx / scores / visibility are compared exactly
    gt_builder = GroundTruth(img, patch_size=go.PATCH, nearness=True, person_center="head", **o("model"))
    got = gt_builder.prepare({k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in y.items()})
    assert set(got) == {k for k in ref if not k.startswith("_")}, set(got) ^ set(ref)
    n_valid, n_vis = int(ref["_visible"].numel()), int(ref["_visible"].sum())
    assert n_valid - n_vis == expect_dropped
    assert len(got["idx"]) == 4
    for a, b in zip(got["idx"], ref["idx"]):
        assert a.is_cuda and torch.equal(a.cpu().long(), b.long())
    assert torch.equal(got["scores"].cpu(), ref["scores"]) and float(got["scores"].sum()) == n_vis
    assert torch.equal(got["K"].cpu(), y["K"])
    for k in ref:
        if k.startswith("_") or k in ("idx", "scores", "K"):
            continue
        assert got[k].shape[0] == n_vis, (k, got[k].shape)               # occluded humans are gone from every key
        gate(f"{name} {k}", got[k], ref[k], yard[k], "px" if k in ("j2d", "v2d", "loc") else ("cell" if k == "offset" else ""))
    return got, ref


def test_prepare_bedlam_family_padded_rows_empty_image_and_two_humans_in_one_cell(assets):
    case = go.PREPARE_CASES["bedlam"]
    y = go.make_y(img_size=go.IMG, **case)
    got, ref = check_prepare("bedlam", y, assets, expect_dropped=1)
    assert {"rotvec", "rotmat", "shape"} <= set(got) and tuple(got["rotvec"].shape[1:]) == (53, 3) and tuple(got["rotmat"].shape[1:]) == (53, 3, 3)
    assert got["v3d"].shape[1:] == (10475, 3) and got["j3d"].shape[1:] == (127, 3) and not bool((got["idx"][0] == 1).any())
    # the duplicate (image 3, human 3) shares its cell with human 1: the first stays, the cell holds a single 1
    b, cy, cx = 3, int(ref["idx"][1][-2]), int(ref["idx"][2][-2])
    assert int((got["idx"][0] == 3).sum()) == 3 and float(got["scores"][b, cy, cx]) == 1.0 and float(got["scores"][b].sum()) == 3.0


def test_prepare_3dpw_family_with_the_female_override(assets):
    for name, dropped in (("3dpw", 1), ("3dpw_one_image", 0)):
        y = go.make_y(img_size=go.IMG, **go.PREPARE_CASES[name])
        got, ref = check_prepare(name, y, assets, expect_dropped=dropped)
        assert got["v3d"].shape[1:] == (6890, 3) and got["j3d"].shape[1:] == (45, 3) and "rotvec" not in got
    # the override matters: with every annotation male the meshes differ
    y_m = go.make_y(img_size=go.IMG, **{**go.PREPARE_CASES["3dpw_one_image"], "female": ()})
    male = GroundTruth(go.IMG, smpl_male=assets["smpl_male"]["model"], smpl_female=assets["smpl_female"]["model"]).prepare({k: v.to(DEV) for k, v in y_m.items()})
    assert float((male["v3d"][0] - got["v3d"][0]).abs().max()) > 1e-2 and torch.equal(male["v3d"][1], got["v3d"][1])


def test_prepare_ehf_family_and_a_batch_without_humans(assets):
    a = assets["smplx"]
    pose, coef, transl = body_inputs(a, 1, seed=21)
    transl = torch.tensor([[0.4, -0.3, 7.5]])
    verts = a["o32"](pose, coef, transl)[0]                              # what the dataset stores: fp32 vertices
    g = torch.Generator().manual_seed(22)
    y = {"K": go.camera_K(go.IMG, 1, g), "valid_humans": torch.ones(1, 1), "smplx_vertices": verts.reshape(1, 1, -1, 3)}
    got, _ = check_prepare("ehf", y, assets)
    assert got["j3d"].shape[1:] == (55, 3) and got["v3d"].shape[1:] == (10475, 3) and torch.equal(got["v3d"].cpu(), verts)
    empty = go.make_y("smplx", 0, go.IMG, [0, 0])
    builder = GroundTruth(go.IMG, smplx_neutral=a["model"])
    assert builder.prepare({k: v.to(DEV) for k, v in empty.items()}) is None
    y0 = go.make_y("smplx", 1, go.IMG, [2])
    y0["valid_humans"] = torch.zeros(1, 2)                               # annotations present, nobody valid
    assert builder.prepare({k: v.to(DEV) for k, v in y0.items()}) is None


def test_evaluator_3dpw_metrics_match_the_fp64_restatement(assets):
    """SMPL ground truth, SMPL-X predictions mapped by smplx2smpl, H36M joints: pve / pa_pve / mpjpe / pa_mpjpe against train.py:372-429
    restated in fp64, with the relative bounds tests/test_evaluate.py uses for the same kernel (1e-5 unaligned, 1e-4 aligned)."""
    s2s, h36m = synthetic.make_smplx2smpl(0), synthetic.make_h36m_regressor(0)
    y = go.make_y("smpl", 31, go.IMG, [3], female=((0, 2),))
    gt = GroundTruth(go.IMG, smpl_male=assets["smpl_male"]["model"], smpl_female=assets["smpl_female"]["model"]).prepare({k: v.to(DEV) for k, v in y.items()})
    M = gt["v3d"].shape[0]
    assert M == 3
    a = assets["smplx"]
    g = torch.Generator().manual_seed(32)
    pose, coef, _ = body_inputs(a, M, seed=33)
    pred = run_body(a, pose, coef, gt["transl_pelvis"].cpu() + 0.05 * torch.randn(M, 3, generator=g))
    humans = [dict(v3d=pred.vertices[i], j3d=pred.joints[i], transl_pelvis=pred.joints[i, :1],
                   j2d=torch.cat([gt["j2d"][i] + 2.0 * torch.randn(45, 2, generator=g).to(DEV), torch.zeros(82, 2, device=DEV)])) for i in (2, 0, 1)]
    ev = Evaluator(smplx2smpl=s2s, h36m_regressor=h36m)
    ev.update(humans, gt)
    s = ev.summary()
    assert s["matched"] == M and s["count"] == M and s["recall"] == 100.0
    ref = [go.metrics_3dpw(pred.vertices[i].cpu(), pred.joints[i, 0].cpu(), gt["v3d"][i].cpu(), gt["transl_pelvis"][i].cpu(), s2s, h36m) for i in range(M)]
    for k, rel in (("pve", 1e-5), ("pa_pve", 1e-4), ("mpjpe", 1e-5), ("pa_mpjpe", 1e-4)):
        want = float(np.mean([r[k] for r in ref]))
        print(f"{k}: evaluator {s[k]:.6f} mm, fp64 {want:.6f} mm, relative {abs(s[k] - want) / want:.2e}")
        assert abs(s[k] - want) <= rel * max(want, 1.0), (k, s[k], want)
    # without the regressors an SMPL ground truth cannot be compared with an SMPL-X prediction
    from multi_hmr_amd import _lib
    with pytest.raises(_lib.MhmrError):
        Evaluator().update(humans, gt)


def test_evaluator_exact_similarity_gives_pa_error_at_the_fp32_floor(assets):
    """pred = s R gt + t on the SMPL topology (no mapping): the aligned errors vanish up to fp32 rounding.  Both meshes are stored in fp32
    at their absolute position ~8 m from the camera (half an ulp of the coordinate each), and the kernel applies the fitted transform in
    fp32 (a few more): the bound is 4 ulp of the largest coordinate, in mm -- about 5e-3 mm at 11 m."""
    from oracle import roma_ref
    h36m = synthetic.make_h36m_regressor(0)
    y = go.make_y("smpl", 41, go.IMG, [2])
    gt = GroundTruth(go.IMG, smpl_male=assets["smpl_male"]["model"]).prepare({k: v.to(DEV) for k, v in y.items()})
    g = torch.Generator().manual_seed(42)
    humans = []
    for i in range(2):
        R = roma_ref.rotvec_to_rotmat(torch.randn(3, generator=g, dtype=F64))
        s, t = 1.3, torch.randn(3, generator=g, dtype=F64) * 0.1
        c = gt["transl_pelvis"][i].cpu().double()
        v = (s * (gt["v3d"][i].cpu().double() - c) @ R.T + t + c).float().to(DEV)
        humans.append(dict(v3d=v, j3d=gt["j3d"][i], transl_pelvis=gt["transl_pelvis"][i], j2d=gt["j2d"][i]))
    ev = Evaluator(h36m_regressor=h36m)
    ev.update(humans, gt)
    s = ev.summary()
    print(f"exact similarity: pve {s['pve']:.3f} mm, pa_pve {s['pa_pve']:.3e} mm, mpjpe {s['mpjpe']:.3f} mm, pa_mpjpe {s['pa_mpjpe']:.3e} mm")
    floor_mm = 4 * float(torch.finfo(torch.float32).eps) * float(gt["v3d"].abs().max()) * 1000
    print(f"fp32 floor (4 ulp of the largest coordinate): {floor_mm:.3e} mm")
    assert s["matched"] == 2 and s["pve"] > 10.0 and s["pa_pve"] < floor_mm and s["pa_mpjpe"] < floor_mm


def test_evaluate_dataset_with_gt_idx_runs_the_small_model_end_to_end(smplx_data, mean_params):
    """The ViT-S model of smoke() over two batches: the ground truth's own idx through the is_training forward, matching, metrics.
    The seeded checkpoint predicts people 2 - 3 m away whatever the image shows, so the annotated humans stand at that distance: the
    2D matching (by joint distance, then box overlap) is meaningful only between figures of comparable size."""
    from multi_hmr_amd import Model
    S, name = 224, "dinov2_vits14"
    sd = synthetic.make_state_dict(name, S, seed=42, depth_override=4, mean_params=mean_params)
    model = Model(backbone=name, img_size=S, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=4, precision="f16")
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    builder = GroundTruth(S, patch_size=14, smplx_neutral=BodyModel(smplx_data, "smplx", num_betas=11))
    g = torch.Generator().manual_seed(0)
    batches = [(torch.randn(2, 3, S, S, generator=g), go.make_y("smplx", 51 + i, S, counts, depth=2.6)) for i, counts in enumerate(([2, 1], [1, 2]))]
    s = evaluate_dataset(model, batches, builder, det_thresh=0.3, nms_kernel_size=3, use_gt_idx=True)
    print(s)
    assert s["count"] == 6 and s["matched"] == 6 and s["recall"] == 100 and s["precision"] == 100
    assert all(np.isfinite(s[k]) and s[k] > 0 for k in ("pve", "pa_pve", "mpjpe", "pa_mpjpe"))
