"""The 3D export on the GPU: ``scene.pack_meshes`` (csrc/scene.hip, mhmr_scene_pack) against the numpy oracle tests/scene_oracle.py,
its strided and repeated calls, ``export_batch`` against one call per image, and the demo's ``--save_mesh`` / ``--distance`` end to
end on the ViT-S 672 model of tests/test_gpu_pipeline.py.

Bounds of the comparison (derived, not measured): positions and bounds are fp64 expressions of fp32 inputs rounded once, operation
for operation the oracle's, hence bit-equal.  A normal differs from the oracle's only through the last bits of fp64 ``acos`` /
``sqrt``, which can move the one fp32 rounding of a component (a value <= 1) by at most one unit in its last place, 2^-23 absolute
-- provided the weighted sum does not cancel, which the test asserts on its own inputs (|sum| / sum of angles >= 0.01) first."""
import glob
import io
import os

import numpy as np
import pytest
import torch

import render_oracle as ro
import scene_oracle as so
import synthetic

PIL = pytest.importorskip("PIL")
from PIL import Image, ImageFont  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "demo_672_s.npz"))
EXAMPLES = os.path.join(os.path.dirname(__file__), "golden", "example_data")
NORMAL_TOL = 2.0 ** -23
MIN_SURVIVE = 0.01


def seeded_transform(seed):
    """[R | t] float32 [3, 4]: a seeded rotation (QR of a normal matrix, determinant +1) and a translation of a few metres."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return np.concatenate([Q, rng.uniform(-3, 3, size=(3, 1))], 1).astype(np.float32)


def icosphere_inputs():
    """Five icospheres of subdivision 4 (2562 vertices), radius 0.5, apart, with seeded per-vertex noise."""
    v, f = ro.icosphere(4)
    rng = np.random.default_rng(11)
    verts = np.stack([0.5 * v + 0.002 * rng.standard_normal(v.shape) + np.array([p - 2.0, 0.1 * p, 3.0 + 0.5 * p])
                      for p in range(5)]).astype(np.float32)
    return verts, f


def smplx_inputs():
    """The synthetic SMPL-X stand-in: its template and three seeded perturbations, on its random faces."""
    data = synthetic.make_smplx_data(seed=0)
    vt = np.asarray(data["v_template"], np.float64)
    rng = np.random.default_rng(23)
    verts = np.stack([vt] + [vt + 0.003 * rng.standard_normal(vt.shape) + rng.uniform(-1, 1, size=3) for _ in range(3)]).astype(np.float32)
    return verts, np.asarray(data["f"], np.int32)


@pytest.mark.parametrize("inputs", [icosphere_inputs, smplx_inputs], ids=["icospheres", "smplx_stand_in"])
@pytest.mark.parametrize("transform", [None, 7], ids=["default", "seeded_Rt"])
def test_pack_meshes_against_the_numpy_oracle(inputs, transform):
    from multi_hmr_amd import scene
    verts, faces = inputs()
    M = None if transform is None else seeded_transform(transform)
    want, want_bounds, none, survive = so.pack(verts, faces, M)
    if inputs is smplx_inputs:
        P3 = verts[0][faces].astype(np.float64)
        degenerate = int((ro._norm(ro._cross(P3[:, 1] - P3[:, 0], P3[:, 2] - P3[:, 0])) == 0).sum())
        print("degenerate faces", degenerate, "vertices without a normal", none.sum(1).tolist())
        assert degenerate == 5 and none.sum(1).tolist() == [25] * 4
    else:
        assert not none.any()
    print("min |sum| / sum of angles", float(survive.min()))
    assert survive.min() >= MIN_SURVIVE                                    # an input that cancels fails here, loudly

    packed, bounds = scene.pack_meshes(torch.from_numpy(verts).cuda(), faces, M)
    assert packed.shape == want.shape and packed.dtype == torch.float32 and bounds.shape == want_bounds.shape
    got, got_bounds = packed.cpu().numpy(), bounds.cpu().numpy()
    assert got[:, 0].tobytes() == want[:, 0].tobytes()                     # positions: bit-equal
    assert got_bounds.tobytes() == np.stack([got[:, 0].min(1), got[:, 0].max(1)], 1).tobytes()
    assert got_bounds.tobytes() == want_bounds.tobytes()
    err = np.abs(got[:, 1].astype(np.float64) - want[:, 1].astype(np.float64))
    print("max normal error", float(err.max()), "in units of 2^-23:", float(err.max() / NORMAL_TOL))
    assert err.max() <= NORMAL_TOL                                         # every component of every vertex
    assert np.array_equal(got[:, 1][none], np.broadcast_to(np.float32([0, 0, 1]), (int(none.sum()), 3)))
    length = np.linalg.norm(got[:, 1].astype(np.float64), axis=2)
    assert np.abs(length - 1).max() <= 4 * NORMAL_TOL                      # unit normals, as glTF wants them


def test_strided_slice_repeat_and_empty_calls():
    from multi_hmr_amd import scene
    verts, faces = icosphere_inputs()
    rng = np.random.default_rng(3)
    big = torch.from_numpy((np.concatenate([verts, verts])[:, :, :] + rng.standard_normal((10, 1, 3))).astype(np.float32)).cuda()
    part = big[3:7]
    assert part.storage_offset() > 0 and part.data_ptr() == big[3].data_ptr()  # read in place
    a, ab = scene.pack_meshes(part, faces)
    b, bb = scene.pack_meshes(part.clone().contiguous(), faces)
    assert torch.equal(a, b) and torch.equal(ab, bb)
    wide = torch.zeros(10, verts.shape[1] + 5, 3, device="cuda")             # a person stride larger than 3 V
    wide[:, :verts.shape[1]] = big
    c, cb = scene.pack_meshes(wide[3:7, :verts.shape[1]], faces)
    assert wide[3:7, :verts.shape[1]].stride(0) > 3 * verts.shape[1] and torch.equal(a, c) and torch.equal(ab, cb)
    a2, ab2 = scene.pack_meshes(part, faces)
    assert torch.equal(a, a2) and torch.equal(ab, ab2) and a.data_ptr() != a2.data_ptr()
    one, oneb = scene.pack_meshes(big[5:6], faces)
    assert torch.equal(one, a[2:3]) and torch.equal(oneb, ab[2:3])
    e, eb = scene.pack_meshes(big[:0], faces)
    assert e.shape == (0, 2, verts.shape[1], 3) and eb.shape == (0, 2, 3)
    with pytest.raises(ValueError):
        scene.pack_meshes(big.cpu(), faces)


def test_export_batch_equals_one_pack_per_image(tmp_path):
    from multi_hmr_amd import scene
    from multi_hmr_amd.render import PALETTE
    verts, faces = icosphere_inputs()
    dev = torch.from_numpy(verts).cuda()
    index = torch.tensor([0, 0, 2, 2, 2], dtype=torch.int32, device="cuda")   # image 1 is empty
    rng = np.random.default_rng(9)
    photos = [Image.fromarray(rng.integers(0, 256, size=(48, 64, 3)).astype(np.uint8)) for _ in range(3)]
    K = np.stack([np.array([[70.0, 0, 32], [0, 70.0, 24], [0, 0, 1]], np.float32)] * 3)
    paths = [str(tmp_path / f"img{b}.glb") for b in range(3)]
    assert scene.export_batch(dev, index, faces, paths, images=photos, K=K) == paths
    for b, (p0, p1) in enumerate([(0, 2), (2, 2), (2, 5)]):
        back = scene.read_glb(paths[b])
        persons = [k for k in back["nodes"] if k.startswith("person_")]
        assert persons == [f"person_{j}" for j in range(p1 - p0)] and {"image", "camera"} <= set(back["nodes"])
        if p1 == p0:
            continue
        block, bounds = (t.cpu().numpy() for t in scene.pack_meshes(dev[p0:p1], faces))
        assert block.tobytes() in open(paths[b], "rb").read()              # the image's persons: one byte range, as packed alone
        for j in range(p1 - p0):
            node = back["nodes"][f"person_{j}"]
            assert node["attributes"]["POSITION"].tobytes() == block[j, 0].tobytes()
            assert node["attributes"]["NORMAL"].tobytes() == block[j, 1].tobytes()
            acc = back["json"]["accessors"][back["json"]["meshes"][j]["primitives"][0]["attributes"]["POSITION"]]
            assert np.array_equal(np.float32(acc["min"]), bounds[j, 0]) and np.array_equal(np.float32(acc["max"]), bounds[j, 1])
            assert node["material"]["pbrMetallicRoughness"]["baseColorFactor"] == [float(c) for c in PALETTE[j]] + [1.0]
    bare = scene.export_batch(dev, index, faces, [str(tmp_path / f"bare{b}.glb") for b in range(3)], normals=False)
    assert scene.read_glb(bare[1])["nodes"] == {}                           # no persons, no photograph: an empty scene
    assert list(scene.read_glb(bare[2])["nodes"]["person_0"]["attributes"]) == ["POSITION"]
    with pytest.raises(ValueError):
        scene.export_batch(dev, torch.tensor([0, 2, 1, 2, 2]), faces, paths)


# ----------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def model(smplx_data, mean_params):
    """The ViT-S 672 model of tests/test_gpu_pipeline.py."""
    from multi_hmr_amd import Model
    sd = synthetic.make_state_dict("dinov2_vits14", 672, seed=31)
    sd["mlp_classif.2.bias"] = torch.from_numpy(GOLD["classif_bias"])
    m = Model(backbone="dinov2_vits14", img_size=672, smplx_data=smplx_data, mean_params=mean_params, precision="f16")
    m.load_state_dict(sd, strict=True)
    return m.to("cuda:0").eval()


def test_demo_save_mesh_and_distance_end_to_end(model, tmp_path, monkeypatch):
    from multi_hmr_amd import demo, scene
    from multi_hmr_amd.pipeline import predict_images
    from multi_hmr_amd.render import PALETTE
    monkeypatch.setattr(demo, "load_model", lambda name, *a, **k: model)
    srcs = sorted(glob.glob(os.path.join(EXAMPLES, "*.jpg")))
    kw = dict(det_thresh=float(GOLD["det_thresh"]), nms_kernel_size=int(GOLD["nms_kernel_size"]))
    base = ["--model_name", "synthetic_672_S", "--img_folder", EXAMPLES, "--det_thresh", str(kw["det_thresh"]),
            "--nms_kernel_size", str(kw["nms_kernel_size"])]
    extra = {"b1": [], "b4": ["--batch_size", "4"]}
    plain = {r: demo.main(base + ["--out_folder", str(tmp_path / ("plain_" + r))] + extra[r]) for r in extra}
    full = {r: demo.main(base + ["--out_folder", str(tmp_path / r), "--save_mesh", "1", "--distance", "1"] + extra[r]) for r in extra}
    stems = [os.path.basename(p) for p in plain["b1"]]
    assert len(stems) == 7 and [os.path.basename(p) for p in plain["b4"]] == stems
    assert [os.path.basename(p) for p in full["b1"]] == [os.path.basename(p) for p in full["b4"]]
    assert [os.path.basename(p) for p in full["b1"]] == [s + ext for s in stems for ext in ("", ".npy", ".glb")]
    assert sorted(os.listdir(tmp_path / "b1")) == sorted(os.listdir(tmp_path / "b4")) and all(os.path.isfile(p) for p in full["b4"])

    # the forwards the two runs made: one image at a time, and four per batch
    forwards = {"b1": [], "b4": [(r.humans, r.K_full) for r in predict_images(model, srcs, batch_size=4, fov=60, **kw)]}
    for src in srcs:
        x, img = demo.open_image(src, model.img_size)
        K = demo.get_camera_parameters(model.img_size, fov=60)
        humans = demo.forward_model(model, x, K, **kw)
        ratio = max(img.size) / x.shape[-1]
        K[0, 0, 2], K[0, 1, 2] = img.size[0] / 2.0, img.size[1] / 2.0
        K[0, [0, 1], [0, 1]] = ratio * K[0, [0, 1], [0, 1]]
        forwards["b1"].append((humans, K))

    font = ImageFont.load_default()
    faces = np.asarray(model.smpl_layer["neutral_10"].bm_x.faces)
    V = int(model.smpl_layer["neutral_10"].bm_x.num_vertices)
    counts = {r: [] for r in extra}
    for run in extra:
        folder = tmp_path / run
        for src, stem, (humans, K) in zip(srcs, stems, forwards[run]):
            img = Image.open(src).convert("RGB")
            W, H = img.size
            Kf = K[0].cpu().numpy().astype(np.float64)
            n = len(humans)
            counts[run].append(n)
            v3d = torch.stack([h["v3d"] for h in humans]).cpu().numpy() if n else np.zeros((0, V, 3), np.float32)
            npy = np.load(folder / (stem + ".npy"))
            assert npy.dtype == np.float32 and npy.shape == v3d.shape and npy.tobytes() == v3d.tobytes()
            back = scene.read_glb(str(folder / (stem + ".glb")))
            assert [k for k in back["nodes"] if k.startswith("person_")] == [f"person_{j}" for j in range(n)]
            assert {"image", "camera"} <= set(back["nodes"])
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(back["images"][0])).convert("RGB")), np.asarray(img))
            for j in range(n):
                node = back["nodes"][f"person_{j}"]
                want = (v3d[j] * np.float32([-1, -1, 1])).astype(np.float32)
                assert node["attributes"]["POSITION"].tobytes() == want.tobytes()
                assert np.array_equal(node["indices"].reshape(-1, 3), faces)
                length = np.linalg.norm(node["attributes"]["NORMAL"].astype(np.float64), axis=1)
                assert np.abs(length - 1).max() <= 4 * NORMAL_TOL
                assert node["material"]["pbrMetallicRoughness"]["baseColorFactor"] == [float(c) for c in PALETTE[j % len(PALETTE)]] + [1.0]
            # the picture, [input | overlay]: only the label boxes of the overlay differ from the run without --distance
            a = np.asarray(Image.open(tmp_path / ("plain_" + run) / stem).convert("RGB"))
            b = np.asarray(Image.open(folder / stem).convert("RGB"))
            assert a.shape == b.shape == (H, 2 * W, 3)
            labels = scene.distance_labels(humans, [PALETTE[j % len(PALETTE)] for j in range(n)], K=K)
            allowed = np.zeros((H, W), bool)
            for j, lab in enumerate(labels):
                x0, y0, x1, y1 = font.getbbox(lab["text"])
                ax, ay = lab["anchor"]
                allowed[max(int(np.floor(ay + y0)), 0):max(int(np.ceil(ay + y1)) + 1, 0),
                        max(int(np.floor(ax + x0)), 0):max(int(np.ceil(ax + x1)) + 1, 0)] = True
                v = v3d[j].astype(np.float64)
                u2 = Kf[0, 0] * v[:, 0] / v[:, 2] + Kf[0, 2]
                v2 = Kf[1, 1] * v[:, 1] / v[:, 2] + Kf[1, 2]
                print(stem, run, j, lab["text"], "anchor", lab["anchor"], "vertex box", u2.min(), v2.min(), u2.max(), v2.max())
                assert u2.min() <= ax <= u2.max() and v2.min() <= ay <= v2.max()
                t = humans[j]["transl_pelvis"].cpu().numpy().reshape(3)
                assert lab["text"] == f"{np.sqrt(t[0] ** 2 + t[2] ** 2):.2f}m"
            changed = np.any(a != b, axis=2)
            assert not changed[:, :W].any()                                 # the input panel
            assert not (changed[:, W:] & ~allowed).any()
            if any(0 <= lab["anchor"][0] < W - 40 and 0 <= lab["anchor"][1] < H - 16 for lab in labels):
                assert changed[:, W:].any()
    print("persons per image:", counts)
    assert sum(counts["b1"]) > 0 and sum(counts["b4"]) > 0
