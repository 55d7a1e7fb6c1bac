"""-m gpu: contacts between persons (csrc/contact.hip, include/mhmr.h mhmr_contact, multi_hmr_amd/contact.py) against the fp64 numpy
restatement of the contract (tests/contact_oracle.py), through the C entry (every output buffer followed by a guard row that must
survive) and through ``contacts``.  The comparison rules -- what must be equal, what is gated, the guard set and its cap -- are
``contact_oracle.compare``'s.  Spheres have radius 0.5; the first is centred at (0.3, -0.2, 6.0)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import contact_oracle as co
import synthetic
from multi_hmr_amd import Model, _lib, contact, contacts, predict_images
from multi_hmr_amd.pipeline import CONTACT_KEYS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C0 = np.array([0.3, -0.2, 6.0])
FIELDS = contact.FIELDS
PATTERN = 0xA5
WORST = {}                     # scene -> the worst errors compare() found; printed by the last test of the file


def spheres(level, offset, faces=None):
    v, f = co.icosphere(level)
    return np.stack([0.5 * v + C0, 0.5 * v + C0 + offset]).astype(np.float32), (f if faces is None else faces)


@functools.lru_cache(maxsize=None)
def scene(name):
    """verts [P, V, 3] fp32, image_index, faces, max_dist, tau of the named scene."""
    if name in ("overlap2", "overlap3"):
        v, f = spheres(int(name[-1]), (0.6, 0.1, 0.2))
        return v, (0, 0), f, 0.10, 0.01
    if name == "deep":
        v, f = spheres(3, (0.2, 0.05, 0.1))
        return v, (0, 0), f, 0.10, 0.01
    if name in ("near", "near_short"):
        v, f = spheres(3, (1.03, 0, 0))
        return v, (0, 0), f, (0.10 if name == "near" else 0.02), 0.01
    if name == "nested":
        v, f = co.icosphere(3)
        return np.stack([0.2 * v + C0 + (0.05, 0.02, 0.03), 0.5 * v + C0]).astype(np.float32), (4, 4), f, 0.10, 0.01
    if name == "three":
        v, f = co.icosphere(2)
        return np.stack([0.5 * v + C0, 0.5 * v + C0 + (0.6, 0.1, 0.2), 0.5 * v + C0 + (-0.55, 0.3, -0.1)]).astype(np.float32), (1, 1, 1), f, 0.10, 0.01
    if name == "two_images":
        v, f = spheres(2, (0.6, 0.1, 0.2))
        return v, (0, 1), f, 0.10, 0.01
    if name == "torus":
        # one vertex and face array for both shapes: person 0 is the torus (the box's vertices collapsed onto its vertex 0, so the box's
        # faces are degenerate and skipped), person 1 the thin box through the hole (the torus's vertices collapsed onto the hole's
        # centre: a query point inside the torus's box and outside the torus)
        vt, ft = co.torus(24, 12)
        vb, fb = co.box()
        vb = vb * (0.1, 0.1, 1.0)
        p0 = np.concatenate([vt, np.repeat(vt[:1], 8, 0)]) + C0
        p1 = np.concatenate([np.zeros_like(vt), vb]) + C0
        return np.stack([p0, p1]).astype(np.float32), (0, 0), np.concatenate([ft, fb + len(vt)]).astype(np.int32), 0.40, 0.01
    if name == "open":
        v, f = co.open_sphere(3)
        return spheres(3, (0.6, 0.1, -0.2), f)[0], (0, 0), f, 0.10, 0.01
    if name == "inverted":
        v, f = spheres(3, (0.6, 0.1, 0.2))
        return v, (0, 0), co.inverted(f), 0.10, 0.01
    if name == "degenerate":
        v, f = spheres(3, (0.6, 0.1, 0.2))
        return v, (0, 0), co.with_degenerate(f), 0.10, 0.01
    if name == "boxes":                                                  # V = 8: less than one wave
        v, f = co.box()
        return np.stack([v + C0, v + C0 + (0.3, 0.2, 0.1)]).astype(np.float32), (0, 0), f, 0.10, 0.01
    if name in ("tile", "tile_plus_one"):                                # F == the face tile and one more, the LAST face a real one
        v, f = co.icosphere(1)
        n = contact.FACE_TILE + (name == "tile_plus_one")
        fd = co.with_degenerate(f[:-1], n - len(f))
        f = np.concatenate([fd, f[-1:]]).astype(np.int32)
        assert len(f) == n
        return np.stack([0.5 * v + C0, 0.5 * v + C0 + (0.55, -0.2, 0.15)]).astype(np.float32), (0, 0), f, 0.10, 0.01   # the last face is two vertices' nearest
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    v, idx, f, md, tau = scene(name)
    return co.contacts(v, idx, f, md, tau)


def run_abi(verts, idx, faces, max_dist, tau, want=FIELDS, pad=0):
    """mhmr_contact itself: every requested output over-allocated by a guard row of PATTERN bytes (asserted intact), the others NULL.
    pad > 0: the persons' rows lie 3 V + pad floats apart, NaN in between."""
    v = np.ascontiguousarray(verts, np.float32)
    P, V = v.shape[:2]
    stride = 3 * V + pad
    buf = np.full((max(P, 1), stride), np.nan, np.float32)
    buf[:P, :3 * V] = v.reshape(P, -1)
    vd = torch.from_numpy(buf).to(DEV)
    idxd = torch.as_tensor(np.asarray(idx, np.int32).reshape(-1)).to(DEV)
    fd = torch.as_tensor(np.ascontiguousarray(faces, np.int32)).to(DEV)
    L = _lib.lib()
    assert L.mhmr_contact_check_faces(np.ascontiguousarray(faces, np.int32).ctypes.data, len(faces), V) == 0
    nbytes = _lib.workspace_bytes("mhmr_contact_workspace_bytes", P, V)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    d = _lib.ContactDesc()
    d.P, d.V, d.F, d.verts, d.vstride = P, V, len(faces), vd.data_ptr(), stride
    d.image_index, d.faces, d.max_dist, d.tau = idxd.data_ptr(), fd.data_ptr(), max_dist, tau
    d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    bufs = {}
    for n in want:
        shape, dtype = contact._SHAPES[n][0](P, V), contact._SHAPES[n][1]
        rows = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        guard = max(64, rows // max(P, 1))
        bufs[n] = (torch.full((rows + guard,), PATTERN, dtype=torch.uint8, device=DEV), rows, shape, dtype)
        setattr(d, n, bufs[n][0].data_ptr())
    _lib.check(L.mhmr_contact(C.byref(d), torch.cuda.current_stream().cuda_stream), "mhmr_contact")
    torch.cuda.synchronize()
    out = {}
    for n, (b, rows, shape, dtype) in bufs.items():
        assert bool((b[rows:] == PATTERN).all()), f"{n}: the guard row was written"
        out[n] = b[:rows].view(dtype).reshape(shape).cpu().numpy()
    return out


def run_py(verts, idx, faces, max_dist, tau, **kw):
    c = contacts(torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(DEV), idx, faces, max_dist=max_dist, tau=tau, **kw)
    return {n: (None if getattr(c, n) is None else getattr(c, n).cpu().numpy()) for n in FIELDS}


def same_bits(x, y):
    return all(np.array_equal(x[n].view(np.uint8), y[n].view(np.uint8)) for n in FIELDS)


def check(name):
    """The scene through the C entry and through ``contacts``: the same bits, and compare()'s rules against the fp64 oracle."""
    v, idx, f, md, tau = scene(name)
    ref = reference(name)
    co.guard_set(ref, tau)                                               # the cap, from the oracle alone, before looking at the kernel
    got, py = run_abi(v, idx, f, md, tau), run_py(v, list(idx), f, md, tau)
    assert same_bits(got, py)
    WORST[name] = co.compare(got, ref, v, f, md, tau)
    return got, ref


# ------------------------------------------------------------------------------------------------------------------ scenes
@pytest.mark.parametrize("name,inside", [("overlap2", 27), ("overlap3", 113)])
def test_overlap(name, inside):
    got, ref = check(name)
    assert ref["inside_count"].tolist() == [inside, inside] == got["inside_count"].tolist()
    assert got["pair_inside"].tolist() == [[0, inside], [inside, 0]] and got["penetration_depth"].min() > 0.3


def test_deep_overlap():
    got, ref = check("deep")
    assert got["inside_count"].min() > 200 and (got["pair_distance"][[0, 1], [1, 0]] < -0.2).all()


def test_near_not_touching():
    got, ref = check("near")
    assert got["inside_count"].tolist() == [0, 0] and (np.isfinite(got["sdf"]).sum(1) == 19).all()
    assert abs(got["sdf"].min() - 0.03) < 1e-6 and np.allclose(got["pair_distance"][[0, 1], [1, 0]], 0.03, atol=1e-6)
    assert got["contact_count"].tolist() == [0, 0] and (got["penetration_depth"] == 0).all()
    got, ref = check("near_short")                                      # max_dist = 0.02: the boxes still make the pair evaluated
    assert ref["detail"]["pair"][0, 1] and ref["detail"]["pair"][1, 0] and np.isinf(got["sdf"]).all() and np.isinf(got["pair_distance"]).all()
    assert (got["nearest_person"] == -1).all() and (got["pair_inside"] == 0).all()


def test_nested_is_asymmetric():
    got, ref = check("nested")
    V = got["sdf"].shape[1]
    assert got["inside_count"].tolist() == [V, 0] and got["pair_inside"].tolist() == [[0, V], [0, 0]]
    assert (got["sdf"][0] < -0.2).all() and np.isinf(got["sdf"][1]).all() and got["pair_distance"][0, 1] < -0.2 and np.isinf(got["pair_distance"][1, 0])


def test_three_persons_union_minimum_and_the_lowest_b_on_a_tie():
    got, ref = check("three")
    assert set(got["nearest_person"][0].tolist()) == {-1, 1, 2} and np.array_equal(got["nearest_person"], ref["nearest_person"])
    # two identical meshes as b: person 0's rows are those of the two-person scene, bit for bit, and name the lower of the two
    v, idx, f, md, tau = scene("overlap3")
    two = run_abi(v, idx, f, md, tau)
    tie = run_abi(np.stack([v[0], v[1], v[1]]), (0, 0, 0), f, md, tau)
    for n in ("sdf", "nearest_person", "nearest_face", "closest"):
        assert np.array_equal(tie[n][0].view(np.uint8), two[n][0].view(np.uint8)), n
    assert set(tie["nearest_person"][0].tolist()) == {-1, 1} and np.array_equal(tie["pair_distance"][0, 1:], two["pair_distance"][0, 1:].repeat(2))
    assert tie["pair_inside"][0].tolist() == [0, 113, 113] and tie["inside_count"][0] == 113


def test_same_coordinates_in_two_images_do_not_interact():
    got, ref = check("two_images")
    assert np.isinf(got["sdf"]).all() and np.isinf(got["pair_distance"]).all() and (got["inside_count"] == 0).all() and (got["valid"] == 1).all()


def test_torus_threaded_by_a_thin_box():
    got, ref = check("torus")
    nt = 288
    centre = got["sdf"][1, 0]                                            # person 1's collapsed vertices sit at the hole's centre
    assert 0.30 < centre < 0.36 and got["nearest_person"][1, 0] == 0    # outside the torus, although inside its box
    assert abs(ref["detail"]["w"][1, 0, 0]) < 0.05 and (got["sdf"][1, :nt] == centre).all()
    assert got["inside_count"].tolist() == [0, 0] and np.isfinite(got["sdf"][0, :nt]).sum() > 24


@pytest.mark.parametrize("name", ["open", "inverted", "degenerate"])
def test_open_inverted_and_degenerate_meshes(name):
    got, ref = check(name)
    if name == "open":
        assert got["inside_count"].min() > 50
        return
    v, idx, f, md, tau = scene("overlap3")
    up = run_abi(v, idx, f, md, tau)
    if name == "inverted":                                               # |w|: the same signs as the upright mesh
        assert np.array_equal(np.sign(got["sdf"]), np.sign(up["sdf"])) and np.array_equal(got["pair_inside"], up["pair_inside"])
    else:                                                                # skipped faces, placed last, change no output bit
        assert same_bits(got, up)


@pytest.mark.parametrize("name", ["boxes", "tile", "tile_plus_one"])
def test_shapes_that_leave_every_tiling(name):
    got, ref = check(name)
    assert got["inside_count"].sum() > 0
    if name == "tile_plus_one":                                          # the face alone in the second tile is found
        last = contact.FACE_TILE
        assert (ref["nearest_face"] == last).any() and np.array_equal(got["nearest_face"] == last, ref["nearest_face"] == last)


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_nobody_and_one_person():
    v, idx, f, md, tau = scene("overlap2")
    c = contacts(torch.zeros(0, v.shape[1], 3, device=DEV), [], f)
    assert c.sdf.shape == (0, v.shape[1]) and c.closest.shape == (0, v.shape[1], 3) and c.pair_distance.shape == (0, 0) and c.valid.shape == (0,)
    L = _lib.lib()
    d = _lib.ContactDesc()
    d.P, d.V, d.F, d.max_dist, d.tau = 0, 162, 320, md, tau
    assert L.mhmr_contact(C.byref(d), None) == 0
    got = run_abi(v[:1], idx[:1], f, md, tau)
    co.compare(got, co.contacts(v[:1], idx[:1], f, md, tau), v[:1], f, md, tau)
    assert np.isinf(got["sdf"]).all() and got["pair_distance"].tolist() == [[np.inf]] and got["valid"].tolist() == [1]


def test_a_person_with_a_nan_vertex_is_invalid_and_ignored():
    v, idx, f, md, tau = scene("overlap2")
    v3 = np.stack([v[0], v[1], v[1]])
    v3[1, 17, 2] = np.nan
    got = run_abi(v3, (0, 0, 0), f, md, tau)
    ref = co.contacts(v3, (0, 0, 0), f, md, tau)
    co.compare(got, ref, v3, f, md, tau)
    assert got["valid"].tolist() == [1, 0, 1] and np.isinf(got["sdf"][1]).all() and (got["nearest_person"][1] == -1).all()
    assert np.array_equal(got["closest"][1].view(np.uint32), v3[1].view(np.uint32)) and np.isinf(got["aabb"][1]).all()
    assert set(got["nearest_person"][0].tolist()) == {-1, 2} and got["pair_inside"][0].tolist() == [0, 0, 27]
    assert np.isinf(got["pair_distance"][1]).all() and np.isinf(got["pair_distance"][:, 1]).all()


def test_strided_vertices_are_read_in_place():
    v, idx, f, md, tau = scene("overlap2")
    base = run_abi(v, idx, f, md, tau)
    assert same_bits(run_abi(v, idx, f, md, tau, pad=7), base)          # NaN between the persons' rows: never read
    P, V = v.shape[:2]
    block = torch.full((P, V + 5, 3), float("nan"), device=DEV)
    block[:, :V] = torch.from_numpy(v).to(DEV)
    view = block[:, :V]
    assert view.stride(0) > 3 * V and contact._strided(view, view.device, "verts").data_ptr() == view.data_ptr()
    c = contacts(view, idx, f, max_dist=md, tau=tau)
    assert all(np.array_equal(getattr(c, n).cpu().numpy().view(np.uint8), base[n].view(np.uint8)) for n in FIELDS)


def test_every_output_alone_equals_its_value_from_the_full_call():
    v, idx, f, md, tau = scene("overlap2")
    full = run_abi(v, idx, f, md, tau)
    for n in FIELDS:
        one = run_abi(v, idx, f, md, tau, want=(n,))                    # the other ten are NULL
        assert list(one) == [n] and np.array_equal(one[n].view(np.uint8), full[n].view(np.uint8)), n
        py = run_py(v, list(idx), f, md, tau, want=(n,))
        assert all((py[k] is None) == (k != n) for k in FIELDS) and np.array_equal(py[n].view(np.uint8), full[n].view(np.uint8)), n


def test_two_runs_give_the_same_bits():
    v, idx, f, md, tau = scene("overlap3")
    assert same_bits(run_abi(v, idx, f, md, tau), run_abi(v, idx, f, md, tau))


def test_contacts_refuses_bad_faces_and_margins():
    v, idx, f, md, tau = scene("overlap2")
    vd = torch.from_numpy(v).to(DEV)
    bad = f.copy()
    bad[5, 1] = v.shape[1]
    for kw in (dict(faces=bad), dict(tau=0.2), dict(max_dist=-1.0), dict(max_dist=float("nan")), dict(want=("sdf", "nope"))):
        args = dict(faces=f, max_dist=md, tau=tau)
        args.update(kw)
        with pytest.raises(ValueError):
            contacts(vd, idx, **args)
    with pytest.raises(ValueError):
        contacts(vd, [0], f)


# ---------------------------------------------------------------------------------------------------------------- pipeline
S, NAME = 224, "dinov2_vits14"


@functools.lru_cache(maxsize=None)
def model_fixture():
    """The depth-3 ViT-S at 224^2 of tests/test_gpu_maps.py and three synthetic frames."""
    data, mean = synthetic.make_smplx_data(seed=0), synthetic.make_mean_params(seed=0)
    m = Model(backbone=NAME, img_size=S, smplx_data=data, mean_params=mean, backbone_depth=3, precision="f16")
    m.load_state_dict(synthetic.make_state_dict(NAME, S, seed=42, depth_override=3, mean_params=mean), strict=True)
    m = m.to(DEV).eval()
    base = torch.randint(0, 256, (S, S, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    return m, [torch.roll(base, 3 * f, dims=1).numpy() for f in range(3)]


@functools.lru_cache(maxsize=None)
def threshold():
    """Half way between the sixth and the seventh score of a plain run that keeps everything: six persons over the three frames."""
    m, frames = model_fixture()
    scores = sorted((float(h["scores"]) for r in predict_images(m, frames, batch_size=4, det_thresh=1e-6) for h in r.humans), reverse=True)
    return (scores[5] + scores[6]) / 2


def test_predict_video_contacts_adds_the_same_keys_to_the_smoothed_persons():
    from multi_hmr_amd import Tracker, predict_video
    m, frames = model_fixture()
    run = lambda **kw: list(predict_video(m, frames, batch_size=4, tracker=Tracker(m, max_dist=1e3), det_thresh=threshold(), **kw))
    plain, con = run(), run(contacts=True)
    faces = m.smpl_layer["neutral_10"].bm_x.faces
    assert sum(len(r.humans) for r in con) == sum(len(r.humans) for r in plain) > 0
    for a, b in zip(plain, con):
        for ha, hb in zip(a.humans, b.humans):
            assert list(hb) == list(ha) + list(CONTACT_KEYS) == list(m.PERSON_KEYS) + ["track_id", "hits"] + list(CONTACT_KEYS)
            assert all(torch.equal(ha[k], hb[k]) if torch.is_tensor(ha[k]) else ha[k] == hb[k] for k in ha)
        if b.humans:
            ref = contacts(torch.stack([h["v3d"] for h in b.humans]), [0] * len(b.humans), faces)
            assert [h["penetration_depth"] for h in b.humans] == ref.penetration_depth.tolist()
            assert [h["inside_vertices"] for h in b.humans] == ref.inside_count.tolist()
            assert [h["contact_vertices"] for h in b.humans] == ref.contact_count.tolist()
            touching = (torch.minimum(ref.pair_distance, ref.pair_distance.T) <= 0.01).cpu().numpy()
            assert [h["contact_with"] for h in b.humans] == [np.nonzero(t)[0].tolist() for t in touching]


def test_demo_contacts_prints_pairs_and_depths_and_writes_the_files_of_before(tmp_path, monkeypatch, capsys):
    import os
    from PIL import Image
    from multi_hmr_amd import demo
    m, frames = model_fixture()
    monkeypatch.setattr(demo, "load_model", lambda name, *a, **k: m)
    os.makedirs(tmp_path / "imgs")
    Image.fromarray(frames[0]).save(tmp_path / "imgs" / "a.png")
    x, _ = demo.open_image(str(tmp_path / "imgs" / "a.png"), S)
    K = demo.get_camera_parameters(S, fov=60)
    scores = sorted((float(h["scores"]) for h in demo.forward_model(m, x, K, det_thresh=1e-6, nms_kernel_size=3)), reverse=True)
    thr = (scores[2] + scores[3]) / 2
    argv = ["--img_folder", str(tmp_path / "imgs"), "--model_name", "synth", "--det_thresh", repr(thr)]
    plain = demo.main(argv + ["--out_folder", str(tmp_path / "plain")])
    capsys.readouterr()
    written = demo.main(argv + ["--out_folder", str(tmp_path / "out"), "--contacts", "1"])
    out = capsys.readouterr().out
    assert [os.path.basename(p) for p in written] == [os.path.basename(p) for p in plain] == ["a.png_synth.png"]
    assert open(plain[0], "rb").read() == open(written[0], "rb").read()
    humans = demo.forward_model(m, x, K, det_thresh=thr, nms_kernel_size=3)
    ref = contacts(torch.stack([h["v3d"] for h in humans]), [0] * len(humans), m.smpl_layer["neutral_10"].bm_x.faces)
    assert len(humans) == 3 and "  touching: " in out
    for j in range(3):
        assert (f"  person {j}: penetration depth {float(ref.penetration_depth[j]):.3f} m ({int(ref.inside_count[j])} vertices inside another "
                f"person, {int(ref.contact_count[j])} in contact)") in out


def test_predict_images_contacts_adds_four_keys_and_moves_nothing():
    m, frames = model_fixture()
    thr = threshold()
    plain = list(predict_images(m, frames, batch_size=4, det_thresh=thr))
    con = list(predict_images(m, frames, batch_size=4, det_thresh=thr, contacts=True))
    assert sum(len(r.humans) for r in plain) == 6
    faces = m.smpl_layer["neutral_10"].bm_x.faces
    for a, b in zip(plain, con):
        assert len(a.humans) == len(b.humans) and torch.equal(a.K, b.K)
        for ha, hb in zip(a.humans, b.humans):
            assert list(ha) == list(m.PERSON_KEYS) and list(hb) == list(m.PERSON_KEYS) + list(CONTACT_KEYS)
            assert all(torch.equal(ha[k], hb[k]) for k in m.PERSON_KEYS)
        if not b.humans:
            continue
        # the four keys are those of a contacts call on that image's persons alone (the model's faces are random triples: any values)
        n = len(b.humans)
        ref = contacts(torch.stack([h["v3d"] for h in b.humans]), [0] * n, faces)
        touching = (torch.minimum(ref.pair_distance, ref.pair_distance.T) <= 0.01).cpu().numpy()
        for j, h in enumerate(b.humans):
            assert type(h["penetration_depth"]) is float and type(h["inside_vertices"]) is int and type(h["contact_vertices"]) is int
            assert h["penetration_depth"] == float(ref.penetration_depth[j]) and h["inside_vertices"] == int(ref.inside_count[j])
            assert h["contact_vertices"] == int(ref.contact_count[j]) and h["contact_with"] == np.nonzero(touching[j])[0].tolist()


def test_worst_errors_are_reported(capsys):
    """Prints what the scene tests measured (the figures of profiles/contact_tests.txt); the gate is 4 x their maximum."""
    with capsys.disabled():
        for name, w in WORST.items():
            print(f"\ncontact worst errors [{name}]: " + ", ".join(f"{k} {e:.3e}" for k, e in w.items()), end="")
        print()
    assert all(max(w.values()) <= co.GATE for w in WORST.values())
