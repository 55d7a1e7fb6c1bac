"""-m gpu: the per-pixel maps, statistics, amodal area and point visibility (csrc/render_maps.hip, multi_hmr_amd/maps.py) against
tests/maps_oracle.py and against the torch expressions on the ``return_debug`` keys a user would write without them.  Every assertion is
bit-exact: every value is an integer, an fp32 copied out of a key, or a comparison of fp64 values formed in the rasteriser's own operation
order.  Image sizes 37 x 29 and 64 x 48: row segments that end inside a wave, heights that are no multiple of the 4-row tile."""
import functools
import os

import numpy as np
import pytest
import torch

import maps_oracle as mo
import render_exact as rx
import render_oracle as ro
import synthetic
from multi_hmr_amd import Model, demo, maps, predict_images, render
from multi_hmr_amd.pipeline import OCCLUSION_KEYS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(29, 37), (48, 64)]                      # (H, W)
LABELS4 = (np.arange(80) * 7 % 4).astype(np.uint8)
NPTS = 256


@functools.lru_cache(maxsize=None)
def scene(H, W, NV):
    """B = 2 with image 1 empty; three icosphere(1) meshes (V = 42, F = 80) overlapping on screen at depths 3.0, 3.5 and 4.1 and a
    fourth whose image_index is out of range.  Returns (verts [4, 42, 3], image_index, K [2, 3, 3], faces, Rt [2, NV, 3, 4] or None),
    the oracle's keys, maps and amodal area with and without labels.  Built once, shared, never modified."""
    sv, faces = ro.icosphere(1)
    centres = np.float32([[-0.35, 0.1, 3.0], [0.25, -0.15, 3.5], [0.0, 0.3, 4.1], [0.0, 0.0, 3.0]])
    verts = (sv[None] * np.float32([0.75, 0.8, 0.9, 0.8])[:, None, None] + centres[:, None]).astype(np.float32)
    idx = np.array([0, 0, 0, 2], np.int32)
    f = 0.9 * W
    K = np.float32([[[f, 0, W / 2 + 0.3], [0, f, H / 2 - 0.2], [0, 0, 1]], [[f * 1.1, 0, W / 2], [0, f * 1.1, H / 2], [0, 0, 1]]])
    Rt = None
    if NV > 1:
        o = demo.orbit_extrinsics(centres[:3].mean(0), "y", [0.0, 25.0, -40.0][:NV]).astype(np.float32)
        Rt = np.stack([o, o[::-1]])
    keys = mo.scene_keys(verts, idx, K, faces, H, W, Rt)
    want = {L: mo.maps(keys, 4, 80, idx, face_label=LABELS4 if L else None) for L in (0, 4)}
    am = mo.amodal(verts, idx, K, faces, H, W, Rt)
    assert (want[0]["visible_px"][:3] > 0).all() and (want[0]["visible_px"][:3] < am[:3]).any() and want[0]["visible_px"][3].sum() == 0
    return (verts, idx, K, faces, Rt), keys, want, am


def call(sc, size, multi, **kw):
    verts, idx, K, faces, Rt = sc
    Rt_in = None if Rt is None else (Rt if multi else Rt[:, 0])
    return maps.render_maps(torch.from_numpy(verts).to(DEV), idx, K, faces, size, Rt=Rt_in, **kw)


def host(m):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in m._asdict().items()}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("L", [0, 4])
@pytest.mark.parametrize("NV", [1, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_maps_and_statistics_equal_the_oracle_and_torch(H, W, NV, L):
    sc, keys, want, am = scene(H, W, NV)
    multi = NV > 1
    m = call(sc, (H, W), multi, face_labels=LABELS4 if L else None)
    got = host(m)
    sq = (lambda a: a) if multi else (lambda a: a[:, 0])
    assert np.array_equal(got["keys"].view(np.uint64), sq(keys))                                   # the rasteriser's own exactness
    for k in ("person", "face", "depth", "visible_px", "bbox", "zmin") + (("label", "label_px") if L else ()):
        assert same_bits(got[k], sq(want[L][k])), k
    if not L:
        assert got["label"] is None and got["label_px"] is None
    assert same_bits(got["amodal_px"], sq(am)) and same_bits(got["occlusion"], sq(mo.occlusion(want[L]["visible_px"], am)))
    # the torch route of today: arithmetic on the return_debug keys
    kt = m.keys
    low, none = kt & 0xFFFFFFFF, kt == -1
    person_t = torch.where(none, -1, low // 80).int()
    face_t = torch.where(none, -1, low % 80).int()
    depth_t = torch.where(none, 0, kt >> 32).int().view(torch.float32)
    assert torch.equal(m.person, person_t) and torch.equal(m.face, face_t) and torch.equal(m.depth.view(torch.int32), depth_t.view(torch.int32))
    for v in range(NV):
        pv = (m.person[:, v] if multi else m.person).long()
        cnt = torch.bincount(pv[pv >= 0], minlength=4)
        vis = m.visible_px[:, v] if multi else m.visible_px
        assert torch.equal(vis.long(), cnt)
    # invariants
    vis, amo = got["visible_px"], got["amodal_px"]
    assert (vis <= amo).all() and (vis[3] == 0).all() and (amo[3] == 0).all()
    if L:
        assert np.array_equal(got["label_px"].sum(-1), vis)
    box = got["bbox"].reshape(4, NV, 4)
    for p in range(3):
        for v in range(NV):
            ys, xs = np.nonzero(sq(want[L]["person"])[0][v] == p if multi else sq(want[L]["person"])[0] == p)
            assert box[p, v].tolist() == [xs.min(), ys.min(), xs.max(), ys.max()]
    assert (box[3] == [W, H, -1, -1]).all() and np.isinf(got["zmin"][3]).all()
    # a second call: the same bits in every field; keys handed in: the same again, without a render
    again, given = host(call(sc, (H, W), multi, face_labels=LABELS4 if L else None)), host(call(sc, (H, W), multi, keys=m.keys,
                                                                                               face_labels=LABELS4 if L else None))
    for k, a in got.items():
        for other in (again, given):
            assert (a is None and other[k] is None) or same_bits(a, other[k]), k


@pytest.mark.parametrize("H,W", SIZES)
def test_a_view_of_a_multi_view_call_is_the_one_view_call(H, W):
    sc, _, _, _ = scene(H, W, 3)
    verts, idx, K, faces, Rt = sc
    pts = torch.from_numpy(verts).to(DEV)
    m = host(call(sc, (H, W), True, face_labels=LABELS4, points=pts))
    for v in range(3):
        one = host(maps.render_maps(pts, idx, K, faces, (H, W), Rt=Rt[:, v], face_labels=LABELS4, points=pts))
        for k in ("person", "face", "depth", "label", "keys"):
            assert same_bits(m[k][:, v], one[k]), (k, v)
        for k in ("visible_px", "amodal_px", "occlusion", "bbox", "zmin", "label_px", "point_visibility"):
            assert same_bits(np.ascontiguousarray(m[k][:, v]), one[k]), (k, v)


@pytest.mark.parametrize("NV", [1, 3])
def test_amodal_is_the_one_person_render_and_does_not_depend_on_the_pass_size(NV):
    H, W = SIZES[0]
    sc, _, _, am = scene(H, W, NV)
    verts, idx, K, faces, Rt = sc
    Rt4 = np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32), (2, 1, 1, 1)) if Rt is None else Rt
    vt = torch.from_numpy(verts).to(DEV)
    black = torch.zeros(2, H, W, 3, dtype=torch.uint8, device=DEV)
    alone = torch.zeros(4, NV, dtype=torch.int64)
    for p in range(4):
        _, k, _ = render.render_views(black, vt[p:p + 1], idx[p:p + 1], K, faces, Rt4, return_debug=True)
        alone[p] = (k != -1).sum(dim=(0, 2, 3)).cpu()
    assert np.array_equal(alone.numpy(), am)
    full = maps.render_maps(vt, idx, K, faces, (H, W), Rt=Rt4)
    floor = maps.amodal_pass_bytes((H, W), 80, NV)
    single = maps.render_maps(vt, idx, K, faces, (H, W), Rt=Rt4, keys=full.keys, max_workspace_bytes=floor)       # one person per pass
    pair = maps.render_maps(vt, idx, K, faces, (H, W), Rt=Rt4, keys=full.keys, max_workspace_bytes=2 * floor)     # two, two
    for m in (full, single, pair):
        assert torch.equal(m.amodal_px.cpu().long(), alone)
    with pytest.raises(ValueError):
        maps.render_maps(vt, idx, K, faces, (H, W), Rt=Rt4, keys=full.keys, max_workspace_bytes=floor - 1)
    off = maps.render_maps(vt, idx, K, faces, (H, W), Rt=Rt4, keys=full.keys, amodal=False)
    assert off.amodal_px is None and off.occlusion is None and torch.equal(off.visible_px, full.visible_px)


def seeded_points(verts, seed):
    """256 points per person: most inside the view volume around the meshes, some far to the side (outside the image), some behind
    znear or the camera, some with a NaN or an infinite coordinate."""
    g = np.random.default_rng(seed)
    P = len(verts)
    pts = (g.uniform(-1.2, 1.2, (P, NPTS, 3)) * [1.0, 1.0, 1.0] + [0.0, 0.0, 3.5]).astype(np.float32)
    pts[:, 200:216, 0] += np.float32(40.0)                                 # far right: outside
    pts[:, 216:224, 1] -= np.float32(40.0)
    pts[:, 224:232, 2] = np.float32(0.04)                                  # nearer than znear = fl32(0.05)
    pts[:, 232:240, 2] = np.float32(-2.0)
    pts[:, 240:244, 0] = np.nan
    pts[:, 244:248, 2] = np.nan
    pts[:, 248:252, 1] = np.inf
    pts[:, 252:256, 2] = np.inf
    return pts


@pytest.mark.parametrize("tau", [0.0, 0.03])
@pytest.mark.parametrize("NV", [1, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_point_visibility_equals_the_oracle(H, W, NV, tau):
    sc, keys, _, _ = scene(H, W, NV)
    verts, idx, K, faces, Rt = sc
    multi = NV > 1
    sq = (lambda a: a) if multi else (lambda a: a[:, 0])
    for name, pts in (("vertices", verts), ("seeded", seeded_points(verts, 5))):
        want = mo.point_visibility(pts, idx, K, keys, Rt, tau=tau)
        block = torch.zeros(4, pts.shape[1] + 5, 3, device=DEV)            # a person stride that is not 3 N: read in place
        block[:, :pts.shape[1]] = torch.from_numpy(pts).to(DEV)
        m = call(sc, (H, W), multi, points=block[:, :pts.shape[1]], tau=tau, amodal=False)
        got = m.point_visibility.cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, sq(want)), (name, int((got != sq(want)).sum()))
        codes = set(np.unique(want[:3]))
        assert codes >= ({0, 1} if name == "vertices" else {0, 1, 2, 3}), (name, codes)         # the scene exercises every code
        assert (want[3] == 2).all()
    assert call(sc, (H, W), multi, points=torch.zeros(4, 0, 3, device=DEV), amodal=False).point_visibility.shape == ((4, NV, 0) if multi else (4, 0))


def test_nobody():
    H, W = SIZES[0]
    K = scene(H, W, 1)[0][2]
    faces = ro.icosphere(1)[1]
    for Rt, shape in ((None, (2, H, W)), (np.zeros((2, 3, 3, 4), np.float32), (2, 3, H, W))):
        m = maps.render_maps(torch.zeros(0, 42, 3, device=DEV), [], K, faces, (H, W), Rt=Rt, face_labels=LABELS4,
                             points=torch.zeros(0, 7, 3, device=DEV))
        assert m.person.shape == shape and bool((m.person == -1).all()) and bool((m.face == -1).all()) and bool((m.depth == 0).all())
        assert bool((m.label == 255).all()) and bool((m.keys == -1).all())
        n = shape[1:2] if len(shape) == 4 else ()
        assert m.visible_px.shape == (0,) + n and m.bbox.shape == (0,) + n + (4,) and m.label_px.shape == (0,) + n + (4,)
        assert m.amodal_px.shape == (0,) + n and m.occlusion.shape == (0,) + n and m.point_visibility.shape == (0,) + n + (7,)


@pytest.mark.parametrize("name", ["twins", "doubled", "crossing"])
def test_depth_ties_go_to_the_lower_person_and_face(name):
    verts, faces, K, H, W = getattr(rx, "tie_scene_" + name)()
    P, F = len(verts), len(faces)
    idx = np.zeros(P, np.int32)
    m = host(maps.render_maps(torch.from_numpy(verts).to(DEV), idx, K[None], faces, (H, W)))
    keys = mo.scene_keys(verts, idx, K[None], faces, H, W)
    want = mo.maps(keys, P, F, idx)
    for k in ("person", "face", "depth", "visible_px", "bbox", "zmin"):
        assert same_bits(m[k], want[k][:, 0]), k
    drawn = m["person"][0] >= 0
    assert drawn.any()
    if name == "twins":                                                    # every pixel is a tie between the persons
        assert (m["person"][0][drawn] == 0).all() and m["visible_px"].tolist() == [int(drawn.sum()), 0]
        assert m["amodal_px"].tolist() == [int(drawn.sum())] * 2 and m["occlusion"].tolist() == [0.0, 1.0]
    elif name == "doubled":                                                # face f and face F / 2 + f are one triangle
        assert (m["face"][0][drawn] < F // 2).all()
    else:
        tied = rx.tied_pixels(verts, faces, K, H, W)
        assert tied[:, rx.TIE_COL].any() and (m["person"][0][tied] == 0).all()


# ---------------------------------------------------------------------------------------------------- the surfaces users touch
S, NAME = 224, "dinov2_vits14"


@functools.lru_cache(maxsize=None)
def model_fixture():
    """The depth-3 ViT-S at 224^2 of tests/test_gpu_track.py, three synthetic frames and a threshold that keeps a handful of persons."""
    data, mean = synthetic.make_smplx_data(seed=0), synthetic.make_mean_params(seed=0)
    m = Model(backbone=NAME, img_size=S, smplx_data=data, mean_params=mean, backbone_depth=3, precision="f16")
    m.load_state_dict(synthetic.make_state_dict(NAME, S, seed=42, depth_override=3, mean_params=mean), strict=True)
    m = m.to(DEV).eval()
    base = torch.randint(0, 256, (S, S, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    frames = [torch.roll(base, 3 * f, dims=1).numpy() for f in range(3)]
    return m, frames


def _threshold(m, frames, n):
    """Half way between the n-th and the (n + 1)-th score of a plain run at a threshold that keeps everything."""
    scores = sorted((float(h["scores"]) for r in predict_images(m, frames, batch_size=4, det_thresh=1e-6) for h in r.humans), reverse=True)
    assert len(scores) > n
    return (scores[n - 1] + scores[n]) / 2


def test_predict_images_occlusion_adds_four_keys_and_moves_nothing():
    m, frames = model_fixture()
    thr = _threshold(m, frames, 6)
    plain = list(predict_images(m, frames, batch_size=4, det_thresh=thr))
    occ = list(predict_images(m, frames, batch_size=4, det_thresh=thr, occlusion=True))
    assert sum(len(r.humans) for r in plain) == 6
    faces = m.smpl_layer["neutral_10"].bm_x.faces
    for a, b in zip(plain, occ):
        assert len(a.humans) == len(b.humans) and torch.equal(a.K, b.K)
        for ha, hb in zip(a.humans, b.humans):
            assert list(ha) == list(m.PERSON_KEYS) and list(hb) == list(m.PERSON_KEYS) + list(OCCLUSION_KEYS)
            for k in m.PERSON_KEYS:
                assert torch.equal(ha[k], hb[k]), k
        if not b.humans:
            continue
        # the four keys are those of a render_maps call on that image's persons alone (other images do not touch them)
        ref = maps.render_maps(torch.stack([h["v3d"] for h in b.humans]), torch.zeros(len(b.humans), dtype=torch.int32), b.K, faces, (S, S))
        for j, h in enumerate(b.humans):
            assert h["visible_px"].is_cuda and h["visible_px"].dtype == torch.int32 and h["bbox_visible"].shape == (4,)
            assert int(h["visible_px"]) == int(ref.visible_px[j]) and int(h["amodal_px"]) == int(ref.amodal_px[j])
            assert float(h["occlusion"]) == float(ref.occlusion[j]) and torch.equal(h["bbox_visible"], ref.bbox[j])
            assert 0 <= int(h["visible_px"]) <= int(h["amodal_px"]) and 0.0 <= float(h["occlusion"]) <= 1.0


def test_predict_video_occlusion_adds_the_same_keys_to_the_smoothed_persons():
    from multi_hmr_amd import Tracker, predict_video
    m, frames = model_fixture()
    thr = _threshold(m, frames, 6)
    run = lambda **kw: list(predict_video(m, frames, batch_size=4, tracker=Tracker(m, max_dist=1e3), det_thresh=thr, **kw))
    plain, occ = run(), run(occlusion=True)
    faces = m.smpl_layer["neutral_10"].bm_x.faces
    assert sum(len(r.humans) for r in occ) == sum(len(r.humans) for r in plain) > 0
    for a, b in zip(plain, occ):
        for ha, hb in zip(a.humans, b.humans):
            assert list(hb) == list(ha) + list(OCCLUSION_KEYS) == list(m.PERSON_KEYS) + ["track_id", "hits"] + list(OCCLUSION_KEYS)
            assert all(torch.equal(ha[k], hb[k]) if torch.is_tensor(ha[k]) else ha[k] == hb[k] for k in ha)
        if b.humans:
            ref = maps.render_maps(torch.stack([h["v3d"] for h in b.humans]), torch.zeros(len(b.humans), dtype=torch.int32), b.K, faces, (S, S))
            assert torch.equal(torch.stack([h["visible_px"] for h in b.humans]), ref.visible_px)
            assert torch.equal(torch.stack([h["amodal_px"] for h in b.humans]), ref.amodal_px)
            assert torch.equal(torch.stack([h["occlusion"] for h in b.humans]), ref.occlusion)
            assert torch.equal(torch.stack([h["bbox_visible"] for h in b.humans]), ref.bbox)


def test_demo_save_masks_writes_the_two_pngs(tmp_path, monkeypatch, capsys):
    from PIL import Image
    m, frames = model_fixture()
    monkeypatch.setattr(demo, "load_model", lambda name, *a, **k: m)
    os.makedirs(tmp_path / "imgs")
    Image.fromarray(frames[0]).save(tmp_path / "imgs" / "a.png")
    # a threshold half way between the third and the fourth score of the forward the demo itself makes
    x, pil = demo.open_image(str(tmp_path / "imgs" / "a.png"), S)
    K = demo.get_camera_parameters(S, fov=60)
    scores = sorted((float(h["scores"]) for h in demo.forward_model(m, x, K, det_thresh=1e-6, nms_kernel_size=3)), reverse=True)
    thr = (scores[2] + scores[3]) / 2
    argv = ["--img_folder", str(tmp_path / "imgs"), "--model_name", "synth", "--det_thresh", repr(thr)]
    plain = demo.main(argv + ["--out_folder", str(tmp_path / "plain")])
    written = demo.main(argv + ["--out_folder", str(tmp_path / "out"), "--save_masks", "1"])
    stem = str(tmp_path / "out" / "a.png_synth")
    assert [os.path.basename(p) for p in plain] == ["a.png_synth.png"]                           # flag off: the files of before
    assert written == [stem + ".png", stem + "_mask.png", stem + "_parts.png"]
    assert open(plain[0], "rb").read() == open(written[0], "rb").read()
    mask, parts = np.asarray(Image.open(stem + "_mask.png")), np.asarray(Image.open(stem + "_parts.png"))
    assert mask.shape == parts.shape == (S, S) and mask.dtype == np.uint8
    # the same persons, drawn again here (the photograph has the model's size, so its camera is the model's)
    humans = demo.forward_model(m, x, K, det_thresh=thr, nms_kernel_size=3)
    assert len(humans) == 3
    ref = maps.render_maps(torch.stack([h["v3d"] for h in humans]), torch.zeros(3, dtype=torch.int32), K, m.smpl_layer["neutral_10"].bm_x.faces,
                           (S, S), face_labels=m.face_part_labels())
    drawn = [p for p in range(3) if int(ref.visible_px[p]) > 0]
    with capsys.disabled():
        print(f"visible_px {ref.visible_px.tolist()}, amodal_px {ref.amodal_px.tolist()}, drawn {drawn}")
    assert set(np.unique(mask)) - {0} == {p + 1 for p in drawn}
    assert int(mask.max()) == len(drawn) == 3                                                    # max(mask) = the number of persons drawn
    assert np.array_equal(mask, (ref.person[0] + 1).cpu().numpy()) and np.array_equal(parts, ((ref.label[0].int() + 1) % 256).cpu().numpy())
    assert ((parts > 0) == (mask > 0)).all()
    out = capsys.readouterr().out
    for p in range(3):
        assert f"person {p}: occlusion {float(ref.occlusion[p]):.3f}" in out
