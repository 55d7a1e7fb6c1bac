"""-m gpu: the tracker (mhmr_track_update, csrc/track.hip; Tracker; predict_video) against tests/track_oracle.py: ``o32``
the contract in numpy fp32 -- the exact yardstick for ids, hits, status and the table's integers -- and ``o64`` the same code in fp64, the
yardstick for the filtered values under the project's rule: per tensor, the kernel's maximum absolute error against ``o64`` may be at most
4x ``o32``'s.  Every pair of figures is printed before anything is asserted (run with -s).  The C entry runs on buffers with sentinels in
front of and behind every output, the table and the workspace, on sentinel-filled outputs, and every call of ``run`` checks those, that every
output element was written and that the inputs kept their bits.

Figures: profiles/track_tests.txt."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import synthetic
import track_oracle as to
from multi_hmr_amd import Model, Preprocessor, Tracker, _lib, predict_images, predict_video
from multi_hmr_amd.preprocess import get_camera_parameters

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT = {torch.float32: -7.25, torch.int64: -7777, torch.int32: -7777}
S, NAME = 224, "dinov2_vits14"


class Guarded:
    """A device buffer with sentinels in front of and behind its data; the data starts as sentinels too unless given."""

    def __init__(self, shape, dtype, data=None):
        self.n = int(np.prod(shape, dtype=np.int64))
        self.sent = SENT[dtype]
        self.big = torch.full((self.n + 2 * GUARD,), self.sent, dtype=dtype, device=DEV)
        self.t = self.big[GUARD:GUARD + self.n].view(shape)
        if data is not None:
            self.t.copy_(data)

    def ok(self):
        return bool((self.big[:GUARD] == self.sent).all()) and bool((self.big[GUARD + self.n:] == self.sent).all())


def run(args, nb, capacity=8, max_dist=0.8, max_age=2, smooth=to.DEFAULT_SMOOTH, fps=30.0, dcutoff=1.0, table=None):
    """mhmr_track_update on the arrays of ``track_oracle.call_args`` -> numpy copies of every output and the table's bytes after the call.
    ``table``: the bytes to start from (None: zeros, the empty tracker)."""
    L = _lib.lib()
    D, F, P = to.width(nb), int(args["F"]), len(args["img_id"])
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)
    inputs = dict(img_id=dev(args["img_id"], torch.int64), idx_y=dev(args["idx_y"], torch.int64), idx_x=dev(args["idx_x"], torch.int64),
                  transl=dev(args["transl"], torch.float32).reshape(P, 3), readout=dev(args["readout"], torch.float32).reshape(P, D),
                  offset=dev(args["offset"], torch.float32).reshape(P, 2))
    before = {k: v.clone() for k, v in inputs.items()}
    sbytes, wbytes = _lib.workspace_bytes("mhmr_track_state_bytes", capacity, D), _lib.workspace_bytes("mhmr_track_workspace_bytes", F, capacity)
    assert sbytes % 8 == 0 and wbytes % 8 == 0
    start = torch.zeros(sbytes // 8, dtype=torch.int64) if table is None else torch.from_numpy(table.copy()).view(torch.int64)
    out = dict(track_id=Guarded((P,), torch.int64), hits=Guarded((P,), torch.int32), readout_s=Guarded((P, D), torch.float32),
               offset_s=Guarded((P, 2), torch.float32), status=Guarded((1,), torch.int32), state=Guarded((sbytes // 8,), torch.int64, start),
               workspace=Guarded((wbytes // 8,), torch.int64))
    d = _lib.TrackDesc()
    d.F, d.P, d.nb, d.capacity = F, P, nb, capacity
    for n, t in inputs.items():
        setattr(d, n, t.data_ptr() or None)
    for n, g in out.items():
        setattr(d, n, g.t.data_ptr() or None)
    d.fps, d.max_dist, d.max_age, d.dcutoff, d.groups = fps, max_dist, max_age, dcutoff, 0
    for bit, g in enumerate(_lib.TRACK_GROUPS):
        if smooth and smooth.get(g) is not None:
            d.groups |= 1 << bit
            setattr(d, "mincutoff_" + g, smooth[g][0])
            setattr(d, "beta_" + g, smooth[g][1])
    d.state_bytes, d.workspace_bytes = sbytes, wbytes
    _lib.check(L.mhmr_track_update(C.byref(d), torch.cuda.current_stream().cuda_stream), "mhmr_track_update")
    torch.cuda.synchronize()
    for n, g in out.items():
        assert g.ok(), f"sentinel of {n} overwritten"
    for n, t in inputs.items():
        assert torch.equal(t, before[n]), f"input {n} was written"
    res = {n: out[n].t.cpu().numpy() for n in ("track_id", "hits", "readout_s", "offset_s")}
    assert not (res["track_id"] == SENT[torch.int64]).any() and not (res["hits"] == SENT[torch.int32]).any()
    assert not (res["readout_s"] == SENT[torch.float32]).any() and not (res["offset_s"] == SENT[torch.float32]).any()      # every element written
    res["status"] = int(out["status"].t.item())
    assert res["status"] in (0, 1)
    res["table"] = out["state"].t.cpu().numpy().view(np.uint8).copy()
    return res


def params(sc, **over):
    return dict(sc["params"], nb=sc["nb"], **over)


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("track_id", "hits", "readout_s", "offset_s", "table")) and \
        a["status"] == b["status"]


def check_integers(res, orc, out, sc):
    """ids, hits, status and the table's integers against the fp32 oracle, exactly."""
    assert res["status"] == out["status"]
    assert np.array_equal(res["track_id"], out["track_id"]) and np.array_equal(res["hits"], out["hits"])
    tv = to.table_views(res["table"], orc.cap, orc.D)
    assert tv["next_id"] == orc.next_id and not tv["reserved"].any()
    for k in ("id", "missed", "hits"):
        assert np.array_equal(tv[k], orc.table()[k]), k
    live = orc.hits > 0
    floats = {k: int((tv[k][live].view(np.uint32) != orc.table()[k][live].view(np.uint32)).sum()) for k in ("pos", "vel", "x", "dx")}
    print(f"  table floats of the live slots that differ from the fp32 oracle's bits: {floats}")
    return tv


@pytest.mark.parametrize("name", sorted(to.scenes()))
def test_scene_ids_hits_and_table_are_the_fp32_oracles(name):
    sc, want = to.scenes()[name]
    orc = to.OracleTracker(sc["nb"], dtype=np.float32, **sc["params"])
    out = orc.update(**to.call_args(sc))
    res = run(to.call_args(sc), **params(sc))
    print(f"{name}: ids {to.ids_by_frame(sc, res['track_id'])}")
    assert res["status"] == 0 and to.ids_by_frame(sc, res["track_id"]) == want
    check_integers(res, orc, out, sc)
    keep = res["hits"] <= 1                                                      # new tracks and rows without a slot: the inputs' bits
    assert keep.any()
    assert np.array_equal(res["readout_s"][keep].view(np.uint32), sc["readout"][keep].view(np.uint32))
    assert np.array_equal(res["offset_s"][keep].view(np.uint32), sc["offset"][keep].view(np.uint32))
    assert np.array_equal(res["hits"] == 0, res["track_id"] == -1)
    if name == "capacity":                                                       # the person without a slot leaves the table as if absent
        m = np.tile([True, True, False], 2)
        two = {k: (v[m] if isinstance(v, np.ndarray) and k != "F" else v) for k, v in to.call_args(sc).items()}
        assert np.array_equal(run(two, **params(sc))["table"], res["table"])
    if name == "crowd":
        assert [int((res["track_id"][sc["img_id"] == f] == -1).sum()) for f in range(3)] == [6, 6, 6]


def test_a_dense_random_walk_is_swept_in_the_contracts_order():
    sc = to.random_walk_scene()
    orc = to.OracleTracker(sc["nb"], dtype=np.float32, **sc["params"])
    out = orc.update(**to.call_args(sc))
    res = run(to.call_args(sc), **params(sc))
    ids = to.ids_by_frame(sc, res["track_id"])
    print(f"random walk: {[len(i) for i in ids]} rows per frame, {orc.next_id} ids, {int((out['track_id'] == -1).sum())} rows without a slot, "
          f"{int((out['hits'] > 1).sum())} matches")
    assert orc.next_id > 40 and (out["hits"] > 1).sum() > 60                  # tracks were lost and started, and most rows matched
    check_integers(res, orc, out, sc)
    tv = to.table_views(res["table"], orc.cap, orc.D)
    for k in ("pos", "vel", "x", "dx"):
        assert np.array_equal(tv[k].view(np.uint32), orc.table()[k].view(np.uint32)), k


def test_a_frame_wider_than_the_kernels_lds_rows():
    sc = to.wide_frame_scene()
    orc = to.OracleTracker(sc["nb"], dtype=np.float32, **sc["params"])
    out = orc.update(**to.call_args(sc))
    res = run(to.call_args(sc), **params(sc))
    assert orc.next_id == 300 and (out["hits"] == 2).sum() == 300 and sorted(out["track_id"][300:]) == list(range(300))
    assert not np.array_equal(out["track_id"][300:], out["track_id"][:300])
    check_integers(res, orc, out, sc)
    for k, name in (("readout_s", "readout"), ("offset_s", "offset")):
        assert np.array_equal(res[k].view(np.uint32), out[name].view(np.uint32)), k


def test_disordered_image_ids_are_refused_on_the_device_and_touch_nothing():
    sc, _ = to.scenes()["leave_and_return"]
    first = run(to.call_args(sc, (0, 4)), **params(sc))                          # a table with two live tracks
    args = to.call_args(sc, (4, 8))
    for bad in (args["img_id"][::-1].copy(), args["img_id"] + 1, args["img_id"] - 1):
        res = run(dict(args, img_id=bad), table=first["table"], **params(sc))
        assert res["status"] == 1 and np.all(res["track_id"] == -1) and np.all(res["hits"] == 0)
        assert np.array_equal(res["readout_s"].view(np.uint32), args["readout"].view(np.uint32))
        assert np.array_equal(res["offset_s"].view(np.uint32), args["offset"].view(np.uint32))
        assert np.array_equal(res["table"], first["table"])


@pytest.mark.parametrize("nb", [10, 11])
def test_filtered_values_against_fp64_and_the_exact_properties_of_one_recursion(nb):
    sc = to.filter_scene(nb)
    kw = params(sc)
    o32, o64 = (to.OracleTracker(nb, dtype=dt, **sc["params"]) for dt in (np.float32, np.float64))
    a32, a64 = o32.update(**to.call_args(sc)), o64.update(**to.call_args(sc))
    whole = run(to.call_args(sc), **kw)
    check_integers(whole, o32, a32, sc)
    assert sorted(set(whole["hits"])) == list(range(1, 9)) and np.array_equal(a32["track_id"], a64["track_id"])
    for k, name in (("readout_s", "readout"), ("offset_s", "offset")):
        e_k, e_y = float(np.abs(whole[k] - a64[name]).max()), float(np.abs(a32[name].astype(np.float64) - a64[name]).max())
        print(f"nb {nb} {name}: kernel against fp64 {e_k:.3e}, fp32 oracle against fp64 {e_y:.3e}, ratio {e_k / e_y:.2f}")
        assert e_y > 0 and e_k <= 4 * e_y
    assert float(np.abs(whole["readout_s"] - sc["readout"]).max()) > 0.5         # the filter did something
    # two calls, equal bits
    assert same_bits(whole, run(to.call_args(sc), **kw))
    # 8 frames = 4 + 4 = 8 x 1 through the table
    for cuts in ((0, 4, 8), tuple(range(9))):
        table, parts = None, []
        for a, b in zip(cuts, cuts[1:]):
            parts.append(run(to.call_args(sc, (a, b)), table=table, **kw))
            table = parts[-1]["table"]
        for k in ("track_id", "hits", "readout_s", "offset_s"):
            assert np.array_equal(np.concatenate([p[k] for p in parts]).view(np.uint8), whole[k].view(np.uint8)), (cuts, k)
        assert np.array_equal(table, whole["table"]) and all(p["status"] == 0 for p in parts)
    # cam[1:3] pass through; a group set to None is a select: its columns keep the input's bits and its state is never written
    cam12 = slice(318 + nb + 1, 318 + nb + 3)
    assert np.array_equal(whole["readout_s"][:, cam12].view(np.uint32), sc["readout"][:, cam12].view(np.uint32))
    part = run(to.call_args(sc), **dict(kw, smooth=dict(to.DEFAULT_SMOOTH, pose=None, loc=None)))
    assert np.array_equal(part["readout_s"][:, :318].view(np.uint32), sc["readout"][:, :318].view(np.uint32))
    assert np.array_equal(part["offset_s"].view(np.uint32), sc["offset"].view(np.uint32))
    assert np.array_equal(part["readout_s"][:, 318:].view(np.uint32), whole["readout_s"][:, 318:].view(np.uint32))
    tv = to.table_views(part["table"], 8, to.width(nb))
    assert not tv["x"][:, :318].any() and not tv["x"][:, -2:].any() and not tv["dx"][:, :318].any() and tv["x"][:2, 318:-2].all()
    none = run(to.call_args(sc), **dict(kw, smooth=None))                        # smooth=None tracks only
    assert np.array_equal(none["readout_s"].view(np.uint32), sc["readout"].view(np.uint32))
    assert np.array_equal(none["offset_s"].view(np.uint32), sc["offset"].view(np.uint32))
    assert np.array_equal(none["track_id"], whole["track_id"]) and not to.table_views(none["table"], 8, to.width(nb))["x"].any()


def test_a_constant_sequence_is_a_fixed_point_and_a_cell_border_is_invisible():
    sc = to.make_scene([[(0.0, 0.0, 3.0), (2.0, 0.5, 4.0)]] * 6, nb=10, seed=21)
    for k in ("readout", "offset", "idx_x", "idx_y"):                            # every frame repeats frame 0's rows
        sc[k] = np.concatenate([sc[k][:2]] * 6)
    res = run(to.call_args(sc), **params(sc))
    assert to.ids_by_frame(sc, res["track_id"]) == [[0, 1]] * 6
    assert np.array_equal(res["readout_s"].view(np.uint32), sc["readout"].view(np.uint32))           # x == z, bit for bit
    tv = to.table_views(res["table"], 8, to.width(sc["nb"]))
    assert not tv["dx"].any()
    # the same absolute location from two cells: cell 3 + 0.5 + 0.5 and cell 4 + 0.5 - 0.5 feed identical bits into the filter
    one = to.make_scene([[(0.0, 0.0, 3.0)]] * 4, nb=11, seed=22)
    one["idx_x"][:], one["offset"][:, 0] = 3, 0.5
    two = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in one.items()}
    two["idx_x"][1:], two["offset"][1:, 0] = 4, -0.5
    ra, rb = run(to.call_args(one), **params(one)), run(to.call_args(two), **params(two))
    assert np.array_equal(ra["table"], rb["table"]) and np.array_equal(ra["readout_s"].view(np.uint32), rb["readout_s"].view(np.uint32))
    assert np.array_equal(ra["offset_s"][:, 1].view(np.uint32), rb["offset_s"][:, 1].view(np.uint32))
    assert np.array_equal(ra["offset_s"][1:, 0] - 1.0, rb["offset_s"][1:, 0])                        # relative to the detection's own cell


def test_permuting_a_frames_rows_permutes_its_outputs():
    rng = np.random.default_rng(5)
    base = rng.uniform(-2, 2, (3, 3)) + np.array([0, 0, 5.0])
    frames = [[tuple(p + 0.05 * f * (i + 1)) for i, p in enumerate(base)] for f in range(4)]       # distinct speeds: no ties
    sc = to.make_scene(frames, nb=10, seed=23)
    res = run(to.call_args(sc), **params(sc))
    assert to.ids_by_frame(sc, res["track_id"]) == [[0, 1, 2]] * 4
    perm = np.arange(12)
    perm[6:9] = [8, 6, 7]                                                        # frame 2's rows, rotated
    sp = dict(sc, **{k: sc[k][perm] for k in ("idx_y", "idx_x", "transl", "readout", "offset")})
    rp = run(to.call_args(sp), **params(sp))
    for k in ("track_id", "hits", "readout_s", "offset_s"):
        assert np.array_equal(rp[k].view(np.uint8), res[k][perm].view(np.uint8)), k
    assert np.array_equal(rp["table"], res["table"])


# ---------------------------------------------------------------------------------------------------- the model level
@functools.lru_cache(maxsize=None)
def fixture():
    """The depth-3 ViT-S at 224^2 of the fit's model test, six frames of one synthetic image shifted three pixels per frame, their camera and
    score maps.  Built once, shared, never modified."""
    data, mean = synthetic.make_smplx_data(seed=0), synthetic.make_mean_params(seed=0)
    m = Model(backbone=NAME, img_size=S, smplx_data=data, mean_params=mean, backbone_depth=3, precision="f16")
    m.load_state_dict(synthetic.make_state_dict(NAME, S, seed=42, depth_override=3, mean_params=mean), strict=True)
    m = m.to(DEV).eval()
    base = torch.randint(0, 256, (S, S, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    frames = [torch.roll(base, 3 * f, dims=1).numpy() for f in range(6)]
    x = Preprocessor(S, torch.device(DEV)).batch([torch.from_numpy(f) for f in frames])
    K = get_camera_parameters(S, fov=60, device=torch.device(DEV), batch=6)
    z = torch.zeros(1, dtype=torch.long, device=DEV)
    scores = m(x, idx=(z, z + 3, z + 5), K=K, is_training=True)["scores"].reshape(6, -1)
    return m, frames, x, K, scores


def between(scores, n):
    """A threshold half way between the n-th and the (n + 1)-th largest score: the low bits of another batch size do not move a detection."""
    top = scores.flatten().sort(descending=True).values
    return float(top[n - 1] + top[n]) / 2


def test_predict_video_tracks_and_smooth_none_is_predict_images():
    m, frames, _, _, scores = fixture()
    thr = between(scores, 18)                                                    # at most 18 detections over the six frames, fewer after the NMS
    plain = list(predict_images(m, frames, batch_size=4, det_thresh=thr))
    counts = [len(r.humans) for r in plain]
    assert 2 <= sum(counts) <= 18
    # random weights: the positions are not a moving person's, so the gate is open; then the ids are as many as the fullest frame's persons
    tracked = list(predict_video(m, frames, batch_size=4, tracker=Tracker(m, max_dist=1e3, smooth=None), det_thresh=thr))
    ids = [[h["track_id"] for h in r.humans] for r in tracked]
    print(f"persons per frame {counts}, ids {ids}")
    assert [len(i) for i in ids] == counts and all(len(set(i)) == len(i) and min(i, default=0) >= 0 for i in ids)
    assert len({t for i in ids for t in i}) == max(counts)                       # one id per person throughout (two batches: 4 + 2 frames)
    seen = {}
    for r in tracked:
        for h in r.humans:
            seen[h["track_id"]] = seen.get(h["track_id"], 0) + 1
            assert h["hits"] == seen[h["track_id"]]
    worst = 0.0
    for a, b in zip(plain, tracked):                                             # smooth=None: predict_images' persons, key for key
        assert a.index == b.index and torch.equal(a.K, b.K) and torch.equal(a.K_full, b.K_full) and a.size == b.size
        for ha, hb in zip(a.humans, b.humans):
            assert list(hb) == list(m.PERSON_KEYS) + ["track_id", "hits"] and list(ha) == list(m.PERSON_KEYS)
            for k in m.PERSON_KEYS:
                worst = max(worst, float((ha[k].double() - hb[k].double()).norm() / ha[k].double().norm().clamp_min(1e-30)))
    print(f"smooth=None against predict_images: worst rel-L2 {worst:.3e}")
    assert worst == 0.0
    # the default tracker smooths: finite persons, the same keys
    smoothed = list(predict_video(m, frames, batch_size=4, tracker=Tracker(m, max_dist=1e3), det_thresh=thr))
    assert [[h["track_id"] for h in r.humans] for r in smoothed] == ids
    assert all(bool(torch.isfinite(h[k]).all()) for r in smoothed for h in r.humans for k in m.PERSON_KEYS)


def test_tracker_state_round_trip_and_the_filter_steadies_a_noisy_still_sequence():
    m, frames, x6, K6, scores = fixture()
    x, K = x6[:1], K6[:1]
    rows, ids = m(x, K=K, det_thresh=between(scores[0], 3), return_batched=True, return_readout=True)
    P, F = int(ids.shape[0]), 8
    assert P >= 1
    g = torch.Generator().manual_seed(9)
    noise = 0.05 * torch.randn(F, P, rows["readout"].shape[1], generator=g).to(DEV)
    rep = lambda t: t.repeat(F, *([1] * (t.dim() - 1)))
    batch = dict(readout=(rows["readout"][None] + noise).flatten(0, 1), offset=rep(rows["offset"]), transl=rep(rows["transl"]),
                 idx=tuple(rep(i) for i in rows["idx"]))
    img = torch.arange(F, device=DEV).repeat_interleave(P)
    kept = {k: (v.clone() if torch.is_tensor(v) else tuple(i.clone() for i in v)) for k, v in batch.items()}
    t = Tracker(m, capacity=16)
    res = t.update(batch, img, F)
    assert int(res.status) == 0 and res.track_id.view(F, P).eq(torch.arange(P, device=DEV)).all() and int(res.hits.max()) == F
    for k in ("readout", "offset", "transl"):                                    # the caller's tensors keep their bits
        assert torch.equal(batch[k], kept[k])
    Kf = K.repeat(F, 1, 1)
    idx = (img, batch["idx"][1], batch["idx"][2])
    dec = m.decode_readout(res.readout, res.offset, idx, Kf)
    raw = m.decode_readout(batch["readout"], batch["offset"], idx, Kf)
    assert all(bool(torch.isfinite(dec[k]).all()) for k in m.PERSON_KEYS if k != "scores")
    move = lambda d: float((d["j3d"].view(F, P, -1, 3)[1:] - d["j3d"].view(F, P, -1, 3)[:-1]).norm(dim=-1).mean())
    ratio = move(dec) / move(raw)
    print(f"frame-to-frame j3d movement, filtered / raw: {ratio:.3f} ({P} persons, {F} frames)")
    assert ratio < 1
    # state_dict round trip: 8 frames = 4, save, load into another tracker, 4
    half = lambda a, b: (dict(readout=batch["readout"][a * P:b * P], offset=batch["offset"][a * P:b * P], transl=batch["transl"][a * P:b * P],
                              idx=tuple(i[a * P:b * P] for i in batch["idx"])), img[a * P:b * P] - a, b - a)
    t1 = Tracker(m, capacity=16)
    r1 = t1.update(*half(0, 4))
    t2 = Tracker(m, capacity=16)
    t2.load_state_dict(t1.state_dict())
    r2 = t2.update(*half(4, 8))
    for k in ("track_id", "hits", "readout", "offset"):
        assert torch.equal(torch.cat([getattr(r1, k), getattr(r2, k)]), getattr(res, k)), k
    assert torch.equal(t2.table, t.table) and not torch.equal(t1.table, t.table)
    empty = t2.update({}, torch.zeros(0, dtype=torch.int32, device=DEV), 3)      # nobody: time passes
    assert int(empty.status) == 0 and empty.track_id.numel() == 0 and not torch.equal(t2.table, t.table)
    t2.reset()
    assert not t2.table.any()

