"""-m gpu: the batched evaluation on the device (csrc/evalm.hip mhmr_eval_match / mhmr_eval_mesh_errors_indexed, Evaluator.update_batched,
evaluate_dataset(batched=True)).  Every matching decision is exact: against the reference's goldens taken as one
batch, and against ``ev.match_2d_greedy`` image by image on seeded batches whose input conditions tests/test_eval_batched_host.py asserts.
The indexed metrics carry the bits of ``ev.mesh_errors`` on gathered copies; the Evaluator agrees with ``update`` called image by image."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_match_oracle as mo  # noqa: E402
from multi_hmr_amd import _lib  # noqa: E402
from multi_hmr_amd import evaluate as ev  # noqa: E402

DEV = torch.device("cuda:0")
KEYS = ("pair_pred", "pair_gt", "pred_fp", "gt_miss", "counters")
SENTINEL, PAD = 77, 5


def raw_match(pred, pimg, gt, gimg, B, counters=None, status=None, thresh=0.05):
    """mhmr_eval_match through the C ABI with PAD sentinel words behind every output -> dict of numpy arrays (``*_tail``: the sentinels)."""
    L = _lib.lib()
    P, G, J = len(pred), len(gt), gt.shape[1]
    M = min(P, G)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    dp, dpi, dg, dgi = t(pred), t(pimg), t(gt), t(gimg)
    out = {k: torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device=DEV) for k, n in (("pair_pred", M), ("pair_gt", M), ("pred_fp", P), ("gt_miss", G))}
    counters = torch.zeros(4, dtype=torch.int64, device=DEV) if counters is None else counters
    status = torch.zeros(1, dtype=torch.int32, device=DEV) if status is None else status
    n = _lib.workspace_bytes("mhmr_eval_match_workspace_bytes", P, G, B)
    ws = torch.empty(n // 8, dtype=torch.int64, device=DEV)
    _lib.check(L.mhmr_eval_match(dp.data_ptr() if P else None, int(pred.shape[1]) * 2, dpi.data_ptr() if P else None, P, dg.data_ptr() if G else None,
                                 dgi.data_ptr() if G else None, G, J, B, thresh, ws.data_ptr(), n, out["pair_pred"].data_ptr(), out["pair_gt"].data_ptr(),
                                 out["pred_fp"].data_ptr(), out["gt_miss"].data_ptr(), counters.data_ptr(), status.data_ptr(),
                                 torch.cuda.current_stream(DEV).cuda_stream), "mhmr_eval_match")
    res = dict(counters=counters.cpu().numpy(), status=int(status.cpu()[0]))
    for k, v in out.items():
        v = v.cpu().numpy()
        res[k], res[k + "_tail"] = v[:len(v) - PAD], v[len(v) - PAD:]
    return res


def assert_same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in ("pair_pred", "pair_gt", "pred_fp", "gt_miss"):
        assert (got[k + "_tail"] == SENTINEL).all(), (what, k)


def test_goldens_as_one_batch():
    """The reference's 12 cases as 12 images of one call (J = 17): pairs in the order found, flags and counters equal the goldens."""
    G = mo.GOLD
    pred, pimg, gt, gimg, B = mo.golden_batch()
    got = raw_match(pred, pimg, gt, gimg, B)
    assert got["status"] == 0
    want = dict(pair_pred=np.full(min(len(pred), len(gt)), -1, np.int32), pair_gt=np.full(min(len(pred), len(gt)), -1, np.int32),
                pred_fp=np.zeros(len(pred), np.int32), gt_miss=np.zeros(len(gt), np.int32), counters=np.zeros(4, np.int64))
    slot = p0 = g0 = 0
    for i in range(B):
        nP, nG, best = len(G[f"pred{i}"]), len(G[f"gt{i}"]), G[f"best{i}"].reshape(-1, 2)
        for k, (p, g) in enumerate(best):
            want["pair_pred"][slot + k], want["pair_gt"][slot + k] = p0 + p, g0 + g
        want["pred_fp"][p0 + G[f"fp{i}"].astype(np.int64)] = 1
        want["gt_miss"][g0 + G[f"miss{i}"].astype(np.int64)] = 1
        want["counters"] += (nG, len(G[f"miss{i}"]), len(G[f"fp{i}"]), len(best))
        slot, p0, g0 = slot + min(nP, nG), p0 + nP, g0 + nG
    assert_same(got, want, "goldens")


@pytest.mark.parametrize("name", sorted(mo.BATCHES))
def test_seeded_batches_decide_as_the_host_matching_per_image(name):
    """J = 55 read from rows of 127 joints and J = 127; images of 0x0, 0x3, 3x0, 1x1, 9x8 (72 pairs: more than a wave) and 17x16 persons
    (272 pairs: more than a workgroup's threads); a duplicated prediction (tied costs) and a distant one (the false-positive round);
    B = 1 and B = 6.  Twice: the same bits, and the counters accumulate."""
    pred, pimg, gt, gimg, B = mo.batch(name)
    want = mo.host_per_image(pred, pimg, gt, gimg, B)
    counters = torch.zeros(4, dtype=torch.int64, device=DEV)
    got = raw_match(pred, pimg, gt, gimg, B, counters=counters)
    assert got["status"] == 0
    assert_same(got, want, name)
    again = raw_match(pred, pimg, gt, gimg, B, counters=counters)
    assert_same(again, dict(want, counters=2 * want["counters"]), name + " (second call)")
    # the Python entry gives the same tensors
    st = ev.new_eval_state(DEV)
    pp, pg, fp, miss = ev.match_batched(torch.from_numpy(pred).to(DEV), torch.from_numpy(pimg).to(DEV), torch.from_numpy(gt).to(DEV),
                                        torch.from_numpy(gimg).to(DEV).long(), B, st)
    for k, v in zip(KEYS, (pp, pg, fp, miss, st[:4])):
        assert np.array_equal(v.cpu().numpy(), want[k]), (name, k)
    assert int(st[6]) == 0


def test_status_bits_are_sticky_and_leave_the_other_images_alone():
    pred, pimg, gt, gimg, B = mo.batch("j127_b6_dup_far")
    bad = pred.copy()
    bad[int(np.nonzero(pimg == 2)[0][0]), 5, 0] = np.nan
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = raw_match(bad, pimg, gt, gimg, B, status=status)
    assert got["status"] == mo.NONFINITE
    assert_same(got, mo.match_batch(bad, pimg, gt, gimg, B), "NaN keypoint in image 2")
    flat = gt.copy()
    flat[int(np.nonzero(gimg == 0)[0][0]), :, 0] = 7.0                          # a zero-width box in image 0
    got = raw_match(pred, pimg, flat, gimg, B, status=status)
    assert got["status"] == mo.NONFINITE | mo.DEGENERATE_BOX                    # sticky: the earlier bit stays
    assert_same(got, mo.match_batch(pred, pimg, flat, gimg, B), "zero-width box in image 0")
    got = raw_match(pred, pimg[::-1].copy(), gt, gimg, B)                       # descending image ids: nothing is matched
    assert got["status"] == mo.BAD_IMAGE_IDS and (got["pair_pred"] == -1).all() and not got["counters"].any() and not got["pred_fp"].any()
    # the Evaluator raises on either bit, from summary()
    for p, g in ((bad, gt), (pred, flat)):
        e = ev.Evaluator()
        t = lambda a: torch.from_numpy(a).to(DEV)
        G_, P_ = len(g), len(p)
        e.update_batched(dict(j2d=t(p), v3d=torch.zeros(P_, 14, 3, device=DEV), j3d=torch.zeros(P_, 4, 3, device=DEV)), t(pimg),
                         dict(j2d=t(g), v3d=torch.zeros(G_, 14, 3, device=DEV), transl_pelvis=torch.zeros(G_, 3, device=DEV), idx=(t(gimg).long(),),
                              scores=torch.zeros(B, 2, 2, device=DEV)))
        with pytest.raises(_lib.MhmrError, match="status"):
            e.summary()


@pytest.mark.parametrize("V", [14, 6890, 10475])
def test_indexed_metrics_carry_the_bits_of_gathered_copies(V):
    """-1 slots at the start, in the middle and at the end, a permuted index: per-pair values bit-equal to ``ev.mesh_errors`` on gathered
    copies, 0 in the empty slots; the device sums equal the fp64 sum of those values in slot order, bit for bit, and accumulate."""
    g = torch.Generator().manual_seed(V)
    P, G = 5, 6
    gt = (torch.randn(G, V, 3, generator=g) * 0.4 + torch.randn(G, 1, 3, generator=g) * 3).to(DEV)
    pred = (torch.randn(P, V, 3, generator=g) * 0.4 + torch.randn(P, 1, 3, generator=g) * 3).to(DEV)
    pc, gc = pred[:, 0].clone(), gt[:, 0].clone()
    ip = torch.tensor([-1, 3, 0, -1, 4, 1, -1], dtype=torch.int32, device=DEV)
    ig = torch.tensor([-1, 1, 5, -1, 0, 2, -1], dtype=torch.int32, device=DEV)
    ok = (ip >= 0).cpu()
    sums, n = torch.zeros(2, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    for centred in (True, False):
        sums.zero_(); n.zero_()
        c = (pc, gc) if centred else (None, None)
        pve, pa = ev.mesh_errors_indexed(pred, gt, ip, ig, *c, sums=sums, n_valid=n)
        sel_p, sel_g = ip[ok.to(DEV)].long(), ig[ok.to(DEV)].long()
        pve_r, pa_r = ev.mesh_errors(pred[sel_p], gt[sel_g], *(None if t is None else t[s] for t, s in zip(c, (sel_p, sel_g))))
        pve, pa = pve.cpu(), pa.cpu()
        assert torch.equal(pve[ok], pve_r.cpu()) and torch.equal(pa[ok], pa_r.cpu())
        assert float(pve[~ok].abs().max()) == 0.0 and float(pa[~ok].abs().max()) == 0.0 and float(pve_r.min()) > 0
        want = [0.0, 0.0]
        for m in range(len(ok)):
            if ok[m]:
                want[0] += float(pve[m])                       # python floats: fp64 additions in slot order
                want[1] += float(pa[m])
        assert sums.cpu().tolist() == want and int(n) == 4
        ev.mesh_errors_indexed(pred, gt, ip, ig, *c, sums=sums, n_valid=n)                       # added to, not overwritten
        assert sums.cpu().tolist() == [want[0] + want[0], want[1] + want[1]] and int(n) == 8
        pve2, pa2 = ev.mesh_errors_indexed(pred, gt, ip, ig, *c)                                  # without sums: the same values
        assert torch.equal(pve2.cpu(), pve) and torch.equal(pa2.cpu(), pa)


# ------------------------------------------------------------------------------------------------------------------ Evaluator level
def _fixture(smplx_data, mean_params):
    """The model and ground-truth builder of tests/test_gpu_train.py (ViT-S 224^2, depth 4) and one batch of four images with 2, 1, 0 and 3
    humans."""
    import gt_oracle as go
    import synthetic
    from multi_hmr_amd import BodyModel, GroundTruth, Model
    S, name = 224, "dinov2_vits14"
    sd = synthetic.make_state_dict(name, S, seed=42, depth_override=4, mean_params=mean_params)
    model = Model(backbone=name, img_size=S, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=4, precision="f16")
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    builder = GroundTruth(S, patch_size=14, smplx_neutral=BodyModel(smplx_data, "smplx", num_betas=11))
    x = torch.randn(4, 3, S, S, generator=torch.Generator().manual_seed(0))
    y = go.make_y("smplx", 51, S, [2, 1, 0, 3], depth=2.6)
    return model, builder, x, y


def _split(pred, img_id, gt, B):
    """Per image: (list of person dicts, ground-truth dict), as ``Evaluator.update`` takes them."""
    img_id, gimg = img_id.cpu(), gt["idx"][0].cpu()
    for b in range(B):
        ps, gs = torch.nonzero(img_id == b).reshape(-1).tolist(), torch.nonzero(gimg == b).reshape(-1).to(DEV)
        pelvis = pred["transl_pelvis"] if "transl_pelvis" in pred else pred["j3d"][:, :1]
        persons = [dict(v3d=pred["v3d"][i], j3d=pred["j3d"][i], j2d=pred["j2d"][i], transl_pelvis=pelvis[i]) for i in ps]
        yield persons, {k: gt[k][gs] for k in ("j2d", "v3d", "j3d", "transl_pelvis") if k in gt}


def _agree(a, b):
    assert set(a) == set(b)
    for k in a:
        if k in ("pve", "pa_pve", "mpjpe", "pa_mpjpe"):
            assert abs(a[k] - b[k]) <= 1e-12 * abs(b[k]), (k, a[k], b[k])           # the fp64 summation order
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def test_update_batched_equals_update_image_by_image(smplx_data, mean_params):
    import synthetic
    model, builder, x, y = _fixture(smplx_data, mean_params)
    gt = builder.prepare({k: v.to(DEV) for k, v in y.items()})
    B = x.shape[0]
    out = model(x.to(DEV), idx=gt["idx"], K=gt["K"], is_training=True)
    pred, ids = {k: out[k] for k in ("v3d", "j3d", "j2d")}, gt["idx"][0]
    pred["transl_pelvis"] = out["transl_pelvis"] if "transl_pelvis" in out else out["j3d"][:, :1]
    assert int(gt["j2d"].shape[0]) == 6
    s2s = ev.SparseRegressor(synthetic.make_smplx2smpl(0))
    gt_smpl = {k: v for k, v in gt.items() if k != "j3d"}
    gt_smpl["v3d"] = s2s(gt["v3d"]) + 0.01                                     # an SMPL ground truth (6890 vertices) for the 3DPW branch
    forms = (("smplx", gt, dict()), ("3dpw", gt_smpl, dict(smplx2smpl=s2s, h36m_regressor=synthetic.make_h36m_regressor(0))))
    for what, g, regs in forms:
        per_image, batched = ev.Evaluator(**regs), ev.Evaluator(**regs)
        for persons, g_b in _split(pred, ids, g, B):
            per_image.update(persons, g_b)
        batched.update_batched(pred, ids, g)                                    # (the first call uploads the regressors and index tables)
        a, b = batched.summary(), per_image.summary()
        print(what, a)
        assert a["count"] == 6 and a["matched"] > 0 and "mpjpe" in a
        _agree(a, b)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                                 # no copy to the host, no synchronisation
        try:
            batched.update_batched(pred, ids, g)
            batched.update_batched({}, ids[:0], g)                              # nobody detected: every ground truth is missed
        finally:
            torch.cuda.set_sync_debug_mode("default")
        for persons, g_b in _split(pred, ids, g, B):
            per_image.update(persons, g_b)
            per_image.update([], g_b)
        _agree(batched.summary(), per_image.summary())
        # the two kinds of update mix in one Evaluator
        mixed = ev.Evaluator(**regs)
        halves = list(_split(pred, ids, g, B))
        for persons, g_b in halves:
            mixed.update(persons, g_b)
        mixed.update_batched(pred, ids, g)
        m = mixed.summary()
        assert m["count"] == 12 and m["matched"] == 2 * a["matched"] and abs(m["pve"] - a["pve"]) <= 1e-12 * a["pve"]


def test_update_batched_pairs_inside_an_image_only():
    """Two images with the same layout of two persons, whose second image's predictions lie closer to the shared 2D layout: ``update`` on
    the whole batch pairs them with the FIRST image's ground truth (the reference's loop knows no images), ``update_batched`` does not."""
    g = torch.Generator().manual_seed(3)
    V, J = 50, 17
    centres = torch.tensor([[200.0, 300.0], [600.0, 320.0]])
    j2d = centres[:, None] + torch.randn(2, J, 2, generator=g) * 40
    gt_v = torch.randn(4, V, 3, generator=g) * 0.3                              # four different meshes
    gt = dict(j2d=torch.cat([j2d, j2d]).to(DEV), v3d=gt_v.to(DEV), j3d=gt_v[:, :J].contiguous().to(DEV), transl_pelvis=gt_v[:, :1].to(DEV),
              idx=(torch.tensor([0, 0, 1, 1], device=DEV),), scores=torch.zeros(2, 2, 2, device=DEV))
    noise = torch.randn(2, J, 2, generator=g)
    pred = dict(j2d=torch.cat([j2d + 3.0 * noise, j2d + 1.0 * noise]).to(DEV), v3d=(gt_v + 0.001).to(DEV), j3d=(gt_v[:, :J] + 0.001).to(DEV),
                transl_pelvis=(gt_v[:, :1] + 0.001).to(DEV))
    ids = torch.tensor([0, 0, 1, 1], dtype=torch.int32, device=DEV)
    persons = [{k: v[i] for k, v in pred.items()} for i in range(4)]
    whole, per_image, batched = ev.Evaluator(), ev.Evaluator(), ev.Evaluator()
    whole.update(persons, gt)
    for b in range(2):
        per_image.update(persons[2 * b:2 * b + 2], {k: gt[k][2 * b:2 * b + 2] for k in ("j2d", "v3d", "j3d", "transl_pelvis")})
    batched.update_batched(pred, ids, gt)
    w, p, a = whole.summary(), per_image.summary(), batched.summary()
    assert w["matched"] == p["matched"] == a["matched"] == 4
    assert p["pve"] < 1e-2 and w["pve"] > 10.0                                  # mm: its own mesh (a 1 mm shift, centred away) / another image's
    _agree(a, p)


def test_evaluate_dataset_batched_keeps_the_loss_and_the_per_image_metrics(smplx_data, mean_params):
    import loss_oracle as lo
    from multi_hmr_amd import Loss, evaluate_dataset
    model, builder, x, y = _fixture(smplx_data, mean_params)
    clone = lambda: [(x.clone(), {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in y.items()})]
    loss = Loss(lo.default_args())
    E = lo.DEFAULTS["start_2d_epoch"]
    plain = evaluate_dataset(model, clone(), builder, use_gt_idx=True, loss=loss, epoch=E)
    batched = evaluate_dataset(model, clone(), builder, use_gt_idx=True, loss=loss, epoch=E, batched=True)
    lk = sorted(k for k in plain if k.startswith("loss/"))
    assert len(lk) == 11 and lk == sorted(k for k in batched if k.startswith("loss/"))
    assert all(plain[k] == batched[k] for k in lk)                              # the same forward, the same loss
    assert set(plain) == set(batched) and batched["count"] == 6
    # image by image (batches of one) is what batched=True computes for the batch of four
    gt = builder.prepare({k: v.to(DEV) for k, v in clone()[0][1].items()})
    out = model(x.to(DEV), idx=gt["idx"], K=gt["K"], is_training=True)
    per_image = ev.Evaluator()
    for persons, g_b in _split(out, gt["idx"][0], gt, 4):
        per_image.update(persons, g_b)
    _agree({k: v for k, v in batched.items() if not k.startswith("loss/")}, per_image.summary())
    # the detector's path: return_batched=True
    s = evaluate_dataset(model, clone(), builder, det_thresh=0.3, batched=True)
    assert s["count"] == 6 and set(s) >= {"pve", "pa_pve", "precision", "recall", "f1_score", "matched"}
