"""-m gpu: the training loss and its gradients on the device (csrc/loss.hip through multi_hmr_amd.loss) against the fp64 statement
of tests/loss_oracle.py.

Gates (derived in tests/loss_oracle.py, not tuned): every L1 term within 4 * 2^-24 * M_term of the fp64 value (M = the same reduction
over |u| + |u_hat|), bce within 4 * 2^-24 |bce|, total within the alpha-weighted sum; every gradient element within 4 * 2^-24
relative of the oracle's and exactly 0 where the oracle's is 0 -- nothing excluded.  Every figure is printed before it is asserted
(run with -s)."""
import functools
import os

import numpy as np
import pytest
import torch

import loss_oracle as lo
from multi_hmr_amd import Loss, _lib, loss_and_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 224.0
ARGS = lo.default_args()
E2D = lo.DEFAULTS["start_2d_epoch"]
SHAPES = [(1, 5, 3), (1, 10475, 127), (7, 10475, 127), (33, 10475, 127), (9, 67, 127)]


@functools.lru_cache(maxsize=None)
def case(P, V, J, seed=3, nb_hat=10, nb_gt=11, num_pos=None, epoch=E2D):
    """Inputs and oracle of one case: computed once, shared, never modified (the tests copy before they edit)."""
    h, y = lo.make_inputs(seed + 1000 * P + V, P, V, J, nb_hat=nb_hat, nb_gt=nb_gt, img_size=S, num_pos=num_pos)
    for d in (h, y):
        for a in d.values():
            a.setflags(write=False)
    return h, y, lo.loss_ref(h, y, epoch, S, ARGS)


def dev(d):
    return {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in d.items()}


def run(h, y, epoch=E2D, grad_total=None):
    dl, gr = loss_and_grads(h, y, epoch, S, ARGS, grad_total=grad_total)
    torch.cuda.synchronize()
    return {k: float(v) for k, v in dl.items()}, {k: v.cpu().numpy() for k, v in gr.items()}, {k: np.float32(v.cpu().numpy()) for k, v in dl.items()}


def check_values(vals, res, tag=""):
    for k in lo.KEYS:
        err, bound = abs(vals[k] - res["values"][k]), res["bound"][k]
        print(f"{tag}{k:7s} kernel {vals[k]:.9g} fp64 {res['values'][k]:.12g} |diff| {err:.3g} bound {bound:.3g}")
        assert err <= bound, (tag, k, err, bound)


def check_grads(grads, res, tag=""):
    assert set(grads) == set(res["grads"]), (sorted(grads), sorted(res["grads"]))
    for k, ref in res["grads"].items():
        got = grads[k].astype(np.float64)
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        nz = ref != 0
        rel = float(np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]))) if nz.any() else 0.0
        bad0 = int(np.count_nonzero(got[~nz]))
        print(f"{tag}grad {k:18s} {ref.size:8d} elements, {int((~nz).sum()):7d} zero; max rel err {rel:.3g} (gate {lo.BOUND_ULPS * lo.U:.3g}); non-zero where the oracle is 0: {bad0}")
        assert rel <= lo.BOUND_ULPS * lo.U and bad0 == 0, (tag, k, rel, bad0)


@pytest.mark.parametrize("P,V,J", SHAPES)
def test_values_and_gradients_against_the_fp64_statement(P, V, J):
    h, y, res = case(P, V, J)
    vals, grads, _ = run(dev(h), dev(y))
    check_values(vals, res)
    check_grads(grads, res)


def test_a_batch_without_persons_has_only_the_focal_term():
    h, y, res = case(0, 1, 1)
    vals, grads, _ = run(dev(h), dev(y))
    check_values(vals, res)
    check_grads(grads, res)
    assert all(vals[k] == 0 for k in lo.KEYS[2:]) and vals["bce"] > 0 and vals["total"] > 0 and set(grads) == {"scores"}


def test_no_positive_cell_is_decided_on_the_device():
    h, y, res = case(7, 67, 127, num_pos=0)
    assert res["counts"]["num_pos"] == 0
    vals, grads, _ = run(dev(h), dev(y))
    check_values(vals, res)
    check_grads(grads, res)


@pytest.mark.parametrize("nb_hat,nb_gt", [(10, 11), (11, 10)])
def test_shape_uses_the_common_columns(nb_hat, nb_gt):
    h, y, res = case(9, 67, 127, nb_hat=nb_hat, nb_gt=nb_gt)
    vals, grads, _ = run(dev(h), dev(y))
    check_values(vals, res)
    check_grads(grads, res)
    assert grads["shape"].shape == (9, nb_hat) and np.all(grads["shape"][:, 10:] == 0) and np.all(grads["shape"][:, :10] != 0)


@pytest.mark.parametrize("epoch", [E2D - 1, E2D])
def test_the_2d_terms_enter_at_start_2d_epoch(epoch):
    h, y, res = case(7, 10475, 127, epoch=epoch)
    vals, grads, _ = run(dev(h), dev(y), epoch=epoch)
    check_values(vals, res)
    check_grads(grads, res)
    on = epoch >= E2D
    assert vals["v2d"] > 0 and vals["j2d"] > 0                   # the values are reported either way (loss.py:100-113)
    assert bool(np.any(grads["v2d"] != 0)) == on and bool(np.any(grads["j2d"] != 0)) == on


def test_an_unaligned_prediction_slice_takes_the_scalar_path():
    h, y, res = case(7, 10475, 127)
    dh, dy = dev(h), dev(y)
    for k in ("v3d", "v2d", "rotmat"):
        buf = torch.empty(dh[k].numel() + 1, device=DEV)
        buf[1:] = dh[k].reshape(-1)
        dh[k] = buf[1:].view(dh[k].shape)
        assert dh[k].data_ptr() % 16 == 4 and dh[k].is_contiguous()
    vals, grads, _ = run(dh, dy)
    check_values(vals, res)
    check_grads(grads, res)


def test_two_calls_are_bit_equal():
    h, y, _ = case(33, 10475, 127)
    dh, dy = dev(h), dev(y)
    _, g1, v1 = run(dh, dy)
    _, g2, v2 = run(dh, dy)
    assert all(v1[k].tobytes() == v2[k].tobytes() for k in lo.KEYS)
    assert all(g1[k].tobytes() == g2[k].tobytes() for k in g1)


def test_a_person_has_the_same_gradient_rows_alone_and_in_a_batch_of_33():
    """An L1 gradient row is (sign pattern) x (one fp32 constant): the PATTERN of a person -- the row divided by its constant, exactly
    -1 / 0 / +1 -- is bit-equal alone and inside a batch of 33, and the constants differ by the 1/P scale: fl(c) against 33 fl(c / 33),
    one rounding each, i.e. within 2 * 2^-24.  The pelvis gradient (integer sign sums scaled once in fp64) likewise, after the factor P.
    (The 2D normaliser is the in-frame count of the whole batch, not P: pattern only.)"""
    h, y, _ = case(33, 10475, 127)
    p = 5
    one = lambda d: {k: (v if k == "scores" else v[p:p + 1]) for k, v in d.items()}
    _, gb, _ = run(dev(h), dev(y))
    _, g1, _ = run(dev(one(h)), dev(one(y)))
    for k in g1:
        if k == "scores":
            continue
        a, b = g1[k][0], gb[k][p]
        if k == "transl_pelvis":
            a64, b64 = a.astype(np.float64), b.astype(np.float64) * 33
            rel = float(np.max(np.abs(a64 - b64) / np.abs(a64)))
            print(f"{k:18s} alone vs 33 x batch row: max rel diff {rel:.3g}")
            assert rel <= 2 * lo.U
            continue
        ca, cb = np.abs(a).max(), np.abs(b).max()
        assert ca > 0 and cb > 0
        pa, pb = a / ca, b / cb
        assert set(np.unique(pa)) <= {-1.0, 0.0, 1.0} and pa.tobytes() == pb.tobytes(), k
        if k not in ("j2d", "v2d"):
            rel = abs(float(ca) - 33.0 * float(cb)) / float(ca)
            print(f"{k:18s} pattern bit-equal; constant alone {ca:.9g}, 33 x batch {33.0 * float(cb):.9g}, rel diff {rel:.3g}")
            assert rel <= 2 * lo.U, k


@pytest.mark.parametrize("key,bad,term", [("rotmat", np.inf, "rotmat"), ("v3d", np.nan, "v3d")])
def test_a_non_finite_term_is_dropped_with_all_its_gradients(key, bad, term):
    h, y, res = case(7, 10475, 127)
    dh, dy = dev(h), dev(y)
    clean_vals, clean_grads, clean_bits = run(dh, dy)
    dh[key] = dh[key].clone()
    dh[key].view(-1)[1234] = bad
    vals, grads, bits = run(dh, dy)
    print({k: vals[k] for k in lo.KEYS})
    assert vals[term] == 0.0 and np.all(grads[key] == 0)
    for k in lo.KEYS[1:]:
        if k != term:
            assert bits[k].tobytes() == clean_bits[k].tobytes(), k
    a = getattr(ARGS, "alpha_" + term)
    assert abs(vals["total"] - (clean_vals["total"] - a * clean_vals[term])) <= res["bound"]["total"] + 2 * lo.U * abs(clean_vals["total"])
    for k in grads:
        if k == key:
            continue
        if k == "transl_pelvis" and term == "v3d":       # the pelvis keeps the j3d part only
            hh = {n: np.array(v) for n, v in h.items()}
            hh["v3d"].reshape(-1)[1234] = np.nan
            with np.errstate(invalid="ignore"):
                want = lo.loss_ref(hh, y, E2D, S, ARGS)["grads"][k]
            assert np.all(np.abs(grads[k] - want) <= lo.BOUND_ULPS * lo.U * np.abs(want))
            continue
        assert grads[k].tobytes() == clean_grads[k].tobytes(), k


def test_autograd_fills_the_leaves_with_the_functional_gradients():
    h, y, _ = case(7, 10475, 127)
    dh, dy = dev(h), dev(y)
    dl_f, g_f = loss_and_grads(dh, dy, E2D, S, ARGS)
    leaves = {k: v.clone().requires_grad_(True) for k, v in dh.items()}
    total, dl = Loss(ARGS)(leaves, dy, epoch=E2D, img_size=S)
    assert total.dim() == 0 and total.is_cuda and total.requires_grad and list(dl) == list(lo.KEYS)
    assert all(v.dim() == 0 and v.is_cuda and not v.requires_grad for v in dl.values())
    total.backward()
    for k in lo.KEYS:
        assert torch.equal(dl[k], dl_f[k]), k
    assert torch.equal(total.detach(), dl_f["total"])
    for k, g in g_f.items():
        assert leaves[k].grad is not None and torch.equal(leaves[k].grad, g), k
    # an upstream factor reaches every gradient
    leaves2 = {k: v.clone().requires_grad_(True) for k, v in dh.items()}
    (Loss(ARGS)(leaves2, dy, epoch=E2D, img_size=S)[0] * 0.5).backward()
    _, g_half = loss_and_grads(dh, dy, E2D, S, ARGS, grad_total=torch.tensor(0.5, device=DEV))
    assert all(torch.equal(leaves2[k].grad, g_half[k]) for k in g_half)
    assert torch.equal(leaves2["v3d"].grad * 2, leaves["v3d"].grad)


def test_transl_pelvis_as_a_view_of_j3d_accumulates_into_joint_0():
    h, y, _ = case(7, 10475, 127)
    dh, dy = dev(h), dev(y)
    _, g_f = loss_and_grads(dh, dy, E2D, S, ARGS)
    leaves = {k: v.clone().requires_grad_(True) for k, v in dh.items() if k != "transl_pelvis"}
    y_hat = dict(leaves, transl_pelvis=leaves["j3d"][:, 0:1])                 # what Model returns
    total, _ = Loss(ARGS)(y_hat, dy, epoch=E2D, img_size=S)
    total.backward()
    want = g_f["j3d"].clone()
    want[:, 0:1] += g_f["transl_pelvis"]
    assert torch.equal(leaves["j3d"].grad, want)
    assert float(g_f["transl_pelvis"].abs().max()) > 0


def test_mismatched_ground_truth_meshes_raise():
    h, y, _ = case(9, 67, 127)
    dh, dy = dev(h), dev(y)
    with pytest.raises(_lib.MhmrError, match="v3d"):
        loss_and_grads(dh, dict(dy, v3d=dy["v3d"][:, :60]), E2D, S, ARGS)
    with pytest.raises(_lib.MhmrError, match="j3d"):
        loss_and_grads(dh, dict(dy, j3d=dy["j3d"][:, :24]), E2D, S, ARGS)


def test_evaluate_dataset_reports_the_loss_of_the_small_model(smplx_data, mean_params):
    """The model and batches of test_evaluate_dataset_with_gt_idx_runs_the_small_model_end_to_end: with loss= the summary gains
    finite loss/<key> means equal to a by-hand call per batch; without it the summary is the existing one, key for key."""
    import gt_oracle as go
    import synthetic
    from multi_hmr_amd import BodyModel, GroundTruth, Model, evaluate_dataset
    Sm, name = 224, "dinov2_vits14"
    sd = synthetic.make_state_dict(name, Sm, seed=42, depth_override=4, mean_params=mean_params)
    model = Model(backbone=name, img_size=Sm, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=4, precision="f16")
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    builder = GroundTruth(Sm, patch_size=14, smplx_neutral=BodyModel(smplx_data, "smplx", num_betas=11))
    g = torch.Generator().manual_seed(0)
    batches = [(torch.randn(2, 3, Sm, Sm, generator=g), go.make_y("smplx", 51 + i, Sm, counts, depth=2.6)) for i, counts in enumerate(([2, 1], [1, 2]))]
    clone = lambda: [(x.clone(), {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in y.items()}) for x, y in batches]
    loss = Loss(ARGS)
    plain = evaluate_dataset(model, clone(), builder, use_gt_idx=True)
    s = evaluate_dataset(model, clone(), builder, use_gt_idx=True, loss=loss, epoch=E2D)
    print({k: v for k, v in s.items() if k.startswith("loss/")})
    assert {k: v for k, v in s.items() if not k.startswith("loss/")} == plain
    assert sorted(k for k in s if k.startswith("loss/")) == sorted("loss/" + k for k in lo.KEYS)
    hand = np.zeros(11)
    for x, y in clone():
        gt = builder.prepare({k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in y.items()})
        with torch.no_grad():
            out = model(x.to(DEV), idx=gt["idx"], K=gt["K"], is_training=True)
            _, dl = loss(out, gt, epoch=E2D, img_size=Sm)
        hand += np.array([float(dl[k]) for k in lo.KEYS], dtype=np.float64) / 2
    for i, k in enumerate(lo.KEYS):
        assert np.isfinite(s["loss/" + k]) and s["loss/" + k] == hand[i], (k, s["loss/" + k], hand[i])
    assert s["loss/v3d"] > 0 and s["loss/bce"] > 0 and s["loss/total"] > 0
    with pytest.raises(_lib.MhmrError):
        evaluate_dataset(model, clone(), builder, use_gt_idx=False, loss=loss)


def test_the_reference_record_is_met_within_our_bound_plus_its_own_error():
    """tests/golden/loss_ref.npz holds the reference's own fp32 CPU result for one seeded case:
    |ours - reference| <= our bound + |reference - fp64|, the last computed here."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_ref.npz"))
    c = dict(zip(z["case_keys"].tolist(), z["case_values"].tolist()))
    i = {k: int(c[k]) for k in ("seed", "P", "V", "J", "B", "G", "nb_hat", "nb_gt", "epoch")}
    h, y = lo.make_inputs(i["seed"], i["P"], i["V"], i["J"], i["B"], i["G"], i["nb_hat"], i["nb_gt"], c["img_size"])
    res = lo.loss_ref(h, y, i["epoch"], c["img_size"], ARGS)
    dl, gr = loss_and_grads(dev(h), dev(y), i["epoch"], c["img_size"], ARGS)
    for k, ref in zip(lo.KEYS, z["values"].astype(np.float64)):
        ours, ref_err = float(dl[k]), abs(ref - res["values"][k])
        print(f"{k:7s} ours {ours:.9g} reference {ref:.9g} |diff| {abs(ours - ref):.3g} our bound {res['bound'][k]:.3g} + reference error {ref_err:.3g}")
        assert abs(ours - ref) <= res["bound"][k] + ref_err, k
    for k, g in gr.items():
        sl = z["gslice_" + k].astype(np.float64)
        ours, o64 = g.reshape(-1)[: sl.size].double().cpu().numpy(), res["grads"][k].reshape(-1)[: sl.size]
        tol = lo.BOUND_ULPS * lo.U * np.abs(o64) + np.abs(sl - o64)
        print(f"grad {k:18s} slice max |ours - reference| {np.abs(ours - sl).max():.3g}")
        assert np.all(np.abs(ours - sl) <= tol), k
