"""-m gpu: the differentiable prediction decode (Model.decode_readout, csrc/heads_bwd.hip) against torch autograd
through the fp64 oracle of tests/heads_oracle.py on the CPU.

The scalar is sum(cotangent * output) over the fourteen outputs with seeded cotangents: N(0, 1) on the 3D and parameter outputs,
N(0, 1) / img_size on the 2D ones.  The gate is the project's rule (tests/test_gpu_groundtruth.py, tests/test_gpu_body_backward.py),
restated: the same oracle differentiated in fp32 on the CPU is the yardstick, and the kernel's maximum absolute error against fp64 may
be at most 4x the yardstick's, for g_readout and g_offset separately.  Every pair of figures is printed before anything is asserted
(run with -s).  Asserted first, as a condition and not a tolerance: the fp32 and the fp64 oracle made the same discrete choices for
every joint and person (quaternion branch, sign flip, series, clamp side) and every point of every person is in front of the camera
(the clamp case, whose clamped-to-zero person stands AT the camera, carries no 2D cotangent and is exempt from the second half).

The inputs of every case are built on the CPU by ``CASES[name]()``: the conditions can be checked without a device."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import gt_oracle as go
import heads_oracle as ho
import loss_oracle as lo
import synthetic
from multi_hmr_amd import BodyModel, GroundTruth, Loss, Model, _lib, loss_and_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
S, GRID, NB, V = 224, 16, 10, 10475
CAM0 = 318 + NB
NAME = "dinov2_vits14"
NO_2D = tuple(k for k in ho.KEYS if k not in ho.KEYS_2D)


@functools.lru_cache(maxsize=None)
def assets():
    """Built once, shared, never modified: the synthetic full-size body, the mean parameters, the two oracles, the read-out's init."""
    data, mean = synthetic.make_smplx_data(seed=0), synthetic.make_mean_params(seed=0)
    init = torch.cat([torch.eye(3)[:, :2].reshape(1, 3, 2).repeat(53, 1, 1).flatten(), torch.zeros(NB + 13)])
    init[:144] = torch.as_tensor(np.asarray(mean["pose"], dtype=np.float32)).flatten()
    init[318:318 + NB] = torch.as_tensor(np.asarray(mean["shape"], dtype=np.float32)).flatten()[:NB]
    return dict(data=data, mean=mean, init=init, o64=go.OracleBody(data, "smplx", NB, dtype=F64), o32=go.OracleBody(data, "smplx", NB, dtype=F32))


@functools.lru_cache(maxsize=None)
def model(center="head", nearness=True):
    a = assets()
    m = Model(backbone=NAME, img_size=S, smplx_data=a["data"], mean_params=a["mean"], backbone_depth=4, precision="f16", person_center=center,
              nearness=nearness)
    m.load_state_dict(synthetic.make_state_dict(NAME, S, seed=42, depth_override=4, mean_params=a["mean"]), strict=True)
    return m.to(DEV).eval()


# ---------------------------------------------------------------------------------------------------- cases (CPU)
def base_case(P, seed, use=ho.KEYS, nearness=True, center="head", general_K=False, B=None):
    B = B if B is not None else max(1, min(P, 2))
    readout, offset, idx, K = ho.make_inputs(assets()["init"], P, B, GRID, S, seed, nearness=nearness, general_K=general_K)
    return dict(readout=readout, offset=offset, idx=idx, K=K, cot=ho.make_cotangents(P, V, S, seed + 1, use=use, nb=NB), nearness=nearness,
                center=center, need_front=True)


def rot6d(axis, angle):
    """The first two columns of the rotation by ``angle`` about coordinate axis ``axis``, as the six read-out numbers (column 0, column 1)."""
    c, s = math.cos(angle), math.sin(angle)
    R = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    R = torch.tensor(R, dtype=torch.float64)
    return torch.cat([R[:, 0], R[:, 1]]).float()


def branch_case():
    """Joints 1 .. 6: rotations of +-(pi - 0.2) about x, y, z (the three non-trace branches, one direction of each with w < 0), scaled and
    slightly perturbed so that Gram-Schmidt has work to do; the other joints as in every case (they land in the trace branch or branch 0)."""
    c = base_case(1, seed=140)
    g = torch.Generator().manual_seed(141)
    for n, (axis, sign) in enumerate([(0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)]):
        j = 1 + n
        c["readout"][0, 6 * j:6 * j + 6] = rot6d(axis, sign * (math.pi - 0.2)) * (0.7 + 0.2 * n) + 0.01 * torch.randn(6, generator=g)
    return c


def identity_case():
    """Joint 3: the exact identity 6D (1,0,0, 0,1,0); joint 4: a rotation of 5e-4 rad about z (the series branch of the scale)."""
    c = base_case(1, seed=150)
    c["readout"][0, 18:24] = torch.tensor([1.0, 0, 0, 0, 1.0, 0])
    c["readout"][0, 24:30] = rot6d(2, 5e-4)
    return c


def clamp_case():
    """Without nearness: person 0 beyond 50 m (d = 60), person 1 behind the camera (d = -2, clamped to 0).  No 2D cotangents: the second
    person stands at the camera."""
    c = base_case(2, seed=160, use=NO_2D, nearness=False)
    scale = c["K"][c["idx"][0], 0, 0] / ho.focal_norm(S)
    c["readout"][:, CAM0] = torch.tensor([60.0, -2.0]) / scale
    c["need_front"] = False
    return c


CASES = {
    "P1": lambda: base_case(1, seed=101),
    "P3": lambda: base_case(3, seed=103),
    "no_center_P2": lambda: base_case(2, seed=112, center=None),
    "only_v2d": lambda: base_case(2, seed=121, use=("v2d",)),
    "only_j2d": lambda: base_case(2, seed=122, use=("j2d",)),
    "only_rotmat": lambda: base_case(2, seed=123, use=("rotmat",)),
    "only_transl": lambda: base_case(2, seed=124, use=("transl",)),
    "only_dist": lambda: base_case(2, seed=125, use=("dist",)),
    "branches": branch_case,
    "identity": identity_case,
    "clamp": clamp_case,
    "nearness_off": lambda: base_case(2, seed=170, nearness=False),
    "general_K": lambda: base_case(2, seed=180, general_K=True),
}


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(g_readout, g_offset, report) of the fp64 and of the fp32 oracle for a case: computed once per case."""
    c, a = CASES[name](), assets()
    kw = dict(nb=NB, img_size=S, nearness=c["nearness"], center=15 if c["center"] == "head" else None)
    return tuple(ho.grads(c["readout"], c["offset"], c["idx"], c["K"], a[o], c["cot"], dt, **kw) for o, dt in (("o64", F64), ("o32", F32)))


def precondition(name):
    c = CASES[name]()
    (_, _, r64), (_, _, r32) = oracle(name)
    assert ho.same_choices(r64, r32), (name, "the fp32 and fp64 oracles chose differently")
    if c["need_front"]:
        assert r64["in_front"] and r32["in_front"], (name, "a point behind the camera")
    return r64


# ---------------------------------------------------------------------------------------------------- device side
def kernel_grads(c, which=None):
    m = model(c["center"], c["nearness"])
    sel = slice(None) if which is None else which
    r = c["readout"][sel].to(DEV).requires_grad_()
    o = c["offset"][sel].to(DEV).requires_grad_()
    idx = tuple(i[sel] for i in c["idx"])
    out = m.decode_readout(r, o, idx, c["K"].to(DEV))
    assert set(out) == set(ho.KEYS)
    sum((out[k] * w[sel].to(DEV)).sum() for k, w in c["cot"].items()).backward()
    torch.cuda.synchronize()
    return r.grad, o.grad, out


def compare(name, got, ref64, ref32):
    res = []
    for n, x, r64, r32 in zip(("g_readout", "g_offset"), got, ref64, ref32):
        assert x is not None and tuple(x.shape) == tuple(r64.shape), (name, n)
        yard, err = go.max_err(r32, r64), go.max_err(x.cpu(), r64)
        print(f"{name} {n}: kernel {err:.3e}, fp32 autograd {yard:.3e}, gate {4 * yard:.3e}, ratio {err / yard if yard else float('nan'):.2f}, "
              f"largest entry {float(r64.abs().max()):.3e}")
        res.append((n, err, yard, bool(torch.isfinite(x).all())))
    for n, err, yard, finite in res:
        assert finite, (name, n)
        assert err <= 4 * yard, (name, n, err, yard)
    return res


def check(name):
    report = precondition(name)
    c = CASES[name]()
    (r64, o64, _), (r32, o32, _) = oracle(name)
    gr, go_, out = kernel_grads(c)
    compare(name, (gr, go_), (r64, o64), (r32, o32))
    assert bool((gr[:, CAM0 + 1:CAM0 + 3] == 0).all()), name           # the forward reads cam[0] only: exact zeros
    return gr, go_, out, report


@pytest.mark.parametrize("name", ["P1", "P3", "no_center_P2", "nearness_off", "general_K"])
def test_all_cotangents(name):
    check(name)


@pytest.mark.parametrize("name", ["only_v2d", "only_j2d", "only_rotmat", "only_transl", "only_dist"])
def test_each_cotangent_alone(name):
    """The absent cotangents reach the kernels as NULL (autograd hands None: the function does not materialise them)."""
    gr, go_, _, _ = check(name)
    if name in ("only_rotmat", "only_dist"):
        assert float(go_.abs().max()) == 0.0                           # nothing reaches the offsets
    if name == "only_rotmat":
        assert float(gr[:, 318:].abs().max()) == 0.0
    assert float(gr.abs().max()) > 0


def test_all_quaternion_branches_and_the_sign_flip():
    _, _, _, report = check("branches")
    print("branches", report["branch"].flatten().bincount(minlength=4).tolist(), "flips", int(report["flip"].sum()))
    assert set(report["branch"].flatten().tolist()) == {0, 1, 2, 3}
    assert bool(report["flip"][0, 1:7].any()) and int(report["flip"].sum()) >= 1


def test_identity_and_small_angle():
    gr, go_, _, report = check("identity")
    assert bool(report["small"][0, 3]) and bool(report["small"][0, 4]) and int(report["branch"][0, 3]) == 3
    assert bool(torch.isfinite(gr).all()) and bool(torch.isfinite(go_).all())
    # the closed form at the identity: g_R = g_rotmat + (c_x (E21 - E12) + c_y (E02 - E20) + c_z (E10 - E01)) / 2 through Gram-Schmidt,
    # with a cotangent on rotvec and rotmat only, so that c is the seeded cotangent itself
    c = dict(CASES["identity"]())
    c["cot"] = {k: v for k, v in c["cot"].items() if k in ("rotvec", "rotmat")}
    g2, _, _ = kernel_grads(c)
    cv, gR = c["cot"]["rotvec"][0, 3].double(), c["cot"]["rotmat"][0, 3].double().clone()
    gR[2, 1] += cv[0] / 2; gR[1, 2] -= cv[0] / 2; gR[0, 2] += cv[1] / 2; gR[2, 0] -= cv[1] / 2; gR[1, 0] += cv[2] / 2; gR[0, 1] -= cv[2] / 2
    six = torch.tensor([1.0, 0, 0, 0, 1.0, 0], dtype=F64, requires_grad=True)
    (ho.roma_ref.special_gramschmidt(six.reshape(2, 3).T) * gR).sum().backward()
    kw = dict(nb=NB, img_size=S, nearness=True, center=15)
    a = assets()
    r64 = ho.grads(c["readout"], c["offset"], c["idx"], c["K"], a["o64"], c["cot"], F64, **kw)[0]
    r32 = ho.grads(c["readout"], c["offset"], c["idx"], c["K"], a["o32"], c["cot"], F32, **kw)[0]
    yard, err = go.max_err(r32, r64), go.max_err(g2[0, 18:24].cpu(), six.grad)
    print(f"identity joint against the closed form: kernel {err:.3e}, fp32 autograd (whole g_readout) {yard:.3e}, gate {4 * yard:.3e}; "
          f"oracle fp64 against the closed form {go.max_err(r64[0, 18:24], six.grad):.3e}")
    assert err <= 4 * yard


def test_the_clamp_blocks_the_distance_gradient_on_both_sides():
    gr, _, out, report = check("clamp")
    assert report["clamp"].tolist() == [1, -1]
    assert out["dist"].flatten().tolist() == [50.0, 0.0]
    want = CASES["clamp"]()["cot"]["dist_postprocessed"].flatten()
    assert torch.equal(gr[:, CAM0].cpu(), want)                        # only the direct cotangent of dist_postprocessed is left


def test_every_element_is_written_and_cam_1_2_are_exact_zeros():
    """The C entry on sentinel-filled outputs, with the rotvec and transl cotangents only."""
    c = CASES["P3"]()
    P = 3
    dev = lambda t: t.to(DEV).contiguous()
    readout, offset, K = dev(c["readout"]), dev(c["offset"]), dev(c["K"])
    det = [dev(i.to(torch.int32)) for i in c["idx"]]
    g_rot, g_tr = dev(c["cot"]["rotvec"]), dev(c["cot"]["transl"])
    g_readout = torch.full((P, 318 + NB + 13), float("nan"), device=DEV)
    g_offset = torch.full((P, 2), float("nan"), device=DEV)
    d = _lib.HeadsDecodeBackwardDesc()
    d.P, d.nb, d.ldr, d.patch, d.nearness, d.fn = P, NB, readout.shape[1], 14, 1, float(ho.focal_norm(S))
    for n, t in (("readout", readout), ("offset", offset), ("K", K), ("det_b", det[0]), ("det_y", det[1]), ("det_x", det[2]), ("g_rotvec", g_rot),
                 ("g_transl", g_tr), ("g_readout", g_readout), ("g_offset", g_offset)):
        setattr(d, n, t.data_ptr())
    _lib.check(_lib.lib().mhmr_heads_decode_backward(C.byref(d), torch.cuda.current_stream().cuda_stream), "mhmr_heads_decode_backward")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g_readout).all()) and bool(torch.isfinite(g_offset).all())
    assert bool((g_readout[:, CAM0 + 1:CAM0 + 3] == 0).all())
    assert float(g_readout[:, 318:CAM0].abs().max()) == 0.0 and float(g_readout[:, CAM0 + 3:].abs().max()) == 0.0    # NULL shape / expression cotangents
    assert float(g_readout[:, :318].abs().max()) > 0 and float(g_readout[:, CAM0].abs().max()) > 0 and float(g_offset.abs().max()) > 0


def test_two_calls_and_two_batch_sizes_give_the_same_bits():
    c = CASES["P3"]()
    a, b = kernel_grads(c), kernel_grads(c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    one = kernel_grads(c, which=slice(0, 1))
    assert torch.equal(a[0][0], one[0][0]) and torch.equal(a[1][0], one[1][0])


def test_nobody():
    m = model()
    r, o = torch.zeros(0, 318 + NB + 13, device=DEV, requires_grad=True), torch.zeros(0, 2, device=DEV, requires_grad=True)
    z = torch.zeros(0, dtype=torch.long)
    out = m.decode_readout(r, o, (z, z, z), torch.eye(3, device=DEV)[None])
    assert tuple(out["v3d"].shape) == (0, V, 3) and tuple(out["j2d"].shape) == (0, 127, 2) and tuple(out["transl_pelvis"].shape) == (0, 1, 3)
    (out["v3d"].sum() + out["rotvec"].sum()).backward()
    assert r.grad is not None and r.grad.shape == r.shape and o.grad is not None


# ---------------------------------------------------------------------------------------------------- through the model
@functools.lru_cache(maxsize=None)
def small_forward():
    """The small model (ViT-S, 224^2, depth 4) on B = 2 images with persons [2, 1]: ground truth, the plain training-mode dict and the
    one with the read-out."""
    m, a = model(), assets()
    builder = GroundTruth(S, patch_size=14, smplx_neutral=BodyModel(a["data"], "smplx", num_betas=11))
    y = go.make_y("smplx", 51, S, [2, 1], depth=2.6)
    gt = builder.prepare({k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in y.items()})
    x = torch.randn(2, 3, S, S, generator=torch.Generator().manual_seed(0)).to(DEV)
    plain = m(x, idx=gt["idx"], K=gt["K"], is_training=True)
    out = m(x, idx=gt["idx"], K=gt["K"], is_training=True, return_readout=True)
    return m, gt, plain, out


def test_values_are_bit_equal_to_the_models_and_the_keyword_adds_one_key():
    m, gt, plain, out = small_forward()
    assert "readout" not in plain and list(out) == list(plain) + ["readout"]
    assert all(torch.equal(plain[k], out[k]) for k in plain)
    assert tuple(out["readout"].shape) == (3, 318 + NB + 13) and out["readout"].is_contiguous()
    dec = m.decode_readout(out["readout"], out["offset"], gt["idx"], gt["K"])
    shared = [k for k in dec if k in out]
    assert sorted(shared) == sorted(ho.KEYS)
    for k in shared:
        assert torch.equal(dec[k], out[k]), k
    assert not dec["v3d"].requires_grad


def test_through_the_loss_and_one_descent_step():
    """total.backward() fills the leaves with what decode_readout's backward makes of loss_and_grads' gradients, and a small step against the
    gradient lowers the loss by the first-order amount: epsilon is shrunk on the fp64 oracle (CPU) until the decrease of the same loss lies
    within 0.9 .. 1.1 of epsilon |g|^2, which must be at least 100x loss_oracle's rounding bound of the total; the device's decrease must
    then be positive and within 0.5 .. 1.5 of epsilon |g|^2.

    Figures: not recorded yet.  The one MI355X run this test has had stopped in the oracle call (a four-entry idx unpacked into three
    names, since mended in tests/heads_oracle.py) before any figure was printed."""
    m, gt, _, out = small_forward()
    args, epoch = lo.default_args(), lo.DEFAULTS["start_2d_epoch"]
    loss = Loss(args)

    def device_loss(readout, offset, backward):
        r, o = readout.clone().requires_grad_(backward), offset.clone().requires_grad_(backward)
        d = m.decode_readout(r, o, gt["idx"], gt["K"])
        total, _ = loss(dict(d, scores=out["scores"]), gt, epoch=epoch, img_size=S)
        if backward:
            total.backward()
        return total.detach(), r.grad, o.grad, d

    t0, g_r, g_o, d0 = device_loss(out["readout"], out["offset"], True)
    assert g_r is not None and g_o is not None and bool(torch.isfinite(g_r).all()) and bool(torch.isfinite(g_o).all())
    # the same gradients by hand: loss_and_grads on the detached dict, pushed through a second decode_readout
    y_hat = {k: v.detach() for k, v in dict(d0, scores=out["scores"]).items()}
    _, lg = loss_and_grads(y_hat, gt, epoch, S, args)
    r2, o2 = out["readout"].clone().requires_grad_(), out["offset"].clone().requires_grad_()
    d2 = m.decode_readout(r2, o2, gt["idx"], gt["K"])
    keys = [k for k in lg if k in d2]
    hand = torch.autograd.grad([d2[k] for k in keys], [r2, o2], grad_outputs=[lg[k] for k in keys])
    assert torch.equal(hand[0], g_r) and torch.equal(hand[1], g_o)

    # the step, sized on the fp64 oracle
    a = assets()
    idx = tuple(i.cpu() for i in gt["idx"])
    K, gnp = gt["K"].cpu(), {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in gt.items()}
    scores = out["scores"].cpu().numpy()

    def oracle_loss(readout, offset):
        o, _ = ho.decode(readout.cpu(), offset.cpu(), idx, K, a["o64"], nb=NB, img_size=S, nearness=True, center=15, dtype=F64)
        h = {k: v.detach().numpy() for k, v in o.items()}
        h["scores"] = scores
        res = lo.loss_ref(h, gnp, epoch, float(S), args)
        return res["values"]["total"], res["bound"]["total"]

    l0, bound = oracle_loss(out["readout"], out["offset"])
    g2 = float((g_r.double() ** 2).sum() + (g_o.double() ** 2).sum())
    eps, ratio = 1.0 / math.sqrt(g2), float("nan")                    # a step of length 1 in read-out space, then halved
    for _ in range(40):
        l1, _ = oracle_loss(out["readout"] - eps * g_r, out["offset"] - eps * g_o)
        ratio = (l0 - l1) / (eps * g2)
        print(f"epsilon {eps:.3e}: oracle decrease {l0 - l1:.6e}, first order {eps * g2:.6e}, ratio {ratio:.4f}")
        if 0.9 <= ratio <= 1.1:
            break
        eps /= 2
    assert 0.9 <= ratio <= 1.1, (eps, ratio)
    print(f"recorded epsilon {eps:.3e}; first-order decrease {eps * g2:.6e}; rounding bound of the total {bound:.3e}")
    assert eps * g2 >= 100 * bound, (eps * g2, bound)
    t1, _, _, _ = device_loss(out["readout"] - eps * g_r, out["offset"] - eps * g_o, False)
    dec = float(t0.double() - t1.double())
    print(f"device: total {float(t0):.9g} -> {float(t1):.9g}, decrease {dec:.6e}, ratio to first order {dec / (eps * g2):.4f}")
    assert dec > 0 and 0.5 <= dec / (eps * g2) <= 1.5
