"""-m gpu: the keypoint fit (mhmr_fit_keypoints, csrc/fit.hip; BodyModel.keypoint_model; KeypointFitter) on the
seeded synthetic SMPL-X, against tests/fit_oracle.py: ``o64`` the objective in fp64 on the CPU, ``y32`` the same code in fp32.

The gate is the project's rule: per tensor, the kernel's maximum absolute error against ``o64`` may be at most 4x ``y32``'s.  The loop uses the
same rule on the trace distance ``max_t |E[t] - E64[t]| / E64[0]``: over 8 seeds two legitimate fp32 orders stayed within 0.79 ... 1.32 of each
other there (profiles/fit_tests.txt), so the ratio is a stable statistic and section 31's fallback gate is not needed.  Every pair of figures
is printed before anything is asserted (run with -s).  The C entry runs on buffers with sentinels behind every output and the workspace, and
on NaN-filled outputs: every call of ``run`` checks both.

Figures: profiles/fit_tests.txt."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fit_oracle as fo
import gt_oracle as go
import heads_oracle as ho
import optim_oracle as oo
import parity
import synthetic
from multi_hmr_amd import COCO17, BodyModel, KeypointFitter, Model, _lib, fit, keypoints_by_name
from multi_hmr_amd.bodymodel import PERSON_GROUP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
S, GRID, NJ = 224, 16, 127
SENT, GUARD = -7.25, 64
LR, BETAS, EPS = 0.01, (0.9, 0.999), 1e-8
LAM = dict(pose=0.3, shape=0.2, depth=0.1, expression=0.4, loc=0.5)
ALL = fo.GROUPS
CHAIN12 = COCO17[5:]                         # the twelve COCO joints that are joints of the chain (shoulders ... ankles)


@functools.lru_cache(maxsize=None)
def assets(nb):
    """Built once per num_betas, shared, never modified."""
    data, mean = synthetic.make_smplx_data(seed=0), synthetic.make_mean_params(seed=0)
    init = torch.cat([torch.eye(3)[:, :2].reshape(1, 3, 2).repeat(53, 1, 1).flatten(), torch.zeros(nb + 13)])
    init[:144] = torch.as_tensor(np.asarray(mean["pose"], dtype=np.float32)).flatten()
    full = BodyModel(data, "smplx", num_betas=nb)
    return dict(data=data, mean=mean, init=init, o64=go.OracleBody(data, "smplx", nb, dtype=F64), o32=go.OracleBody(data, "smplx", nb, dtype=F32),
                full=full, km=full.keypoint_model())


@functools.lru_cache(maxsize=None)
def case(P, nb, robust, seed, given="all", optimize=ALL, lam="priors", sigma=20.0, moved=0.02):
    """Anchors (the recovery scene of fit_oracle), an iterate ``moved`` away from them, targets, weights.  ``given``: "all" (seeded weights
    in 0.3 ... 1), "ones" (every weight 1), or a tuple of joint names -- every other joint has weight 0 and a NaN target.  ``lam``:
    "priors" (LAM) or "none"."""
    a = assets(nb)
    sc = fo.scene(a["init"], P, 2, GRID, S, seed, a["o64"], nb=nb)
    g = torch.Generator().manual_seed(seed + 13)
    r0, o0 = sc["readout"], sc["offset"]
    r, o = r0 + moved * torch.randn(r0.shape, generator=g), o0 + moved * torch.randn(o0.shape, generator=g)
    kp, conf = sc["keypoints"].clone(), 0.3 + 0.7 * torch.rand(P, NJ, generator=g)
    if given == "ones":
        conf = torch.ones(P, NJ)
    elif given != "all":
        rows = fit.joint_indices(given)
        keep = torch.zeros(NJ, dtype=torch.bool)
        keep[rows] = True
        conf[:, ~keep] = 0.0
        kp[:, ~keep] = float("nan")
    return dict(P=P, nb=nb, robust=robust, readout0=r0, offset0=o0, readout=r, offset=o, idx=sc["idx"], K=sc["K"], keypoints=kp, confidence=conf,
                lam=dict(LAM) if lam == "priors" else {}, sigma=sigma, mask=fo.column_mask(nb, optimize))


def oracle_kw(c):
    return dict(nb=c["nb"], img_size=S, sigma=c["sigma"], robust=c["robust"], lam=c["lam"])


class Guarded:
    """A device buffer with sentinels in front of and behind its data."""

    def __init__(self, data=None, shape=None, fill=float("nan"), dtype=F32):
        shape = tuple(data.shape) if data is not None else tuple(shape)
        self.n = int(np.prod(shape, dtype=np.int64))
        self.big = torch.full((self.n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
        self.t = self.big[GUARD:GUARD + self.n].view(shape)
        if data is not None:
            self.t.copy_(data.to(dtype))
        else:
            self.t.fill_(fill)

    def ok(self):
        return bool((self.big[:GUARD] == SENT).all()) and bool((self.big[GUARD + self.n:] == SENT).all())


def run(c, steps=0, which=None, state=None, body="km", keypoints=None):
    """mhmr_fit_keypoints on case ``c`` (rows ``which``) -> CPU copies of every output.  ``state``: (exp_avg, exp_avg_sq, step0)."""
    sel = slice(None) if which is None else which
    a = assets(c["nb"])
    bm = a[body]
    nb, W = c["nb"], 318 + c["nb"] + 13
    r0, o0 = c["readout0"][sel], c["offset0"][sel]
    P = int(r0.shape[0])
    dev = torch.device(DEV)
    p, pb = bm._consts(dev), bm._bwd_consts(dev)
    L = _lib.lib()
    kp = (c["keypoints"] if keypoints is None else keypoints)[sel]
    m0, v0, step0 = state if state is not None else (torch.zeros(P, W + 2), torch.zeros(P, W + 2), 0)
    nbytes = _lib.workspace_bytes("mhmr_fit_keypoints_workspace_bytes", p["struct"], P)
    assert nbytes % 8 == 0
    inputs = dict(readout0=r0, offset0=o0, K=c["K"], keypoints=kp, confidence=c["confidence"][sel], mask=c["mask"])
    inputs = {k: v.to(DEV).contiguous() for k, v in inputs.items()}
    det = torch.stack([i[sel] for i in c["idx"][:3]]).to(torch.int32).to(DEV).contiguous() if P else torch.zeros(3, 0, dtype=torch.int32, device=DEV)
    before = {k: v.clone() for k, v in inputs.items()}
    out = dict(readout=Guarded(c["readout"][sel]), offset=Guarded(c["offset"][sel]), exp_avg=Guarded(m0), exp_avg_sq=Guarded(v0),
               objective=Guarded(shape=(steps + 1, P)), grad=Guarded(shape=(P, W + 2)), workspace=Guarded(shape=(nbytes // 8,), dtype=F64))
    d = _lib.FitDesc()
    d.c, d.bc = C.pointer(p["struct"]), C.pointer(pb["struct"])
    d.P, d.nb, d.ldr, d.patch, d.nearness, d.center_joint, d.fn = P, nb, W, 14, 1, 15, float(ho.focal_norm(S))
    for n, t in inputs.items():
        setattr(d, n, t.data_ptr())
    d.det_b, d.det_y, d.det_x = det[0].data_ptr(), det[1].data_ptr(), det[2].data_ptr()
    for n, gbuf in out.items():
        setattr(d, n, gbuf.t.data_ptr())
    d.workspace_bytes = nbytes
    d.sigma, d.robust = c["sigma"], _lib.FIT_ROBUST[c["robust"]]
    lam = c["lam"]
    d.lambda_pose, d.lambda_shape, d.lambda_depth = lam.get("pose", 0.0), lam.get("shape", 0.0), lam.get("depth", 0.0)
    d.lambda_expr, d.lambda_loc = lam.get("expression", 0.0), lam.get("loc", 0.0)
    d.steps, d.step0, d.lr, d.beta1, d.beta2, d.eps = steps, step0, LR, BETAS[0], BETAS[1], EPS
    rc = L.mhmr_fit_keypoints(C.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for n, gbuf in out.items():
        assert gbuf.ok(), ("sentinel overwritten around", n)
    for k, v in inputs.items():                                        # the caller's tensors keep their bits
        assert torch.equal(v.view(torch.int32), before[k].view(torch.int32)), k
    res = {n: gbuf.t.cpu().clone() for n, gbuf in out.items() if n != "workspace"}
    if P:
        assert bool(torch.isfinite(res["objective"]).all()) and bool(torch.isfinite(res["grad"]).all())       # every element written
    return res


def same_bits(a, b, keys=("readout", "offset", "exp_avg", "exp_avg_sq", "objective", "grad")):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in keys)


@functools.lru_cache(maxsize=None)
def oracle_value_and_grad(key):
    c = case(*key)
    a = assets(c["nb"])
    args = (c["readout"], c["offset"], c["readout0"], c["offset0"], c["idx"], c["K"])
    return tuple(fo.value_and_grad(*args, a[o], c["keypoints"], c["confidence"], c["mask"], dt, **oracle_kw(c)) for o, dt in (("o64", F64), ("o32", F32)))


def four_times(name, got, ref64, ref32):
    yard, err = go.max_err(ref32, ref64), go.max_err(got, ref64)
    print(f"{name}: kernel {err:.3e}, y32 {yard:.3e}, gate {4 * yard:.3e}, ratio {err / yard if yard else float('nan'):.2f}, "
          f"largest entry {float(ref64.abs().max()):.3e}")
    return name, err, yard


# ---------------------------------------------------------------------------------------------------- the keypoint model
def body_call(bm, pose, coef, g_joints):
    """mhmr_body_forward (no transl, no K) and mhmr_body_backward with the joint cotangent alone (g_vertices = NULL) -> vertices, joints,
    g_pose, g_coef."""
    dev, G = pose.device, int(pose.shape[0])
    p, pb = bm._consts(dev), bm._bwd_consts(dev)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    f = lambda *s: torch.full(s, float("nan"), device=dev)
    U, UJ = f(G, bm.num_vertices, 3), f(G, bm.num_out_joints, 3)
    ws_F, ws_A = f(-(-G // PERSON_GROUP), p["K"], PERSON_GROUP), f(G, bm.num_joints, 12)
    _lib.check(L.mhmr_body_forward(p["struct"], pose.data_ptr(), coef.data_ptr(), None, None, G, ws_F.data_ptr(), ws_A.data_ptr(), U.data_ptr(),
                                   UJ.data_ptr(), None, None, stream), "mhmr_body_forward")
    nbytes = _lib.workspace_bytes("mhmr_body_backward_workspace_bytes", p["struct"], G)
    ws = torch.empty(nbytes // 8, dtype=F64, device=dev)
    g_pose, g_coef = f(G, bm.num_joints, 3), f(G, p["nc"])
    b = _lib.BodyBackwardDesc()
    b.c, b.bc, b.G = C.pointer(p["struct"]), C.pointer(pb["struct"]), G
    for n, t in (("pose", pose), ("coef", coef), ("ws_F", ws_F), ("ws_A", ws_A), ("vertices", U), ("joints", UJ), ("g_joints", g_joints),
                 ("g_pose", g_pose), ("g_coef", g_coef), ("workspace", ws)):
        setattr(b, n, t.data_ptr())
    b.workspace_bytes = nbytes
    _lib.check(L.mhmr_body_backward(C.byref(b), stream), "mhmr_body_backward")
    torch.cuda.synchronize()
    return U.cpu(), UJ.cpu(), g_pose.cpu(), g_coef.cpu()


@pytest.mark.parametrize("G,nb", [(3, 10), (9, 11)])
def test_keypoint_model_against_the_full_model(G, nb):
    """Forward: bit-equal joints, and the kept vertices bit-equal to the full model's.  Backward (g_vertices = NULL, the same joint
    cotangents): the fp32 sum over the 64 lanes of a vertex tile depends on which vertices share a tile, i.e. on V, so the bits may differ;
    both models are held to the 4x rule against fp64 autograd."""
    a = assets(nb)
    g = torch.Generator().manual_seed(40 + G)
    pose, coef, gj = go.random_pose(g, G, 55), torch.randn(G, nb + 10, generator=g), torch.randn(G, NJ, 3, generator=g)
    dev = lambda t: t.to(DEV).contiguous()
    Uf, UJf, gpf, gcf = body_call(a["full"], dev(pose), dev(coef), dev(gj))
    Uk, UJk, gpk, gck = body_call(a["km"], dev(pose), dev(coef), dev(gj))
    assert torch.equal(UJk.view(torch.int32), UJf.view(torch.int32))
    assert torch.equal(Uk.view(torch.int32), Uf[:, a["km"].vertex_ids].view(torch.int32))
    print(f"backward bit-equal to the full model: g_pose {torch.equal(gpk, gpf)}, g_coef {torch.equal(gck, gcf)}; "
          f"max difference {go.max_err(gpk, gpf):.3e} / {go.max_err(gck, gcf):.3e}")
    ref = {}
    for o, dt in (("o64", F64), ("o32", F32)):
        ps, cf = pose.to(dt).requires_grad_(), coef.to(dt).requires_grad_()
        _, j = a[o](ps, cf, None)
        ref[o] = torch.autograd.grad((j * gj.to(dt)).sum(), [ps, cf])
    res = []
    for name, got, i in (("compact g_pose", gpk, 0), ("compact g_coef", gck, 1), ("full g_pose", gpf, 0), ("full g_coef", gcf, 1)):
        res.append(four_times(f"G={G} nb={nb} {name}", got, ref["o64"][i], ref["o32"][i]))
    for name, err, yard in res:
        assert err <= 4 * yard, (name, err, yard)


# ---------------------------------------------------------------------------------------------------- value and gradient
VG_CASES = [(1, 10, "gmof", 601), (3, 11, "l2", 603), (9, 10, "l2", 609), (9, 11, "gmof", 611)]


@pytest.mark.parametrize("key", VG_CASES, ids=lambda k: f"P{k[0]}-nb{k[1]}-{k[2]}")
def test_value_and_gradient_all_joints_given(key):
    c = case(*key)
    (E64, g64), (E32, g32) = oracle_value_and_grad(key)
    out = run(c, steps=0)
    res = [four_times(f"{key} objective", out["objective"][0], E64, E32), four_times(f"{key} grad", out["grad"], g64, g32)]
    W = 318 + c["nb"] + 13
    assert bool((out["grad"][:, 318 + c["nb"] + 1:318 + c["nb"] + 3] == 0).all())                    # cam[1:3]
    assert same_bits(out, dict(out, readout=c["readout"], offset=c["offset"]), keys=("readout", "offset"))      # steps = 0 moves nothing
    assert float(out["exp_avg"].abs().max()) == 0.0 and float(out["exp_avg_sq"].abs().max()) == 0.0
    assert float(out["grad"][:, :318].abs().min()) > 0 and float(out["grad"][:, W:].abs().min()) > 0
    for name, err, yard in res:
        assert err <= 4 * yard, (name, err, yard)
    if key[0] == 9:                                                    # the full model in the place of the keypoint model: the same objective
        full = run(c, steps=0, body="full")
        assert torch.equal(full["objective"], out["objective"])        # bit-equal joints -> bit-equal value
        four = four_times(f"{key} grad, full body model", full["grad"], g64, g32)
        assert four[1] <= 4 * four[2]


def test_nobody():
    c = case(3, 10, "gmof", 603)
    out = run(c, steps=2, which=slice(0, 0))
    assert tuple(out["objective"].shape) == (3, 0) and tuple(out["grad"].shape) == (0, 318 + 10 + 15)


def influencing(c, bm):
    """[53] bool per person-independent rule: may predicted rotation r move a given output joint?  A given chain joint hangs on its strict
    ancestors.  A given picked vertex or landmark hangs, through the pose correctives (dense), on every rotation."""
    conf = c["confidence"]
    given = (conf > 0).any(0)
    if bool(given[55:].any()) and float(np.abs(bm.posedirs).max()) > 0:
        return torch.ones(53, dtype=torch.bool)
    rows = torch.zeros(55, dtype=torch.bool)
    for j in range(55):
        if bool(given[j]) or j == 15:                                  # (every placed joint is taken relative to the head, joint 15)
            k = fo.PARENTS[j]
            while k >= 0:
                rows[k] = True
                k = fo.PARENTS[k]
    src = list(range(0, 22)) + list(range(25, 55)) + [22]             # pose row of predicted rotation r
    return rows[src]


@pytest.mark.parametrize("given", [COCO17, CHAIN12], ids=["coco17", "chain12"])
def test_joints_that_are_not_given_and_masked_columns_are_exact_zeros(given):
    """Only some joints given (the others: weight 0, NaN targets), pose and depth optimised, no priors.  Exact zeros: the masked columns (shape,
    expression, offset), cam[1:3], and the 6D columns of every rotation no given joint hangs on -- for COCO's face vertices that set is
    empty (pose correctives reach them from every joint); for the twelve chain joints it holds the head, jaw, wrists, ankles, feet and
    both hands (not the neck: it moves the head, the person centre every joint is taken relative to)."""
    key = (3, 10, "gmof", 620, given, ("pose", "depth"), "none")           # no priors: they would reach every column
    c = case(*key)
    a = assets(10)
    (E64, g64), (E32, g32) = oracle_value_and_grad(key)
    out = run(c, steps=0)
    res = [four_times(f"{len(given)} joints objective", out["objective"][0], E64, E32), four_times(f"{len(given)} joints grad", out["grad"], g64, g32)]
    g = out["grad"]
    assert float(g[:, 318:328].abs().max()) == 0.0 and float(g[:, 329:].abs().max()) == 0.0          # masked, and cam[1:3]
    moves = influencing(c, a["km"])
    still = [r for r in range(53) if not bool(moves[r])]
    print(f"{len(given)} joints given: {len(still)} rotations without a given joint behind them")
    assert (len(still) == 0) == (given is COCO17) and (given is COCO17 or len(still) >= 35)
    for r in still:
        assert float(g[:, 6 * r:6 * r + 6].abs().max()) == 0.0, r
        assert float(g64[:, 6 * r:6 * r + 6].abs().max()) == 0.0, r   # the oracle agrees that they are zeros
    for r in range(53):
        if bool(moves[r]):
            assert float(g[:, 6 * r:6 * r + 6].abs().max()) > 0.0, r
    assert float(g[:, 328].abs().min()) > 0.0
    for name, err, yard in res:
        assert err <= 4 * yard, (name, err, yard)
    # NaN targets behind weight 0 change no bit: the same call with ordinary numbers there
    other = run(c, steps=3, keypoints=torch.nan_to_num(c["keypoints"], nan=123.0))
    assert same_bits(run(c, steps=3), other)


# ---------------------------------------------------------------------------------------------------- the update
def test_one_step_is_torchs_single_tensor_adam_on_the_kernels_own_gradient():
    """steps = 1 from given moments at step count 3: new rows and moments against fp64 Adam (tests/optim_oracle.py) on the kernel's own
    gradient, gate: torch.optim.Adam (single tensor, fp32, CPU) from the same state, 4x -- the figures of tests/test_gpu_optim.py."""
    c = case(3, 11, "gmof", 603)
    W = 318 + 11 + 13
    g = torch.Generator().manual_seed(77)
    m0, v0 = 0.05 * torch.randn(3, W + 2, generator=g) * c["mask"], (0.05 * torch.randn(3, W + 2, generator=g)) ** 2 * c["mask"]
    grad = run(c, steps=0)["grad"]
    out = run(c, steps=1, state=(m0, v0, 3))
    x0 = torch.cat([c["readout"], c["offset"]], 1)
    ref, _ = oo.adam_step([dict(p=x0.numpy(), m=m0.numpy(), v=v0.numpy(), step=3)], [grad.numpy()], LR, BETAS, EPS)
    prm = torch.nn.Parameter(x0.clone())
    opt = torch.optim.Adam([prm], lr=LR, betas=BETAS, eps=EPS, foreach=False)
    prm.grad = grad.clone()
    opt.state[prm] = dict(step=torch.tensor(3.0), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    opt.step()
    got = dict(p=torch.cat([out["readout"], out["offset"]], 1), m=out["exp_avg"], v=out["exp_avg_sq"])
    tor = dict(p=prm.detach(), m=opt.state[prm]["exp_avg"], v=opt.state[prm]["exp_avg_sq"])
    rows = []
    for k in ("p", "m", "v"):
        r64 = torch.from_numpy(np.asarray(ref[0][k]))
        e_us, e_t = go.max_err(got[k], r64), go.max_err(tor[k], r64)
        print(f"adam {k}: kernel {e_us:.3e}, torch fp32 {e_t:.3e}, bit-equal to torch: {torch.equal(got[k], tor[k])}")
        rows.append((k, e_us, e_t))
    assert not torch.equal(got["p"], x0)
    off = c["mask"] == 0
    assert torch.equal(got["p"][:, off], x0[:, off]) and float(got["m"][:, off].abs().max()) == 0.0
    for k, e_us, e_t in rows:
        assert e_us <= 4.0 * e_t, (k, e_us, e_t)


# ---------------------------------------------------------------------------------------------------- the loop
LOOP = (3, 10, "l2", 500, "ones", ("pose", "shape", "depth", "loc"), "none", 1.0, 0.0)


@functools.lru_cache(maxsize=None)
def oracle_loop(steps):
    c, a = case(*LOOP), assets(10)
    args = (c["readout"], c["offset"], c["idx"], c["K"])
    tail = (c["keypoints"], c["confidence"], c["mask"], steps)
    kw = dict(lr=LR, betas=BETAS, eps=EPS, **oracle_kw(c))
    return fo.loop(*args, a["o64"], *tail, F64, **kw)[2], fo.loop(*args, a["o32"], *tail, F32, **kw)[2]


@pytest.mark.parametrize("steps", [5, 30])
def test_loop_recovers_the_perturbed_persons(steps):
    """The recovery scene: L2, zero priors, every joint given with weight 1, from the anchors themselves."""
    c = case(*LOOP)
    assert torch.equal(c["readout"], c["readout0"])
    t64, t32 = oracle_loop(steps)
    out = run(c, steps=steps)
    first = run(c, steps=0)
    trace = out["objective"]
    assert torch.equal(trace[0].view(torch.int32), first["objective"][0].view(torch.int32))
    d_k, d_y = fo.trace_distance(trace, t64), fo.trace_distance(t32, t64)
    print(f"steps {steps}: E[0] {trace[0].tolist()} -> E[last] {trace[-1].tolist()} (fp64: {t64[-1].tolist()})")
    print(f"steps {steps}: trace distance kernel {d_k:.3e}, y32 {d_y:.3e}, gate {4 * d_y:.3e}, ratio {d_k / d_y:.2f}")
    assert bool((trace[-1] < trace[0]).all())
    assert d_k <= 4 * d_y, (d_k, d_y)


# ---------------------------------------------------------------------------------------------------- exact properties
PROP = (9, 10, "gmof", 640, "all", ("pose", "shape", "loc"))


def test_two_calls_give_equal_bits_and_masked_columns_never_move():
    c = case(*PROP)
    a, b = run(c, steps=4), run(c, steps=4)
    assert same_bits(a, b)
    off = c["mask"] == 0
    x0, x1 = torch.cat([c["readout"], c["offset"]], 1), torch.cat([a["readout"], a["offset"]], 1)
    assert torch.equal(x1[:, off].view(torch.int32), x0[:, off].view(torch.int32)) and not torch.equal(x1[:, ~off], x0[:, ~off])
    assert float(a["exp_avg"][:, off].abs().max()) == 0.0 and float(a["grad"][:, off].abs().max()) == 0.0
    assert int(off.sum()) == 1 + 2 + 10                                # depth, cam[1:3], expression


@pytest.mark.parametrize("p", [0, 8])
def test_a_person_alone_equals_the_same_person_in_the_batch(p):
    """Nine persons cross the body kernels' group of eight: person 8 is alone in the second group of the batch and first in its own call."""
    c = case(*PROP)
    batch, alone = run(c, steps=3), run(c, steps=3, which=slice(p, p + 1))
    for k in ("readout", "offset", "exp_avg", "exp_avg_sq", "grad"):
        assert torch.equal(batch[k][p].view(torch.int32), alone[k][0].view(torch.int32)), k
    assert torch.equal(batch["objective"][:, p].view(torch.int32), alone["objective"][:, 0].view(torch.int32))


def test_thirty_steps_equal_ten_and_twenty_continued():
    c = case(3, 10, "gmof", 603)
    whole = run(c, steps=30)
    ten = run(c, steps=10)
    rest = run(dict(c, readout=ten["readout"], offset=ten["offset"]), steps=20, state=(ten["exp_avg"], ten["exp_avg_sq"], 10))
    assert same_bits(whole, rest, keys=("readout", "offset", "exp_avg", "exp_avg_sq", "grad"))
    assert torch.equal(whole["objective"][:10], ten["objective"][:10]) and torch.equal(whole["objective"][10:], rest["objective"])
    assert bool((whole["objective"][-1] < whole["objective"][0]).all())


# ---------------------------------------------------------------------------------------------------- through the model
NAME = "dinov2_vits14"


@functools.lru_cache(maxsize=None)
def fixture():
    """The depth-3 ViT-S at 224^2 on two images, a detection threshold that lets a few cells through, and the two inference calls."""
    a = assets(10)
    m = Model(backbone=NAME, img_size=S, smplx_data=a["data"], mean_params=a["mean"], backbone_depth=3, precision="f16")
    m.load_state_dict(synthetic.make_state_dict(NAME, S, seed=42, depth_override=3, mean_params=a["mean"]), strict=True)
    m = m.to(DEV).eval()
    x = torch.randn(2, 3, S, S, generator=torch.Generator().manual_seed(0)).to(DEV)
    K = synthetic.get_camera_K(S, 2).to(DEV)
    z = torch.zeros(1, dtype=torch.long)
    scores = m(x, idx=(z, z + 3, z + 5), K=K, is_training=True)["scores"]
    thr = float(scores.flatten().sort().values[-6]) - 1e-6
    plain, ids_p = m(x, K=K, det_thresh=thr, return_batched=True)
    rich, ids_r = m(x, K=K, det_thresh=thr, return_batched=True, return_readout=True)
    return m, x, K, thr, plain, ids_p, rich, ids_r


def test_inference_returns_the_rows_decode_readout_reproduces():
    m, x, K, thr, plain, ids_p, rich, ids_r = fixture()
    P = int(ids_p.shape[0])
    assert 1 <= P <= 6 and torch.equal(ids_p, ids_r)
    assert list(rich) == list(plain) + ["readout", "offset", "idx"] and list(plain) == list(m.PERSON_KEYS)
    for k in plain:                                                    # the old keys with the old bits
        assert torch.equal(plain[k], rich[k]), k
    assert tuple(rich["readout"].shape) == (P, 341) and rich["readout"].is_contiguous() and tuple(rich["offset"].shape) == (P, 2)
    assert len(rich["idx"]) == 3 and all(i.dtype == torch.long and tuple(i.shape) == (P,) for i in rich["idx"])
    assert torch.equal(rich["idx"][0].to(ids_r.dtype), ids_r)
    # a person list, and a call without return_batched, are what they were
    persons = m(x, K=K, det_thresh=thr, return_readout=True)
    assert isinstance(persons, list) and len(persons) == P and list(persons[0]) == list(m.PERSON_KEYS)
    dec = m.decode_readout(rich["readout"], rich["offset"], rich["idx"], K)
    for k in m.PERSON_KEYS:
        if k == "scores":
            continue
        e = parity.rel(dec[k].detach().cpu().numpy(), rich[k].cpu().numpy())
        print(f"decode_readout of the inference rows, {k}: rel-L2 {e:.3e}")
        assert e < parity.tolerance(k, "f16"), (k, e)


def test_keypoint_fitter_lowers_the_keypoint_error():
    m, x, K, thr, plain, ids_p, rich, ids_r = fixture()
    P = int(ids_p.shape[0])
    r, o, idx = rich["readout"], rich["offset"], rich["idx"]
    g = torch.Generator().manual_seed(5)
    rt, ot = r + 0.05 * torch.randn(r.shape, generator=g).to(DEV), o + 0.05 * torch.randn(o.shape, generator=g).to(DEV)
    target = m.decode_readout(rt, ot, idx, K)["j2d"].detach()
    rows = fit.joint_indices(COCO17)
    kp, conf = keypoints_by_name(COCO17, target[:, rows], torch.ones(P, 17, device=DEV))
    fitter = KeypointFitter(m, sigma=20.0, robust="gmof", weights=dict(pose=0.01, shape=0.01, expression=0.0), lr=0.01)
    r_in, o_in = r.clone(), o.clone()
    res = fitter.fit(r, o, idx, K, kp, conf, steps=50)
    assert torch.equal(r, r_in) and torch.equal(o, o_in) and res.readout.data_ptr() != r.data_ptr()
    assert tuple(res.objective.shape) == (51, P) and res.state["step"] == 50
    err = lambda rr, oo: float((m.decode_readout(rr, oo, idx, K)["j2d"][:, rows] - target[:, rows]).norm(dim=-1).mean())
    e0, e1 = err(r, o), err(res.readout, res.offset)
    print(f"mean COCO keypoint error {e0:.3f} px -> {e1:.3f} px after 50 steps; objective {res.objective[0].tolist()} -> {res.objective[-1].tolist()}")
    assert e1 < e0 and bool((res.objective[-1] < res.objective[0]).all())
    out = m.decode_readout(res.readout, res.offset, idx, K)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    assert torch.equal(res.readout[:, 331:], r[:, 331:])              # expression is not among the optimised groups
    # continuing through the state equals one longer run; the workspace is reused
    a = fitter.fit(r, o, idx, K, kp, conf, steps=4)
    b = fitter.fit(a.readout, a.offset, idx, K, kp, conf, steps=6, state=a.state)
    w = fitter.fit(r, o, idx, K, kp, conf, steps=10)
    assert torch.equal(b.readout, w.readout) and torch.equal(b.offset, w.offset) and torch.equal(b.objective, w.objective[4:])
    assert len(fitter._ws) == 1
    res0, grad = fitter.fit(r, o, idx, K, kp, conf, steps=0, return_grad=True)
    assert torch.equal(res0.readout, r) and torch.equal(res0.objective[0], res.objective[0]) and tuple(grad.shape) == (P, 343)
