"""-m gpu: the body model's backward (mhmr_body_backward, BodyModel.differentiable) against torch autograd through the fp64 oracle of
tests/gt_oracle.py (OracleBody + perspective_projection on the CPU).

The scalar is sum(cotangent * output) with seeded cotangents: N(0, 1) on the 3D outputs, N(0, 1) / img_size on the 2D ones.  The
tolerance is the rule of tests/test_gpu_groundtruth.py, restated here: the same oracle differentiated in fp32 on the CPU is the
yardstick, and for each of g_pose, g_coef, g_transl the kernel's maximum absolute error against fp64 may be at most 4x the yardstick's.
Every pair of figures is printed before anything is asserted (run with -s to see them)."""
import numpy as np
import pytest
import torch

from multi_hmr_amd import BodyModel
import gt_oracle as go
import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
IMG = 448
OUTS = ("vertices", "joints", "v2d", "j2d")


def _asset(d, kind, nb, extra=None):
    return dict(kind=kind, nb=nb, model=BodyModel(d, kind, num_betas=nb), o64=go.OracleBody(d, kind, nb, dtype=F64, extra=extra),
                o32=go.OracleBody(d, kind, nb, dtype=F32, extra=extra))


@pytest.fixture(scope="module")
def small():
    """The synthetic SMPL-X with 1000 vertices (15 tiles of 64 + 40), picked vertices overridden through the data."""
    d = dict(synthetic.make_smplx_data(3, num_verts=1000, num_faces=2000))
    d["extra_joint_verts"] = np.arange(21) * 47 + 5
    return _asset(d, "smplx", 11, list(d["extra_joint_verts"]))


@pytest.fixture(scope="module")
def smpl():
    return _asset(synthetic.make_smpl_data(0, "male"), "smpl", 10)


def inputs(a, G, seed):
    g = torch.Generator().manual_seed(seed)
    pose = go.random_pose(g, G, a["model"].num_joints)
    coef = torch.randn(G, a["nb"], generator=g)
    if a["kind"] == "smplx":
        coef = torch.cat([coef, 0.5 * torch.randn(G, 10, generator=g)], 1)
    return pose, coef, go.random_transl(g, G), go.camera_K(IMG, G, g)


def cotangents(a, G, seed, use=OUTS):
    g = torch.Generator().manual_seed(seed)
    V, NJ = a["model"].num_vertices, a["model"].num_out_joints
    full = dict(vertices=torch.randn(G, V, 3, generator=g), joints=torch.randn(G, NJ, 3, generator=g),
                v2d=torch.randn(G, V, 2, generator=g) / IMG, j2d=torch.randn(G, NJ, 2, generator=g) / IMG)
    return {k: v for k, v in full.items() if k in use}


def keywords(a, pose, coef):
    G, nb = pose.shape[0], a["nb"]
    if a["kind"] == "smplx":
        return dict(global_orient=pose[:, 0], body_pose=pose[:, 1:22].reshape(G, 63), jaw_pose=pose[:, 22], leye_pose=pose[:, 23], reye_pose=pose[:, 24],
                    left_hand_pose=pose[:, 25:40].reshape(G, 45), right_hand_pose=pose[:, 40:55].reshape(G, 45), betas=coef[:, :nb],
                    expression=coef[:, nb:])
    return dict(global_orient=pose[:, 0], body_pose=pose[:, 1:].reshape(G, 69), betas=coef)


def kernel_grads(a, pose, coef, transl, K, cot):
    """Through BodyModel.differentiable with leaves on the device -> (g_pose, g_coef, g_transl or None), the outputs."""
    leaf = lambda t: None if t is None else t.to(DEV).requires_grad_()
    p, c, t = leaf(pose), leaf(coef), leaf(transl)
    out = a["model"].differentiable(transl=t, K=None if K is None else K.to(DEV), **keywords(a, p, c))
    sum(((getattr(out, k) * v.to(DEV)).sum() for k, v in cot.items())).backward()
    return (p.grad, c.grad, None if t is None else t.grad), out


def oracle_grads(o, dtype, pose, coef, transl, K, cot):
    leaf = lambda t: None if t is None else t.to(dtype).requires_grad_()
    p, c, t = leaf(pose), leaf(coef), leaf(transl)
    v, j = o(p, c, t)
    out = dict(vertices=v, joints=j)
    if K is not None:
        out["v2d"], out["j2d"] = go.perspective_projection(v, K.to(dtype)), go.perspective_projection(j, K.to(dtype))
    s = sum((out[k] * w.to(dtype)).sum() for k, w in cot.items())
    leaves = [x for x in (p, c, t) if x is not None]
    g = list(torch.autograd.grad(s, leaves, allow_unused=True))
    g = [torch.zeros_like(x) if y is None else y for x, y in zip(leaves, g)]
    return (g[0], g[1], g[2] if t is not None else None)


def compare(name, got, ref64, ref32):
    """The 4x rule on every gradient: all figures first, then the assertions -> {tensor: (kernel error, yardstick)}."""
    res = {}
    for n, x, r64, r32 in zip(("g_pose", "g_coef", "g_transl"), got, ref64, ref32):
        if r64 is None:
            assert x is None, (name, n)
            continue
        assert x is not None and tuple(x.shape) == tuple(r64.shape), (name, n)
        yard, err = go.max_err(r32, r64), go.max_err(x.cpu(), r64)
        print(f"{name} {n}: kernel {err:.3e}, fp32 autograd {yard:.3e}, gate {4 * yard:.3e}, ratio {err / yard if yard else float('nan'):.2f}, "
              f"largest entry {float(r64.abs().max()):.3e}")
        res[n] = (err, yard, bool(torch.isfinite(x).all()))
    for n, (err, yard, finite) in res.items():
        assert finite, (name, n)
        assert err <= 4 * yard, (name, n, err, yard)
    return res


def check(name, a, pose, coef, transl, K, cot):
    got, out = kernel_grads(a, pose, coef, transl, K, cot)
    compare(name, got, oracle_grads(a["o64"], F64, pose, coef, transl, K, cot), oracle_grads(a["o32"], F32, pose, coef, transl, K, cot))
    return got, out


@pytest.mark.parametrize("G", [1, 8, 9])
def test_small_smplx_all_four_cotangents(small, G):
    """V = 1000 is 15 tiles + 40 vertices; G = 9 crosses the group of 8."""
    pose, coef, transl, K = inputs(small, G, seed=300 + G)
    check(f"V=1000 G={G}", small, pose, coef, transl, K, cotangents(small, G, seed=400 + G))


def test_smpl_24_joints_no_landmarks(smpl):
    pose, coef, transl, K = inputs(smpl, 3, seed=31)
    check("smpl G=3", smpl, pose, coef, transl, K, cotangents(smpl, 3, seed=32))


def test_full_size_smplx(smplx_data):
    a = _asset(smplx_data, "smplx", 11)
    assert a["model"].num_vertices == 10475
    pose, coef, transl, K = inputs(a, 2, seed=41)
    check("V=10475 G=2", a, pose, coef, transl, K, cotangents(a, 2, seed=42))


def test_zero_rotations_are_an_ordinary_input(small):
    """One person with the whole pose zero, everyone's eye joints (23, 24) zero: sin(angle) / angle at angle = 1.7e-8."""
    pose, coef, transl, K = inputs(small, 3, seed=51)
    pose[0] = 0.0
    pose[:, 23:25] = 0.0
    got, _ = check("zero rotations", small, pose, coef, transl, K, cotangents(small, 3, seed=52))
    assert all(bool(torch.isfinite(x).all()) for x in got)
    assert float(got[0][0].abs().max()) > 0 and float(got[0][:, 23:25].abs().max()) > 0   # a zero rotation still has a gradient


@pytest.mark.parametrize("case", ["only_g_vertices", "only_g_j2d", "no_transl", "no_K"])
def test_partial_inputs_and_cotangents(small, case):
    pose, coef, transl, K = inputs(small, 3, seed=61)
    use = {"only_g_vertices": ("vertices",), "only_g_j2d": ("j2d",), "no_transl": OUTS, "no_K": ("vertices", "joints")}[case]
    if case == "no_transl":
        transl, K, use = None, None, ("vertices", "joints")       # without transl the body stands AT the camera: nothing to project
    if case == "no_K":
        K = None
    got, out = check(case, small, pose, coef, transl, K, cotangents(small, 3, seed=62, use=use))
    if case == "no_transl":
        assert got[2] is None
    if K is None:
        assert out.v2d is None and out.j2d is None


def test_only_betas_require_grad(small):
    pose, coef, transl, K = inputs(small, 3, seed=71)
    cot = cotangents(small, 3, seed=72)
    kw = {k: v.to(DEV) for k, v in keywords(small, pose, coef).items()}
    kw["betas"] = kw["betas"].clone().requires_grad_()
    tr = transl.to(DEV)
    out = small["model"].differentiable(transl=tr, K=K.to(DEV), **kw)
    sum(((getattr(out, k) * v.to(DEV)).sum() for k, v in cot.items())).backward()
    assert all(v.grad is None for k, v in kw.items() if k != "betas") and tr.grad is None
    r64, r32 = (oracle_grads(small[o], dt, pose, coef, transl, K, cot) for o, dt in (("o64", F64), ("o32", F32)))
    yard, err = go.max_err(r32[1][:, :11], r64[1][:, :11]), go.max_err(kw["betas"].grad.cpu(), r64[1][:, :11])
    print(f"only betas: kernel {err:.3e}, fp32 autograd {yard:.3e}, gate {4 * yard:.3e}")
    assert err <= 4 * yard


@pytest.mark.parametrize("which", ["landmark", "picked"])
def test_landmark_and_picked_vertex_routing(small, which):
    """A cotangent on ONE landmark (one picked-vertex joint): it reaches the vertices through the inverted list only, and transl directly."""
    m = small["model"]
    pose, coef, transl, K = inputs(small, 2, seed=81)
    j = m.num_joints + (len(m.extra_joint_verts) + 7 if which == "landmark" else 3)
    cj = torch.zeros(2, m.num_out_joints, 3)
    cj[:, j] = torch.randn(2, 3, generator=torch.Generator().manual_seed(82))
    got, _ = check(which, small, pose, coef, transl, None, dict(joints=cj))
    diff = (got[2].cpu() - cj[:, j]).abs()
    print(f"{which}: |g_transl - cotangent| max {float(diff.max()):.3e}")
    assert bool((diff <= cj[:, j].abs() * 2.0 ** -23).all())                 # one fp32 rounding
    assert float(got[0].abs().max()) > 0 and float(got[1].abs().max()) > 0


def test_two_calls_and_two_batch_sizes_give_the_same_bits(small):
    pose, coef, transl, K = inputs(small, 9, seed=91)
    cot = cotangents(small, 9, seed=92)
    a, _ = kernel_grads(small, pose, coef, transl, K, cot)
    b, _ = kernel_grads(small, pose, coef, transl, K, cot)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    one, _ = kernel_grads(small, pose[:1], coef[:1], transl[:1], K[:1], {k: v[:1] for k, v in cot.items()})
    assert all(torch.equal(x[0], y[0]) for x, y in zip(a, one))


def test_through_the_public_interface_with_a_torch_loss_on_top(small):
    """smplx keyword tensors that require grad, an L1 loss to a target mesh, .backward(); the forward equals __call__ bit for bit."""
    m = small["model"]
    G = 3
    pose, coef, transl, K = inputs(small, G, seed=101)
    target = small["o64"](*inputs(small, G, seed=102)[:3])[0].to(F32)
    names = ("global_orient", "body_pose", "left_hand_pose", "betas", "expression")
    kw = {k: v.to(DEV).clone() for k, v in keywords(small, pose, coef).items()}
    for k in names:
        kw[k].requires_grad_()
    tr = transl.to(DEV).requires_grad_()
    out = m.differentiable(transl=tr, K=K.to(DEV), **kw)
    plain = m(transl=tr.detach(), K=K.to(DEV), **{k: v.detach() for k, v in kw.items()})
    for k in OUTS:
        assert torch.equal(getattr(out, k), getattr(plain, k)), k
    assert out.vertices.requires_grad and not plain.vertices.requires_grad
    (out.vertices - target.to(DEV)).abs().mean().backward()
    assert all(kw[k].grad is not None for k in names) and tr.grad is not None and kw["jaw_pose"].grad is None

    def oracle(o, dt):
        p, c, t = (x.to(dt).requires_grad_() for x in (pose, coef, transl))
        ((o(p, c, t)[0] - target.to(dt)).abs().mean()).backward()
        return p.grad, c.grad, t.grad
    (p64, c64, t64), (p32, c32, t32) = oracle(small["o64"], F64), oracle(small["o32"], F32)
    cut = dict(global_orient=lambda p, c: p[:, 0], body_pose=lambda p, c: p[:, 1:22].reshape(G, 63), left_hand_pose=lambda p, c: p[:, 25:40].reshape(G, 45),
               betas=lambda p, c: c[:, :11], expression=lambda p, c: c[:, 11:])
    rows = [(k, kw[k].grad, f(p64, c64), f(p32, c32)) for k, f in cut.items()] + [("transl", tr.grad, t64, t32)]
    figs = []
    for k, got, r64, r32 in rows:
        yard, err = go.max_err(r32, r64), go.max_err(got.cpu(), r64)
        print(f"L1 loss {k}.grad: kernel {err:.3e}, fp32 autograd {yard:.3e}, gate {4 * yard:.3e}")
        figs.append((k, err, yard))
    for k, err, yard in figs:
        assert err <= 4 * yard, (k, err, yard)


def test_nobody(small):
    m = small["model"]
    z = lambda *s: torch.zeros(*s, device=DEV, requires_grad=True)
    go_, betas, tr = z(0, 3), z(0, 11), z(0, 3)
    out = m.differentiable(global_orient=go_, betas=betas, transl=tr, K=torch.zeros(0, 3, 3, device=DEV))
    assert tuple(out.vertices.shape) == (0, 1000, 3) and tuple(out.joints.shape) == (0, 127, 3)
    assert tuple(out.v2d.shape) == (0, 1000, 2) and tuple(out.j2d.shape) == (0, 127, 2) and out.vertices.is_cuda
    (out.vertices.sum() + out.j2d.sum()).backward()
    assert all(t.grad is not None and t.grad.shape == t.shape for t in (go_, betas, tr))


def test_a_malformed_parent_table_is_the_same_tree_in_both_directions():
    """csrc/body_shared.h body_parent: forward and backward read the parent of joint i clamped into [0, i - 1].  BodyModel refuses a table
    with parents[5] = 7 or parents[3] = -1, so it is planted in the packed constants that go to mhmr_body_forward / mhmr_body_backward:
    outputs and gradients must be bit-equal to the table that holds 4 and 0 there."""
    d = dict(synthetic.make_smplx_data(3, num_verts=1000, num_faces=2000))
    d["extra_joint_verts"] = np.arange(21) * 47 + 5
    G = 2
    a = dict(kind="smplx", nb=11)

    def run(p5, p3):
        m = BodyModel(d, "smplx", num_betas=11)
        a["model"] = m
        p = m._consts(torch.device(DEV))
        table = torch.from_numpy(m.parents).to(torch.int32)
        table[5], table[3] = p5, p3
        assert int(table.min()) >= -1 and int(table.max()) < m.num_joints
        p["parents"] = table.to(DEV)
        p["struct"].parents = p["parents"].data_ptr()
        pose, coef, transl, K = inputs(a, G, seed=111)
        grads, out = kernel_grads(a, pose, coef, transl, K, cotangents(a, G, seed=112))
        return [getattr(out, k).detach() for k in OUTS] + list(grads)

    bad, good = run(7, -1), run(4, 0)
    for n, x, y in zip(OUTS + ("g_pose", "g_coef", "g_transl"), bad, good):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0, n
        assert torch.equal(x, y), n
