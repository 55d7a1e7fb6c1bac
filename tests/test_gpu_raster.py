"""-m gpu: the differentiable rasteriser (csrc/raster_grad.hip, multi_hmr_amd/raster.py) against tests/raster_oracle.py.

Forward: ``depth`` equals ``render_maps(...).depth`` bit for bit, ``bary`` and ``attributes`` equal the numpy oracle bit for bit.
Backward: against fp64 autograd of the oracle, per tensor max |got - want| <= 2^-22 max |want| (the kernel's terms and sums are fp64 and
rounded to fp32 once, 2^-24 of an element; the gate is four times that at the largest magnitude), and a set of exact properties.
Images 29 x 37 and 48 x 64 (H x W): row segments end inside a wave and the heights are no multiple of the 4-row tile.

Measured on an MI355X (profiles/raster_tests.txt has every case): the worst max |got - want| / max |want| over all cases is
4.3e-8 for g_verts and 4.2e-8 for g_attr, i.e. 0.18 and 0.17 of the 2^-22 gate (both in scene b, three views, C = 16)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import maps_oracle as mo
import raster_oracle as rso
import render_exact as rx
import render_oracle as ro
import synthetic
from multi_hmr_amd import Model, _lib, demo, depth_loss, maps, raster, rasterize, render

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S0, S1 = (29, 37), (48, 64)                       # (H, W)
GATE = 2.0 ** -22
GUARD = 64


@functools.lru_cache(maxsize=None)
def scene(name, NV, size):
    """(verts, image_index, K, faces, Rt, cull) and the oracle's keys.  Built once, shared, never modified.
    a: the scene of tests/test_gpu_maps.py: B = 2 with image 1 empty, three overlapping icosphere(1) meshes (V = 42, F = 80) at depths
       3.0, 3.5 and 4.1 and a fourth whose image_index is out of range.
    b: a, and a fifth person that is a two-triangle quad behind the spheres filling most of the image (two more faces on four more
       vertices; every person's other faces are collapsed to a point and draw nothing).
    c: a with cull_back=False and sphere 1 mirrored (turned inside out: its faces have negative sigma).
    d: a with sphere 1's vertices NaN."""
    H, W = size
    sv, faces = ro.icosphere(1)
    centres = np.float32([[-0.35, 0.1, 3.0], [0.25, -0.15, 3.5], [0.0, 0.3, 4.1], [0.0, 0.0, 3.0]])
    unit = np.repeat(sv[None], 4, 0)
    if name == "c":
        unit[1, :, 0] *= -1
    verts = (unit * np.float32([0.75, 0.8, 0.9, 0.8])[:, None, None] + centres[:, None]).astype(np.float32)
    idx = np.array([0, 0, 0, 2], np.int32)
    if name == "d":
        verts[1] = np.nan
    if name == "b":
        faces = np.concatenate([faces, np.int32([[42, 44, 43], [42, 45, 44]])])
        quad = np.float32([[-3.2, -2.4, 6.0], [3.1, -2.3, 6.2], [3.2, 2.4, 5.8], [-3.1, 2.3, 6.1]])
        extra = np.repeat(centres[:, None], 4, 1)                                       # the spheres' quad faces: a point
        person = np.concatenate([np.repeat(quad[:1], 42, 0), quad])[None]               # the quad's sphere faces: a point
        verts = np.concatenate([np.concatenate([verts, extra], 1), person]).astype(np.float32)
        idx = np.array([0, 0, 0, 2, 0], np.int32)
    f = 0.9 * W
    K = np.float32([[[f, 0, W / 2 + 0.3], [0, f, H / 2 - 0.2], [0, 0, 1]], [[f * 1.1, 0, W / 2], [0, f * 1.1, H / 2], [0, 0, 1]]])
    Rt = None
    if NV > 1:
        o = demo.orbit_extrinsics(centres[:3].mean(0), "y", [0.0, 25.0, -40.0][:NV]).astype(np.float32)
        Rt = np.stack([o, o[::-1]])
    cull = name != "c"
    keys = mo.scene_keys(verts, idx, K, faces, H, W, Rt, cull=cull)
    return (verts, idx, K, faces, Rt, cull), keys


@functools.lru_cache(maxsize=None)
def reference(name, NV, size, C_, shared=False):
    """Attributes, the oracle's forward, cotangents with NaN at every pixel that is not owned, and fp64 autograd of the oracle."""
    (verts, idx, K, faces, Rt, cull), keys = scene(name, NV, size)
    g = np.random.default_rng(7 + C_)
    attr = g.standard_normal(((verts.shape[1], C_) if shared else verts.shape[:2] + (C_,))).astype(np.float32) if C_ else None
    fwd = rso.forward_np(verts, idx, K, faces, size[0], size[1], keys, Rt, attr, cull=cull)
    shape = keys.shape
    cot = dict(g_depth=g.standard_normal(shape).astype(np.float32), g_bary=g.standard_normal(shape + (3,)).astype(np.float32))
    if C_:
        cot["g_attr"] = g.standard_normal(shape + (C_,)).astype(np.float32)
    for v in cot.values():
        v[~fwd["owned"]] = np.nan
    gv, ga = rso.backward_autograd(verts, attr, fwd, K, faces, Rt, **cot)
    return attr, fwd, cot, gv, ga


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    a, b = (t.detach().cpu().numpy() if torch.is_tensor(t) else t for t in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def full(t, multi):
    """[B, H, W, ...] -> [B, 1, H, W, ...] when the call had one view."""
    return t if multi or t is None else t.unsqueeze(1)


def run(name, NV, size, attr, cot=None, want=raster.WANT, verts=None, **kw):
    """rasterize and, with cotangents, autograd through it: (Raster, g_verts, g_attr)."""
    (v0, idx, K, faces, Rt, cull), _ = scene(name, NV, size)
    vt = (dev(v0) if verts is None else verts).requires_grad_(True)
    at = None if attr is None else dev(attr).requires_grad_(True)
    multi = NV > 1
    r = rasterize(vt, idx, K, faces, size, Rt=(Rt if multi else (None if Rt is None else Rt[:, 0])), attributes=at, cull_back=cull, want=want, **kw)
    if cot is None:
        return r, None, None
    sq = (lambda t: t) if multi else (lambda t: t.squeeze(1))
    pairs = [(y, sq(dev(cot[k]))) for y, k in ((r.depth, "g_depth"), (r.bary, "g_bary"), (r.attributes, "g_attr")) if y is not None and k in cot]
    ins = [vt] + ([at] if at is not None and r.attributes is not None else [])
    grads = torch.autograd.grad([y for y, _ in pairs], ins, [g for _, g in pairs], allow_unused=True)
    return r, grads[0], grads[1] if len(grads) > 1 else None


class Guarded:
    """A device buffer with a guard row of sentinels behind (and in front of) its data."""

    def __init__(self, shape):
        self.n = int(np.prod(shape, dtype=np.int64))
        self.big = torch.full((self.n + 2 * GUARD,), -7.25, dtype=torch.float32, device=DEV)
        self.t = self.big[GUARD:GUARD + self.n].view(shape)
        self.t.fill_(float("nan"))

    def ok(self):
        return bool((self.big[:GUARD] == -7.25).all()) and bool((self.big[GUARD + self.n:] == -7.25).all())


def c_entry(name, NV, size, attr, keys, cot, per_pass=None, forward=False):
    """The C entries on guarded buffers: the forward's three outputs, or the backward's (g_verts, g_attr)."""
    (v0, idx, K, faces, Rt, cull), _ = scene(name, NV, size)
    P, V = v0.shape[:2]
    B, H, W = len(K), size[0], size[1]
    f_dev, off_dev, adj_dev = render._faces_on(faces, V, torch.device(DEV))
    keep = [dev(v0), dev(idx), dev(K), dev(Rt), dev(attr), keys.contiguous()] + [dev(c) for c in (cot or {}).values()]
    d = _lib.RasterDesc()
    d.B, d.NV, d.H, d.W, d.P, d.V, d.F, d.C = B, NV, H, W, P, V, len(faces), 0 if attr is None else attr.shape[-1]
    d.verts, d.vstride, d.faces, d.adj_off, d.adj = keep[0].data_ptr(), 3 * V, f_dev.data_ptr(), off_dev.data_ptr(), adj_dev.data_ptr()
    d.image_index, d.K, d.view_Rt, d.keys = keep[1].data_ptr(), keep[2].data_ptr(), _lib.ptr(keep[3]), keep[5].data_ptr()
    d.znear, d.cull_back = render.ZNEAR, int(cull)
    if attr is not None:
        d.attr, d.astride = keep[4].data_ptr(), 0 if attr.ndim == 2 else V * d.C
    stream = torch.cuda.current_stream().cuda_stream
    img = (B, NV, H, W)
    if forward:
        outs = [Guarded(img), Guarded(img + (3,)), Guarded(img + (d.C,)) if d.C else None]
        d.depth, d.bary, d.out_attr = outs[0].t.data_ptr(), outs[1].t.data_ptr(), outs[2].t.data_ptr() if d.C else None
        _lib.check(_lib.lib().mhmr_raster_interpolate(C.byref(d), stream), "mhmr_raster_interpolate")
        return outs
    names = list(cot)
    for field, k in (("g_depth", "g_depth"), ("g_bary", "g_bary"), ("g_out_attr", "g_attr")):
        if k in cot:
            setattr(d, field, keep[6 + names.index(k)].data_ptr())
    gv, ga = Guarded((P, V, 3)), Guarded((P, V, d.C)) if d.C else None
    d.g_verts, d.g_attr = gv.t.data_ptr(), ga.t.data_ptr() if d.C else None
    nbytes = _lib.workspace_bytes("mhmr_raster_workspace_bytes", C.byref(d), per_pass or P)
    ws = torch.empty(nbytes + 4 * GUARD, dtype=torch.uint8, device=DEV).fill_(0xA5)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    _lib.check(_lib.lib().mhmr_raster_backward(C.byref(d), stream), "mhmr_raster_backward")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), "the workspace's guard"
    return gv, ga


def untouched(fwd, faces, P, V):
    """[P, V] bool: the vertices no owned pixel touches (from the oracle alone)."""
    hit = np.zeros((P, V), bool)
    p, f = fwd["person"][fwd["owned"]], fwd["face"][fwd["owned"]]
    for c in range(3):
        hit[p, np.asarray(faces)[f, c]] = True
    return ~hit


CASES = [("a", 1, S0, 0), ("a", 1, S0, 1), ("a", 1, S0, 3), ("a", 1, S0, 16), ("a", 3, S0, 3), ("a", 1, S1, 3), ("a", 3, S1, 16),
         ("b", 1, S0, 0), ("b", 1, S0, 1), ("b", 1, S1, 3), ("b", 3, S0, 16), ("c", 1, S0, 3), ("c", 3, S1, 1), ("d", 1, S1, 3), ("d", 3, S0, 0)]


@pytest.mark.parametrize("name,NV,size,C_", CASES)
def test_forward_and_backward_equal_the_oracle(name, NV, size, C_):
    (verts, idx, K, faces, Rt, cull), keys = scene(name, NV, size)
    attr, fwd, cot, gv_want, ga_want = reference(name, NV, size, C_)
    P, V = verts.shape[:2]
    multi = NV > 1
    free = untouched(fwd, faces, P, V)
    if name == "b":                                                    # from the oracle alone: the workgroup path runs, a sphere vertex is untouched
        X = ro.camera_vertices(verts[4], *mo._view(mo.views_of(Rt, 2)[0], 0, 0))
        t = ro.setup(X, faces, K[0], size[0], size[1], ro.ZNEAR, cull)
        big = t["idx"][(t["x1"] - t["x0"] + 1) * (t["y1"] - t["y0"] + 1) > rx.SMALL_MAX]
        assert len(big) and any(((fwd["person"][0, 0] == 4) & (fwd["face"][0, 0] == f)).any() for f in big)
        assert free[:3, :42].any()
    assert fwd["owned"][0].any() and not fwd["owned"][1].any() and free[3].all() and (name != "d" or free[1].all())

    # ---- forward
    r, gv, ga = run(name, NV, size, attr, cot)
    assert np.array_equal(full(r.keys, multi).cpu().numpy().view(np.uint64), keys)
    m = maps.render_maps(dev(verts), idx, K, faces, size, Rt=(Rt if multi else (None if Rt is None else Rt[:, 0])), amodal=False, cull_back=cull)
    assert same_bits(r.depth, m.depth) and same_bits(full(r.depth, multi), fwd["depth"])
    assert same_bits(full(r.bary, multi), fwd["bary"]) and (C_ == 0 or same_bits(full(r.attributes, multi), fwd["attr"]))
    assert (C_ > 0) == (r.attributes is not None)
    own = torch.from_numpy(fwd["owned"]).to(DEV)
    assert torch.equal(full(r.mask, multi), own) and bool((full(r.depth, multi)[~own] == 0).all()) and bool((full(r.bary, multi)[~own] == 0).all())
    assert torch.equal(full(r.person, multi).long().cpu(), torch.from_numpy(fwd["person"])) and torch.equal(full(r.face, multi).long().cpu(), torch.from_numpy(fwd["face"]))
    outs = c_entry(name, NV, size, attr, full(r.keys, multi), None, forward=True)
    torch.cuda.synchronize()
    assert all(o is None or o.ok() for o in outs)
    assert same_bits(outs[0].t, fwd["depth"]) and same_bits(outs[1].t, fwd["bary"]) and (C_ == 0 or same_bits(outs[2].t, fwd["attr"]))

    # ---- backward: the C entry on guarded buffers, the same bits through autograd, twice, and one person per pass
    cg, ca = c_entry(name, NV, size, attr, full(r.keys, multi), cot)
    assert cg.ok() and (ca is None or ca.ok())
    assert same_bits(cg.t, gv) and (C_ == 0 or same_bits(ca.t, ga))
    _, gv2, ga2 = run(name, NV, size, attr, cot)
    assert same_bits(gv, gv2) and (C_ == 0 or same_bits(ga, ga2))
    og, oa = c_entry(name, NV, size, attr, full(r.keys, multi), cot, per_pass=1)
    assert og.ok() and same_bits(og.t, gv) and (C_ == 0 or same_bits(oa.t, ga))
    _, gv3, ga3 = run(name, NV, size, attr, cot, max_workspace_bytes=raster.pass_bytes(size, len(faces), NV, C_))
    assert same_bits(gv, gv3) and (C_ == 0 or same_bits(ga, ga3))
    # ---- against fp64 autograd of the oracle
    got = [("g_verts", gv.cpu().numpy().astype(np.float64), gv_want)] + ([("g_attr", ga.cpu().numpy().astype(np.float64), ga_want)] if C_ else [])
    for what, g, want in got:
        assert np.isfinite(g).all() and np.abs(want).max() > 0
        ratio = np.abs(g - want).max() / np.abs(want).max()
        print(f"raster {name} NV={NV} {size[0]}x{size[1]} C={C_} {what}: max|got-want|/max|want| = {ratio:.3e} = {ratio / GATE:.3f} of the gate")
        assert ratio <= GATE, (what, ratio)
        # zeros, not NaN: untouched vertices (hidden faces, the back of a sphere), the person of no image, the NaN person
        assert (g[free] == 0).all() and (want[free] == 0).all()


def test_each_cotangent_and_each_output_alone():
    name, NV, size, C_ = "b", 1, S0, 3
    (verts, idx, K, faces, Rt, cull), _ = scene(name, NV, size)
    attr, fwd, cot, _, _ = reference(name, NV, size, C_)
    everything, _, _ = run(name, NV, size, attr)
    for k in cot:
        one = {k: cot[k]}
        gv_want, ga_want = rso.backward_autograd(verts, attr, fwd, K, faces, Rt, **one)
        _, gv, ga = run(name, NV, size, attr, one)
        cg, ca = c_entry(name, NV, size, attr, everything.keys.unsqueeze(1), one)
        assert same_bits(cg.t, gv) and cg.ok() and ca.ok()
        assert np.abs(gv.cpu().numpy() - gv_want).max() <= GATE * np.abs(gv_want).max(), k
        if k == "g_attr":
            assert same_bits(ca.t, ga) and np.abs(ga.cpu().numpy() - ga_want).max() <= GATE * np.abs(ga_want).max()
        else:
            assert (ga_want == 0).all() and (ga is None or bool((ga == 0).all())) and bool((ca.t == 0).all())
    for w, field, ck in (("depth", "depth", "g_depth"), ("bary", "bary", "g_bary"), ("attributes", "attributes", "g_attr")):
        r, gv, ga = run(name, NV, size, attr, {ck: cot[ck]}, want=(w,))
        assert [f for f in ("depth", "bary", "attributes") if getattr(r, f) is not None] == [field]
        assert same_bits(getattr(r, field), getattr(everything, field)) and torch.equal(r.mask, everything.mask)
        gv_want, _ = rso.backward_autograd(verts, attr, fwd, K, faces, Rt, **{ck: cot[ck]})
        assert np.abs(gv.cpu().numpy() - gv_want).max() <= GATE * np.abs(gv_want).max(), w
    # attributes given to a call that does not want them are not read and get no gradient
    r, gv, ga = run(name, NV, size, attr, {"g_depth": cot["g_depth"]}, want=("depth", "bary"))
    assert r.attributes is None and ga is None


@pytest.mark.parametrize("C_", [1, 16])
def test_a_shared_table_gets_the_sum_over_the_persons(C_):
    name, NV, size = "a", 3, S0
    (verts, idx, K, faces, Rt, cull), _ = scene(name, NV, size)
    attr, fwd, cot, _, ga_want = reference(name, NV, size, C_, shared=True)
    assert attr.shape == (42, C_) and ga_want.shape == (42, C_)
    r, gv, ga = run(name, NV, size, attr, cot)
    assert same_bits(r.attributes, fwd["attr"]) and tuple(ga.shape) == (42, C_)
    assert np.abs(ga.cpu().numpy() - ga_want).max() <= GATE * np.abs(ga_want).max()
    per_person = np.ascontiguousarray(np.broadcast_to(attr, (4, 42, C_)))
    r2, gv2, ga2 = run(name, NV, size, per_person, cot)
    assert same_bits(r2.attributes, r.attributes) and same_bits(gv2, gv)
    total = ga2.double().sum(0)                                          # autograd's own sum over the expanded dimension, in fp32
    assert float((ga.double() - total).abs().max()) <= GATE * float(total.abs().max())
    _, ca = c_entry(name, NV, size, attr, r.keys, cot)                   # astride = 0 through the C entry: the per-person gradients
    assert ca.ok() and same_bits(ca.t, ga2)


def test_nobody_strided_vertices_and_given_keys():
    size = S0
    (verts, idx, K, faces, Rt, cull), keys = scene("a", 3, size)
    attr, fwd, cot, _, _ = reference("a", 3, size, 3)
    # P = 0
    for Rt0, shape in ((None, (2,) + size), (Rt, (2, 3) + size)):
        v = torch.zeros(0, 42, 3, device=DEV, requires_grad=True)
        a = torch.zeros(0, 42, 3, device=DEV, requires_grad=True)
        r = rasterize(v, [], K, faces, size, Rt=Rt0, attributes=a)
        assert tuple(r.depth.shape) == shape and tuple(r.bary.shape) == shape + (3,) and tuple(r.attributes.shape) == shape + (3,)
        assert not bool(r.mask.any()) and bool((r.person == -1).all()) and bool((r.depth == 0).all()) and bool((r.attributes == 0).all())
        (r.depth.sum() + r.bary.sum() + r.attributes.sum()).backward()
        assert tuple(v.grad.shape) == (0, 42, 3) and tuple(a.grad.shape) == (0, 42, 3)
    # a strided block (a person stride that is not 3 V) is read in place and gives the bits of its contiguous copy
    r, gv, ga = run("a", 3, size, attr, cot)
    block = torch.zeros(4, 42 + 5, 3, device=DEV)
    block[:, :42] = dev(verts)
    view = block[:, :42].detach()
    assert not view.is_contiguous()
    rs, gvs, gas = run("a", 3, size, attr, cot, verts=view)
    for f in ("depth", "bary", "attributes", "person", "face", "mask", "keys"):
        assert same_bits(getattr(rs, f), getattr(r, f)), f
    assert same_bits(gvs, gv) and same_bits(gas, ga)
    # the call's own keys handed back: nothing is rendered, the same bits
    rk, gvk, gak = run("a", 3, size, attr, cot, keys=r.keys)
    assert same_bits(rk.depth, r.depth) and same_bits(rk.bary, r.bary) and same_bits(rk.attributes, r.attributes) and same_bits(gvk, gv) and same_bits(gak, ga)
    # keys that belong to other vertices: the stale pixels are background, as the oracle has them, and nothing is NaN
    moved = verts + np.float32([0.06, 0.0, 0.0])
    fs = rso.forward_np(moved, idx, K, faces, size[0], size[1], keys, Rt, attr)
    assert (fs["owned"] != fwd["owned"]).any() and fs["owned"].any()
    vt = dev(moved).requires_grad_(True)
    rm = rasterize(vt, idx, K, faces, size, Rt=Rt, attributes=dev(attr), keys=r.keys)
    assert same_bits(rm.depth, fs["depth"]) and same_bits(rm.bary, fs["bary"]) and same_bits(rm.attributes, fs["attr"])
    g = {k: np.where(np.isnan(v), np.float32(1.0), v) for k, v in cot.items()}
    for k in g:
        g[k][~fs["owned"]] = np.nan
    gv_want, _ = rso.backward_autograd(moved, attr, fs, K, faces, Rt, **g)
    got, = torch.autograd.grad([rm.depth, rm.bary, rm.attributes], [vt], [dev(g["g_depth"]), dev(g["g_bary"]), dev(g["g_attr"])])
    assert np.abs(got.cpu().numpy() - gv_want).max() <= GATE * np.abs(gv_want).max()
    with pytest.raises(ValueError):
        rasterize(dev(verts), idx, K, faces, size, Rt=Rt, max_workspace_bytes=raster.pass_bytes(size, 80, 3) - 1)


# ---------------------------------------------------------------------------------------------------- through the model
S, NAME = 224, "dinov2_vits14"


@functools.lru_cache(maxsize=None)
def fixture():
    """The seeded depth-3 ViT-S at 224^2 of tests/test_gpu_fit.py on two images and the inference call that returns the read-out."""
    data, mean = synthetic.make_smplx_data(seed=0), synthetic.make_mean_params(seed=0)
    m = Model(backbone=NAME, img_size=S, smplx_data=data, mean_params=mean, backbone_depth=3, precision="f16")
    m.load_state_dict(synthetic.make_state_dict(NAME, S, seed=42, depth_override=3, mean_params=mean), strict=True)
    m = m.to(DEV).eval()
    x = torch.randn(2, 3, S, S, generator=torch.Generator().manual_seed(0)).to(DEV)
    K = synthetic.get_camera_K(S, 2).to(DEV)
    z = torch.zeros(1, dtype=torch.long)
    scores = m(x, idx=(z, z + 3, z + 5), K=K, is_training=True)["scores"]
    thr = float(scores.flatten().sort().values[-6]) - 1e-6
    rich, _ = m(x, K=K, det_thresh=thr, return_batched=True, return_readout=True)
    return m, K, rich


def test_depth_loss_alone_pulls_a_perturbed_distance_back():
    m, K, rich = fixture()
    faces = m.smpl_layer["neutral_10"].bm_x.faces
    r0, o0, idx = rich["readout"], rich["offset"], rich["idx"]
    P = int(r0.shape[0])
    assert 1 <= P <= 6
    with torch.no_grad():
        target = rasterize(m.decode_readout(r0, o0, idx, K)["v3d"], idx[0], K, faces, (S, S), want=("depth",))
    assert bool(target.mask.any())
    readout = r0.clone()
    readout[:, 318 + 10] += 0.05                                         # the distance column (nearness): every person a little off
    readout.requires_grad_(True)
    opt = torch.optim.Adam([readout], lr=0.01)
    losses = []
    for _ in range(12):
        opt.zero_grad()
        d = m.decode_readout(readout, o0, idx, K)
        ras = rasterize(d["v3d"], idx[0], K, faces, (S, S), want=("depth",))
        loss = depth_loss(ras, target.depth, valid=target.mask, sigma=0.1)
        loss.backward()
        assert bool(torch.isfinite(readout.grad).all())
        opt.step()
        losses.append(float(loss.detach()))
    print(f"depth_loss alone, {P} persons, Adam lr 0.01: {losses[0]:.4f} -> {losses[-1]:.4f} after {len(losses) - 1} steps")
    assert losses[0] > 0 and losses[-1] < losses[0]
