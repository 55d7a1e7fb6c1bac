"""-m gpu: the distance maps and the silhouette term (csrc/silhouette.hip, multi_hmr_amd/silhouette.py) against tests/silhouette_oracle.py.

Distance maps: ``dist2`` and ``nearest`` equal the brute-force transform bit for bit, at every size, map kind and cap below.
Silhouette: ``counts``, the splat owners and the moments equal the oracle bit for bit; ``terms`` within 1e-12 relative; ``g_verts``
against fp64 autograd of the oracle, per tensor max |got - want| <= 2^-22 max |want| (tests/test_gpu_raster.py's gate: the kernel's
terms are fp64 and rounded to fp32 once, 2^-24 of an element; the gate is four times that at the largest magnitude).  Images 29 x 37
and 48 x 64 (H x W): rows end inside a wave, nothing is a multiple of a tile.

Measured on an MI355X (profiles/silhouette_tests.txt has every case): the worst max |got - want| / max |want| over all cases is
3.8e-8 for the outside gradient (scene a, 48 x 64) and 3.8e-8 for the uncovered gradient (scene e, 48 x 64), 0.16 of the 2^-22 gate; the
worst relative error of a term is 3.9e-16 (scene f, 29 x 37)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import render_exact as rx
import render_oracle as ro
import silhouette_oracle as so
import synthetic
from multi_hmr_amd import Model, _lib, assign_instance_masks, distance_transform, maps, render, silhouette, silhouette_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S0, S1 = (29, 37), (48, 64)                       # (H, W)
GATE = 2.0 ** -22
GUARD = 64
SIGMA, R = 4.0, 11


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    a, b = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))


class Guarded:
    """A device buffer with a guard row of sentinels behind (and in front of) its data."""

    def __init__(self, shape, dtype, fill):
        self.n = int(np.prod(shape, dtype=np.int64))
        self.big = torch.full((self.n + 2 * GUARD,), 77, dtype=dtype, device=DEV)
        self.t = self.big[GUARD:GUARD + self.n].view(shape)
        self.t.fill_(fill)

    def ok(self):
        return bool((self.big[:GUARD] == 77).all()) and bool((self.big[GUARD + self.n:] == 77).all())


# ------------------------------------------------------------------------------------------------------------------ distance maps
def c_transform(src, Rcap, want=(True, True)):
    """mhmr_distance_transform on guarded outputs and a guarded workspace: (dist2, nearest) numpy; an output that is not wanted is passed
    as NULL and comes back untouched (-5 everywhere)."""
    N, H, W = src.shape
    keep = dev(src.astype(np.uint8))
    d2, near = Guarded((N, H, W), torch.int32, -5), Guarded((N, H, W), torch.int32, -5)
    d = _lib.DistanceTransformDesc()
    d.N, d.H, d.W, d.max_dist, d.src = N, H, W, Rcap, keep.data_ptr()
    d.dist2, d.nearest = (d2.t.data_ptr() if want[0] else None), (near.t.data_ptr() if want[1] else None)
    nbytes = _lib.workspace_bytes("mhmr_distance_transform_workspace_bytes", C.byref(d))
    ws = torch.empty(nbytes + 4 * GUARD, dtype=torch.uint8, device=DEV).fill_(0xA5)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    _lib.check(_lib.lib().mhmr_distance_transform(C.byref(d), torch.cuda.current_stream().cuda_stream), "mhmr_distance_transform")
    torch.cuda.synchronize()
    assert d2.ok() and near.ok() and bool((ws[nbytes:] == 0xA5).all())
    return d2.t.cpu().numpy(), near.t.cpu().numpy()


@pytest.mark.parametrize("size", [(1, 1), (1, 37), (37, 1), (29, 37), (48, 64), (3, 300)])
def test_distance_transform_equals_brute_force_bit_for_bit(size):
    kinds = so.maps_of_every_kind(*size, seed=size[0] * 1000 + size[1])
    src = np.stack(list(kinds.values()))                               # eleven maps of different kinds in one call
    want = [so.transform_brute(m, 0) for m in src]
    for Rcap in (0, 1, 5):
        d2, near = c_transform(src, Rcap)
        d2b, nearb = c_transform(src, Rcap)
        assert same_bits(d2, d2b) and same_bits(near, nearb)
        for i, name in enumerate(kinds):
            wd, wn = so._cap(want[i][0].astype(np.int64), want[i][1], Rcap)
            assert np.array_equal(d2[i], wd) and np.array_equal(near[i], wn), (name, Rcap, size)
        pd, pn = distance_transform(dev(src.reshape((1,) + src.shape)), Rcap)                  # the Python surface, bool, [1, N, H, W]
        assert pd.dtype == torch.int32 and tuple(pd.shape) == (1,) + src.shape and same_bits(pd[0], d2) and same_bits(pn[0], near)
    # each output alone through the C entry (the other pointer NULL), and three maps of the eleven through the Python surface
    only_d, none_n = c_transform(src, 5, want=(True, False))
    none_d, only_n = c_transform(src, 5, want=(False, True))
    assert same_bits(only_d, d2) and same_bits(only_n, near) and (none_n == -5).all() and (none_d == -5).all()
    d = distance_transform(dev(src[[0, 6, 9]].astype(np.uint8)), 5)
    assert np.array_equal(d[0].cpu().numpy(), d2[[0, 6, 9]]) and np.array_equal(d[1].cpu().numpy(), near[[0, 6, 9]])
    assert tuple(distance_transform(torch.zeros((0, 4, 5), dtype=torch.bool, device=DEV))[0].shape) == (0, 4, 5)


# ------------------------------------------------------------------------------------------------------------------- the scenes
@functools.lru_cache(maxsize=None)
def scene(name, size):
    """(verts, image_index, K, faces, Rt, mask, allowed, robust): icosphere(1) meshes (V = 42, F = 80); masks are the oracle's own cover
    of the same spheres moved by a few pixels.  Built once, shared, never modified.
    a: two spheres in image 0 and one in image 1, allowed = a person's mask or another's of the same image, with extrinsics.
    b: one sphere cut by the image border, one vertex behind znear; allowed = mask; L2.
    c: two overlapping spheres with MODAL masks (each person's visible pixels), allowed = "others".
    c0: c with allowed = mask.
    d: one empty mask, one person of no image (image_index = B), one sphere with a NaN vertex.
    e: all-ones masks.
    f: a sphere, then a two-triangle quad person whose two faces have pixel boxes above SMALL_MAX (the workgroup pass of the cover; two
       more faces on four more vertices, every person's other faces collapsed to a point, as scene b of tests/test_gpu_raster.py: the
       quad person's 42 sphere vertices share one pixel), then a sphere in image 1; the quad's mask is moved by three pixels."""
    H, W = size
    sv, faces = ro.icosphere(1)
    f = 0.9 * W
    K = np.float32([[[f, 0, W / 2 + 0.3], [0, f, H / 2 - 0.2], [0, 0, 1]], [[f * 1.1, 0, W / 2], [0, f * 1.1, H / 2], [0, 0, 1]]])
    Rt = None
    robust = so.GMOF
    shift = np.float32([0.22, -0.1, 0.0])
    if name == "a":
        centres, radii, idx = np.float32([[-0.35, 0.1, 3.0], [0.45, -0.15, 3.5], [0.0, 0.05, 3.2]]), np.float32([0.5, 0.55, 0.6]), [0, 0, 1]
        Rt = np.float32([[[0.96, 0.0, 0.28, -0.85], [0.0, 1.0, 0.0, -0.05], [-0.28, 0.0, 0.96, 0.2]], [[1, 0, 0, 0.02], [0, 1, 0, 0], [0, 0, 1, 0]]])
    elif name == "b":
        centres, radii, idx, robust = np.float32([[-1.35, 0.6, 3.0]]), np.float32([0.7]), [0], so.L2
    elif name in ("c", "c0"):
        centres, radii, idx = np.float32([[-0.2, 0.05, 3.0], [0.25, -0.05, 3.6]]), np.float32([0.55, 0.7]), [0, 0]
    elif name == "d":
        centres, radii, idx = np.float32([[-0.4, 0.1, 3.0], [0.0, 0.0, 3.0], [0.4, -0.1, 3.3]]), np.float32([0.5, 0.5, 0.55]), [0, 2, 1]
    elif name == "f":
        centres, radii, idx = np.float32([[-0.3, 0.1, 3.0], [0.0, 0.0, 6.0], [0.2, 0.0, 3.3]]), np.float32([0.5, 1.0, 0.55]), [0, 0, 1]
    else:
        centres, radii, idx = np.float32([[-0.3, 0.1, 3.0], [0.3, 0.0, 3.4]]), np.float32([0.5, 0.6]), [0, 1]
    idx = np.array(idx, np.int32)
    verts = (sv[None] * radii[:, None, None] + centres[:, None]).astype(np.float32)
    if name == "f":
        faces = np.concatenate([faces, np.int32([[42, 44, 43], [42, 45, 44]])])
        quad = np.float32([[-2.0, -1.4, 6.0], [1.6, -1.3, 6.2], [1.7, 1.1, 5.8], [-1.9, 1.2, 6.1]])
        verts = np.concatenate([verts, np.repeat(centres[:, None], 4, 1)], 1)          # the spheres' quad faces: a point
        verts[1] = np.concatenate([np.repeat(quad[:1], 42, 0), quad])                  # the quad's sphere faces: a point
        shift = np.float32([[0.22, -0.1, 0.0], [0.6, -0.3, 0.0], [0.22, -0.1, 0.0]])[:, None]
    moved = verts + shift
    mask = so.cover(moved, idx, K, faces, H, W, Rt)
    if name in ("c", "c0"):                                            # modal: the front sphere hides part of the back one's segment
        import maps_oracle as mo
        keys = mo.scene_keys(moved, idx, K, faces, H, W)
        person = mo.maps(keys, len(verts), len(faces), idx)["person"][:, 0]
        mask = np.stack([person[idx[p]] == p for p in range(len(verts))])
        assert (so.cover(moved, idx, K, faces, H, W, Rt)[1] & ~mask[1]).any()
    if name == "b":
        verts[0, 3, 2] = 0.01
    if name == "d":
        mask[0] = False
        verts[2, 11] = np.nan
    if name == "e":
        mask[:] = True
    allowed = so.others_allowed(mask, idx, 2) if name in ("a", "c", "d", "e", "f") else mask
    return verts, idx, K, faces, Rt, mask, allowed, robust


@functools.lru_cache(maxsize=None)
def reference(name, size):
    verts, idx, K, faces, Rt, mask, allowed, robust = scene(name, size)
    fwd = so.forward(verts, idx, K, faces, mask, allowed, sigma=SIGMA, robust=robust, R=R, Rt=Rt)
    return fwd, so.backward_autograd(verts, idx, K, fwd, Rt)


def c_entry(name, size, per_pass=None, verts=None, vstride=None):
    """mhmr_silhouette on guarded buffers: terms, counts, g_verts, splat, moments (numpy)."""
    v0, idx, K, faces, Rt, mask, allowed, robust = scene(name, size)
    P, V = v0.shape[:2]
    H, W = size
    keep = [dev(v0) if verts is None else verts, dev(idx), dev(K), dev(Rt), dev(mask.astype(np.uint8)), dev(allowed.astype(np.uint8)),
            render._faces_on(faces, V, torch.device(DEV))[0]]
    outs = dict(terms=Guarded((P, 2), torch.float64, float("nan")), counts=Guarded((P, 2), torch.int32, -9),
                g_verts=Guarded((2, P, V, 3), torch.float32, float("nan")), splat=Guarded((P, H, W), torch.int32, -9),
                moments=Guarded((P, V, 4), torch.int64, -9))
    d = _lib.SilhouetteDesc()
    d.B, d.H, d.W, d.P, d.V, d.F = len(K), H, W, P, V, len(faces)
    d.verts, d.vstride, d.faces, d.image_index, d.K, d.Rt = keep[0].data_ptr(), vstride or 3 * V, keep[6].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), _lib.ptr(keep[3])
    d.znear, d.zfar, d.cull_back, d.mask, d.allowed = render.ZNEAR, render.ZFAR, 1, keep[4].data_ptr(), keep[5].data_ptr()
    d.sigma, d.robust, d.max_dist = SIGMA, robust, R
    for k, g in outs.items():
        setattr(d, k, g.t.data_ptr())
    nbytes = _lib.workspace_bytes("mhmr_silhouette_workspace_bytes", C.byref(d), per_pass or P)
    ws = torch.empty(nbytes + 4 * GUARD, dtype=torch.uint8, device=DEV).fill_(0xA5)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    _lib.check(_lib.lib().mhmr_silhouette(C.byref(d), torch.cuda.current_stream().cuda_stream), "mhmr_silhouette")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), "the workspace's guard"
    assert all(g.ok() for g in outs.values())
    return {k: g.t.cpu().numpy() for k, g in outs.items()}


def through_autograd(name, size, verts=None, **kw):
    """silhouette_loss and the gradient of each term's sum: (Silhouette, g [2, P, V, 3] numpy)."""
    v0, idx, K, faces, Rt, mask, allowed, robust = scene(name, size)
    vt = (dev(v0) if verts is None else verts).requires_grad_(True)
    ignore = "others" if name in ("a", "c", "d", "e", "f") else None
    s = silhouette_loss(vt, idx, K, faces, dev(mask), Rt=Rt, ignore=ignore, sigma=SIGMA, robust=("gmof" if robust == so.GMOF else "l2"), max_dist=R,
                        weights=(0.5, 2.0), **kw)
    g = [torch.autograd.grad(t.sum(), vt, retain_graph=True)[0].cpu().numpy() for t in (s.outside, s.uncovered)]
    return s, np.stack(g), vt


CASES = [(n, s) for n in ("a", "b", "c", "c0", "d", "e", "f") for s in (S0, S1)]


@pytest.mark.parametrize("name,size", CASES)
def test_silhouette_equals_the_oracle(name, size):
    verts, idx, K, faces, Rt, mask, allowed, robust = scene(name, size)
    fwd, g_want = reference(name, size)
    P, V = verts.shape[:2]
    # ---- from the oracle alone: the scene shows what it is there for
    if name in ("a", "b", "c", "c0", "f"):
        assert (fwd["counts"] > 0).all() and (fwd["terms"] > 0).all()
    if name == "f":                                                    # the workgroup pass of the cover runs, for the second person of the pass
        t = ro.setup(ro.camera_vertices(verts[1]), faces, K[0], size[0], size[1], ro.ZNEAR, True)
        boxes = (t["x1"] - t["x0"] + 1) * (t["y1"] - t["y0"] + 1)
        assert sorted(t["idx"][boxes > rx.SMALL_MAX]) == [80, 81] and fwd["cover"][1].sum() > 2 * rx.SMALL_MAX
        assert (fwd["moments"][1, 0, 0] > 0 or fwd["moments"][1, 42:, 0].sum() > 0) and (fwd["splat"][1] == 0).sum() == 1
    if name == "b":
        ok, u, v, _, _ = so.project(verts[0], K, 0, Rt, *size)
        assert 5 < ok.sum() < V - 5 and not ok[3] and (~fwd["cover"][0][:, 0]).any() and fwd["cover"][0][:, 0].any()      # cut by the left border
    if name == "c":
        f0, _ = reference("c0", size)
        assert fwd["counts"][1, 0] < f0["counts"][1, 0] and np.array_equal(fwd["counts"][:, 1], f0["counts"][:, 1])          # "others" forgives the hidden part
    if name == "d":                                                    # an empty mask: every vertex is far outside, on the flat cap
        assert fwd["counts"][0, 0] == fwd["ok"][0].sum() > 0 and fwd["counts"][0, 1] == 0 and fwd["terms"][0, 1] == 0 and fwd["terms"][0, 0] > 0
        assert (g_want[:, 0] == 0).all()
        assert (fwd["counts"][1] == 0).all() and (fwd["terms"][1] == 0).all() and not fwd["ok"][2, 11] and (fwd["counts"][2] > 0).all()
    if name == "e":
        assert (fwd["terms"][:, 0] == 0).all() and (fwd["counts"][:, 0] == 0).all() and (g_want[0] == 0).all()

    # ---- the C entry on guarded buffers: integers bit for bit, the terms to 1e-12
    got = c_entry(name, size)
    assert np.array_equal(got["counts"], fwd["counts"]) and np.array_equal(got["splat"], fwd["splat"]) and np.array_equal(got["moments"], fwd["moments"])
    worst_t = 0.0
    for p in range(P):
        for k in range(2):
            want = fwd["terms"][p, k]
            assert np.isfinite(got["terms"][p, k]) and abs(got["terms"][p, k] - want) <= 1e-12 * abs(want), (p, k, got["terms"][p, k], want)
            worst_t = max(worst_t, abs(got["terms"][p, k] - want) / want if want else 0.0)
    if name == "e":
        assert (got["terms"][:, 0] == 0).all() and (got["g_verts"][0] == 0).all()                                             # exactly
    # ---- twice, one person per pass, and through autograd: the same bits
    again, single = c_entry(name, size), c_entry(name, size, per_pass=1)
    s, g_auto, _ = through_autograd(name, size)
    s1, g_auto1, _ = through_autograd(name, size, max_workspace_bytes=silhouette.pass_bytes(size, V, len(faces)))
    for k in got:
        assert same_bits(got[k], again[k]) and same_bits(got[k], single[k]), k
    assert same_bits(g_auto, got["g_verts"]) and same_bits(g_auto1, got["g_verts"])
    t32 = torch.from_numpy(got["terms"]).float()
    assert same_bits(s.outside, t32[:, 0]) and same_bits(s.uncovered, t32[:, 1]) and same_bits(s1.outside, t32[:, 0])
    assert same_bits(s.loss, 0.5 * t32[:, 0] + 2.0 * t32[:, 1])
    assert same_bits(s.outside_vertices, got["counts"][:, 0]) and same_bits(s.uncovered_px, got["counts"][:, 1])
    # ---- a strided vertex block is read in place
    block = torch.zeros(P, V + 5, 3, device=DEV)
    block[:, :V] = dev(verts)
    view = block[:, :V].detach()
    assert P == 1 or not view.is_contiguous()
    strided = c_entry(name, size, verts=block, vstride=3 * (V + 5))
    _, g_view, _ = through_autograd(name, size, verts=view)
    for k in got:
        assert same_bits(got[k], strided[k]), k
    assert same_bits(g_view, got["g_verts"])
    # ---- against fp64 autograd of the oracle
    for k, what in enumerate(("outside", "uncovered")):
        g = got["g_verts"][k].astype(np.float64)
        assert np.isfinite(g).all()
        scale = np.abs(g_want[k]).max()
        ratio = np.abs(g - g_want[k]).max() / scale if scale else 0.0
        assert scale > 0 or (g == 0).all()
        print(f"silhouette {name} {size[0]}x{size[1]} {what}: max|got-want|/max|want| = {ratio:.3e} = {ratio / GATE:.3f} of the gate; terms rel {worst_t:.1e}")
        assert ratio <= GATE, (what, ratio)
        assert (g[~fwd["ok"]] == 0).all() and (g_want[k][~fwd["ok"]] == 0).all()                  # zeros, not NaN


@pytest.mark.parametrize("name", ["a", "f"])
def test_the_cover_is_what_mhmr_render_amodal_counts(name):
    """With all-ones masks and a cap no shorter than the image's diagonal every pixel the cover misses is in U_p, so
    counts[:, 1] = H W - amodal_px: the restated face and pixel rules of silhouette.hip against mhmr_render_amodal itself (both face
    passes: scene f's quad takes the workgroup pass in both files)."""
    H, W = S1
    verts, idx, K, faces, Rt, _, _, _ = scene(name, S1)
    assert all(so.project(verts[p], K, int(idx[p]), Rt, H, W)[0].any() for p in range(len(verts)))             # every person has a splat
    ones = torch.ones((len(verts), H, W), dtype=torch.bool, device=DEV)
    s = silhouette_loss(dev(verts), idx, K, faces, ones, Rt=Rt, ignore=None, max_dist=80)                      # 80 = sqrt(48^2 + 64^2)
    amodal = maps.render_maps(dev(verts), idx, K, faces, S1, Rt=Rt, amodal=True).amodal_px.reshape(-1)
    assert bool((amodal > 0).all()) and bool((amodal < H * W).all())
    assert torch.equal(s.uncovered_px, H * W - amodal)


def test_nobody_and_refusals_of_the_python_surface():
    verts, idx, K, faces, Rt, mask, _, _ = scene("a", S0)
    v = torch.zeros(0, 42, 3, device=DEV, requires_grad=True)
    s = silhouette_loss(v, [], K, faces, torch.zeros((0,) + S0, dtype=torch.bool, device=DEV), Rt=Rt)
    assert all(tuple(t.shape) == (0,) for t in s) and s.loss.dtype == torch.float32 and s.uncovered_px.dtype == torch.int32
    s.loss.sum().backward()
    assert tuple(v.grad.shape) == (0, 42, 3)
    # a region every person may project into: the whole image forgives everything outside
    whole = torch.ones((2,) + S0, dtype=torch.bool, device=DEV)
    s = silhouette_loss(dev(verts), idx, K, faces, dev(mask), Rt=Rt, ignore=whole, max_dist=R)
    assert bool((s.outside == 0).all()) and bool((s.outside_vertices == 0).all()) and bool((s.uncovered > 0).all())
    for bad in (dict(robust="huber"), dict(sigma=0.0), dict(max_dist=0), dict(ignore="all"), dict(ignore=whole[:1]), dict(size=(5, 5)),
                dict(max_workspace_bytes=silhouette.pass_bytes(S0, 42, 80) - 1), dict(Rt=Rt[:1])):
        with pytest.raises(ValueError):
            silhouette_loss(dev(verts), idx, K, faces, dev(mask), **{**dict(Rt=Rt), **bad})
    with pytest.raises(ValueError):
        distance_transform(torch.zeros(4, 5, device=DEV))
    # the person map of the scene, cut into a segmenter's unordered instances, comes back as the persons' own visible masks
    m = maps.render_maps(dev(verts), idx, K, faces, S0, Rt=Rt, amodal=False)
    person = m.person.reshape(2, *S0)
    inst = torch.stack([torch.stack([person[0] == 1, person[0] == 0]), torch.stack([person[1] == 2, torch.zeros_like(person[1], dtype=torch.bool)])])
    masks, matched = assign_instance_masks(person, idx, inst)
    assert matched.tolist() == [1, 0, 0] and all(torch.equal(masks[p], person[int(idx[p])] == p) for p in range(3))


# ---------------------------------------------------------------------------------------------------- through the model
S, NAME = 224, "dinov2_vits14"


@functools.lru_cache(maxsize=None)
def fixture():
    """The seeded depth-3 ViT-S at 224^2 of tests/test_gpu_raster.py on two images and the inference call that returns the read-out."""
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


def test_silhouette_loss_alone_pulls_a_person_moved_sideways_back():
    m, K, rich = fixture()
    faces = m.smpl_layer["neutral_10"].bm_x.faces
    r0, o0, idx = rich["readout"], rich["offset"], rich["idx"]
    P = int(r0.shape[0])
    assert 1 <= P <= 6
    with torch.no_grad():                                                # masks: the cover of each unmoved mesh, rendered alone
        v3d = m.decode_readout(r0, o0, idx, K)["v3d"]
        alone = [maps.render_maps(v3d[p:p + 1], idx[0][p:p + 1], K, faces, (S, S), amodal=False).person.reshape(-1, S, S) for p in range(P)]
        masks = torch.stack([alone[p][int(idx[0][p])] == 0 for p in range(P)])
    assert bool(masks.flatten(1).any(1).all())
    offset = (o0.clone() + torch.tensor([0.3, 0.0], device=DEV)).requires_grad_(True)          # loc is (cell + 0.5 + offset) * patch: 4 px sideways
    opt = torch.optim.Adam([offset], lr=0.02)
    losses = []
    for _ in range(12):
        opt.zero_grad()
        d = m.decode_readout(r0, offset, idx, K)
        loss = silhouette_loss(d["v3d"], idx[0], K, faces, masks).loss.sum()
        loss.backward()
        assert bool(torch.isfinite(offset.grad).all())
        opt.step()
        losses.append(float(loss.detach()))
    print(f"silhouette_loss alone, {P} persons, Adam lr 0.02 on the offset: {losses[0]:.4f} -> {losses[-1]:.4f} after {len(losses) - 1} steps")
    assert losses[0] > 0 and losses[-1] < losses[0]
