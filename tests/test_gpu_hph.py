"""-m gpu: the person-head kernels -- everything behind the backbone, in fp32 (csrc/hph.hip, csrc/anny.hip) -- called through the C ABI
against float64 references on the same fp32 (or already-rounded 16-bit) operands, at the edges the end-to-end goldens never reach:
more than 64 persons in one image (the self-attention's blockIdx.z > 0), more than 512 cross-attention work items (the launcher's second
launch), key slices without keys (N < 64), padding work items, logits of +-60 whose maximum comes first or last, the rotmat -> rotvec
branches (small angle, angle pi, argmax ties, nearly parallel 6D columns), the distance clamps, a skewed camera, the detection clamp.
Rows that no work item covers hold a sentinel that must survive.  Every gate is at most 4x the worst case measured on MI355X."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from multi_hmr_amd import _lib  # noqa: E402
from oracle import anny_hph_ref, roma_ref  # noqa: E402

EPS = 2.0 ** -23                       # fp32 machine epsilon
SCALE = 32 ** -0.5                     # dim_head = 32
SENT = -7777.0                         # rows no work item covers


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=dev())


# ------------------------------------------------------------------------------------------------------ attention inputs
def _qk(g, nq, nk, mode, spread=60.0):
    """[nq, 32] queries and [nk, 32] keys of one head whose logits q.k / sqrt(32) span about +-spread.
    random: isotropic.  rising: every query's logit grows with the key index (the largest key LAST: every step of an online softmax
    rescales).  falling: the largest key FIRST."""
    if mode == "random":
        s = math.sqrt(spread / 3)
        return torch.randn(nq, 32, generator=g, dtype=torch.float64) * s, torch.randn(nk, 32, generator=g, dtype=torch.float64) * s
    q = torch.randn(nq, 32, generator=g, dtype=torch.float64) * 0.3
    k = torch.randn(nk, 32, generator=g, dtype=torch.float64) * 0.01
    q[:, 0] = 1 + torch.rand(nq, generator=g, dtype=torch.float64)                  # in [1, 2): the same sign for every query
    w = torch.linspace(-1, 1, nk, dtype=torch.float64) * (spread / 2 / SCALE)
    k[:, 0] = w if mode == "rising" else w.flip(0)
    return q, k


def _softmax_ref(q, k, v):
    return torch.softmax(q.double() @ k.double().T * SCALE, dim=-1) @ v.double()


def _row_maxrel(got, ref):
    """per row: max |got - ref| / max |ref|  (rows = persons, all heads)"""
    got, ref = got.double(), ref.double()
    return ((got - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------------ (a) self-attention
@pytest.mark.parametrize("heads", [8, 16])
@pytest.mark.parametrize("mode", ["random", "rising", "falling"])
def test_self_attention_against_fp64(L, heads, mode):
    """Groups of 1, 8, 63, 64, 65 and 130 queries in ONE call (an empty group between them, three repeated end entries behind them:
    group count and nmax = P are upper bounds, as mhmr_person_groups leaves them), logits of +-60.  Groups past 64 queries are
    the workgroups with blockIdx.z > 0.  Measured worst row (max norm): 5.4e-6 random, 1.35e-5 largest key last, 1.0e-5 first
    (gate 3e-5: logits of 60 carry ~1e-5 of absolute fp32 error into exp)."""
    g = torch.Generator().manual_seed(100 * heads + ["random", "rising", "falling"].index(mode))
    inner = 32 * heads
    sizes = [1, 8, 0, 63, 64, 65, 130]
    gstart = [0]
    for n in sizes:
        gstart.append(gstart[-1] + n)
    n_real = gstart[-1]
    gstart += [n_real] * 3
    P = n_real + 5                                            # rows behind the last group: nobody's
    qkv = torch.randn(P, 3 * inner, generator=g, dtype=torch.float64)
    for s0, n in zip(gstart[:-4], sizes):
        for h in range(heads):
            if n == 0:
                continue
            q, k = _qk(g, n, n, mode)
            qkv[s0:s0 + n, h * 32:(h + 1) * 32] = q
            qkv[s0:s0 + n, inner + h * 32:inner + (h + 1) * 32] = k
    qkv = qkv.float()
    out = torch.full((P, inner), SENT, device=dev())
    qkv_d, gstart_d = qkv.to(dev()), i32(gstart)                # (named: a temporary's memory could be reused before the kernel runs)
    _lib.check(L.mhmr_hph_self_attn(qkv_d.data_ptr(), gstart_d.data_ptr(), out.data_ptr(), len(gstart) - 1, P, heads, stream()),
               "hph_self_attn")
    out = out.cpu()
    ref = torch.zeros(n_real, inner, dtype=torch.float64)
    for s0, n in zip(gstart[:-4], sizes):
        for h in range(heads):
            c = slice(h * 32, (h + 1) * 32)
            ref[s0:s0 + n, c] = _softmax_ref(qkv[s0:s0 + n, c], qkv[s0:s0 + n, inner:][:, c], qkv[s0:s0 + n, 2 * inner:][:, c])
    err = _row_maxrel(out[:n_real], ref)
    worst = float(err.max())
    print(f"\n[hph self-attn heads {heads} {mode}] worst row {worst:.2e} (row {int(err.argmax())})")
    assert worst < 3e-5, (worst, int(err.argmax()))
    assert bool((out[n_real:] == SENT).all())


# ------------------------------------------------------------------------------------------------------ (b) cross-attention
def _xattn(L, heads, N, items, B, mode, seed, npad=3):
    """items: (image, count) work items; their rows are laid out in order with one uncovered row after every third item; npad
    count-0 items at the tail.  Returns (worst row error, sentinel rows intact)."""
    g = torch.Generator().manual_seed(seed)
    inner = 32 * heads
    chunks, rows, row = [], [], 0
    for t, (b, c) in enumerate(items):
        chunks += [b, row, c]
        rows.append((b, row, c))
        row += c + (1 if t % 3 == 2 else 0)
    chunks += [0, 0, 0] * npad
    P = row + 1
    q = torch.randn(P, inner, generator=g, dtype=torch.float64)
    kv = torch.randn(B * N, 2 * inner, generator=g, dtype=torch.float64)
    if mode == "random":
        q *= math.sqrt(20.0)
        kv[:, :inner] *= math.sqrt(20.0)
    else:
        for h in range(heads):
            c = slice(h * 32, (h + 1) * 32)
            for b in range(B):
                qb, kb = _qk(g, P, N, mode)
                kv[b * N:(b + 1) * N, c] = kb
                if b == 0:
                    q[:, c] = qb
    q, kv = q.float(), kv.float()
    out = torch.full((P, inner), SENT, device=dev())
    q_d, kv_d, chunks_d = q.to(dev()), kv.to(dev()), i32(chunks)
    _lib.check(L.mhmr_hph_cross_attn(q_d.data_ptr(), kv_d.data_ptr(), chunks_d.data_ptr(), len(chunks) // 3, out.data_ptr(), heads, N,
                                     stream()), "hph_cross_attn")
    out = out.cpu()
    covered = torch.zeros(P, dtype=torch.bool)
    errs = []
    for b, r0, c in rows:
        covered[r0:r0 + c] = True
        ref = torch.zeros(c, inner, dtype=torch.float64)
        for h in range(heads):
            hc = slice(h * 32, (h + 1) * 32)
            ref[:, hc] = _softmax_ref(q[r0:r0 + c, hc], kv[b * N:(b + 1) * N, hc], kv[b * N:(b + 1) * N, inner:][:, hc])
        errs.append(_row_maxrel(out[r0:r0 + c], ref))
    worst = float(torch.cat(errs).max())                       # (a NaN row makes this NaN, and every gate fails)
    return worst, bool((out[~covered] == SENT).all()) and bool(torch.isfinite(out[covered]).all())


ITEMS = [(0, c) for c in range(1, 9)] + [(1, c) for c in range(8, 0, -1)]


@pytest.mark.parametrize("heads", [8, 16])
@pytest.mark.parametrize("N", [1, 7, 63, 64, 65, 256, 4096])
def test_cross_attention_against_fp64(L, heads, N):
    """Work items of 1 ... 8 queries over two images, three count-0 items at the tail, logits of +-60.  N < 64 leaves key slices (and,
    for N < 57, whole waves) without keys: m = -inf in the xor merge and in the LDS merge.  Measured worst row: 6.3e-6 (gate 2.5e-5)."""
    worst, kept = _xattn(L, heads, N, ITEMS, 2, "random", seed=N * 31 + heads)
    print(f"\n[hph cross-attn heads {heads} N {N}] worst row {worst:.2e}")
    assert worst < 2.5e-5, worst
    assert kept


@pytest.mark.parametrize("mode", ["rising", "falling"])
@pytest.mark.parametrize("N", [7, 65, 4096])
def test_cross_attention_largest_key_last_or_first(L, mode, N):
    """Every query's largest logit on the LAST key (every slice rescales at every step; at N = 4096 the maximum sits in the last
    slice of the last wave) or on the first one.  Measured worst row: 1.0e-5, largest key last at N = 4096 (gate 3e-5)."""
    worst, kept = _xattn(L, 8, N, ITEMS, 2, mode, seed=N + (0 if mode == "rising" else 1))
    print(f"\n[hph cross-attn {mode} N {N}] worst row {worst:.2e}")
    assert worst < 3e-5, worst
    assert kept


def test_cross_attention_more_than_512_work_items(L):
    """600 work items over two images (+ 10 count-0 items): the launcher's second launch over entries 512 ... 609, whose workgroups
    count their real items with __syncthreads_count.  Measured worst row: 6.3e-6 (gate 2.5e-5)."""
    items = [(0 if t < 300 else 1, 1 + t % 8) for t in range(600)]
    worst, kept = _xattn(L, 8, 16, items, 2, "random", seed=600, npad=10)
    print(f"\n[hph cross-attn 600 items] worst row {worst:.2e}")
    assert worst < 2.5e-5, worst
    assert kept


# ------------------------------------------------------------------------------------------------------ (c) the layer stack
def _stack_case(dim, heads, mlp, depth, counts, N, precision, seed):
    from multi_hmr_amd.anny_hph import HPH
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16}[precision]
    sd, x, context, mask = anny_hph_ref.make_case(seed=seed, dim=dim, depth=depth, heads=heads, mlp=mlp, counts=counts, N=N)
    m = HPH(dim=dim, depth=depth, heads=heads, dim_head=32, mlp_dim=mlp, dropout=0.0, precision=precision)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev()).eval()
    y = m(x.to(dev()), context.to(dev()), mask.to(dev())).cpu()
    # the operands the kernels see: fp32 weights and queries, the context and to_kv.weight rounded to the 16-bit type
    sd64 = {k: (v.to(tdt) if ".1.fn.to_kv." in k else v).double() for k, v in sd.items()}
    ref = anny_hph_ref.forward(sd64, x.double(), context.to(tdt).double(), mask.double(), depth=depth, heads=heads)
    real = mask.bool()
    d = (y[real].double() - ref[real]).norm(dim=1) / ref[real].norm(dim=1)
    return float(d.max()), float((y[real].double() - ref[real]).norm() / ref[real].norm()), bool((y[~real] == 0).all())


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("cfg", ["multihmr", "anny"])
def test_layer_stack_against_fp64(precision, cfg):
    """mhmr_xattn_layers_forward through anny_hph.HPH vs oracle/anny_hph_ref.forward in float64, persons (130, 0, 1, 65, 9) at N = 256.
    On real rows that is also the Multi-HMR decoder (oracle/multihmr_ref.transformer_decoder: its mask multiplies only touch padded
    rows), so one reference covers both configurations.  Per person rel-L2, worst over persons: measured 4.2e-7 (Multi-HMR) and 6.7e-7
    (Anny), f16 and bf16 alike (gate 2.5e-6)."""
    dim, heads, mlp, depth = {"multihmr": (1024, 8, 1024, 2), "anny": (512, 16, 2048, 8)}[cfg]
    worst, whole, zeros = _stack_case(dim, heads, mlp, depth, (130, 0, 1, 65, 9), 256, precision, seed=7)
    print(f"\n[hph stack {cfg} {precision}] worst person {worst:.2e}, batch {whole:.2e}")
    assert worst < 2.5e-6, worst
    assert zeros


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_layer_stack_long_context(precision):
    """One image of 4096 context tokens (896^2), three persons, a small stack.  Measured worst person: 3.0e-7 (gate 1.2e-6)."""
    worst, whole, zeros = _stack_case(256, 8, 512, 2, (3,), 4096, precision, seed=8)
    print(f"\n[hph stack N 4096 {precision}] worst person {worst:.2e}")
    assert worst < 1.2e-6, worst


# ------------------------------------------------------------------------------------------------------ (d) decode battery
def _rot(axis, angle):
    a = torch.tensor(axis, dtype=torch.float64)
    return roma_ref.rotvec_to_rotmat((a / a.norm() * angle)[None])[0]


GEN1, GEN2 = (0.3, -0.5, 0.81), (-0.7, 0.2, -0.4)


def _battery(g, n):
    """n pairs of 6D columns (x, y) [n, 3, 2] in float64: chosen rotations first, then random 6D read-outs."""
    R = [torch.eye(3, dtype=torch.float64)]
    for a in (1e-6, 9.9e-4, 1.01e-3, 1e-2):                                  # around the small-angle series' threshold 1e-3
        R += [_rot(GEN1, a), _rot(GEN2, a)]
    for d in (0.0, 1e-6, 1e-3):                                              # angle pi - d: qw ~ 0, the sign flip
        R += [_rot(ax, math.pi - d) for ax in ((1, 0, 0), (0, 1, 0), (0, 0, 1), GEN1, GEN2, (-1, 0, 0), (0, -1, 0))]
    t = lambda *m: torch.tensor(m, dtype=torch.float64).reshape(3, 3)
    R += [t(0, -1, 0, 1, 0, 0, 0, 0, 1),                                     # R22 == trace
          t(0, 1, 0, 1, 0, 0, 0, 0, -1),                                     # R00 == R11 (angle pi)
          t(0, 0, 1, 1, 0, 0, 0, 1, 0),                                      # R00 == R11 == R22 == trace
          t(-1, 0, 0, 0, 0, 1, 0, 1, 0),                                     # R11 == R22
          t(0, 0, 1, 0, -1, 0, 1, 0, 0),                                     # R00 == R22
          t(1, 0, 0, 0, 0, -1, 0, 1, 0),                                     # R00 == trace
          t(-1, 0, 0, 0, -1, 0, 0, 0, 1)]                                    # R22 == 1 > trace
    for _ in range(24):                                                      # large angles about random axes: qw < 0 in half of them
        ax = torch.randn(3, generator=g, dtype=torch.float64)
        R.append(roma_ref.rotvec_to_rotmat((ax / ax.norm() * (2.0 + 1.1 * torch.rand(1, generator=g, dtype=torch.float64)))[None])[0])
    cols = [torch.stack([r[:, 0], r[:, 1]], dim=1) for r in R]
    for r in R[-8:]:                                                         # nearly parallel columns: the same rotation
        for phi in (1e-3, 1e-2):
            cols.append(torch.stack([r[:, 0], math.cos(phi) * r[:, 0] + math.sin(phi) * r[:, 1]], dim=1))
    for r in R[-6:]:                                                         # column norms far from 1
        for sx, sy in ((1e-3, 1e-3), (1e3, 1e3), (1e-3, 1e3), (1e3, 1e-3)):
            cols.append(torch.stack([sx * r[:, 0], sy * r[:, 1]], dim=1))
    cols = torch.stack(cols)
    assert len(cols) <= n
    return torch.cat([cols, torch.randn(n - len(cols), 3, 2, generator=g, dtype=torch.float64)])


def _check_rotations(M32, rotmat, rotvec, tag):
    """M32 [n, 3, 2] fp32 6D columns, rotmat [n, 3, 3] / rotvec [n, 3] the kernel's.  Returns the worst gate ratios."""
    M = M32.double()
    ref_R = roma_ref.special_gramschmidt(M)
    x, y = M[..., 0], M[..., 1]
    sin_phi = torch.linalg.cross(x, y).norm(dim=-1) / (x.norm(dim=-1) * y.norm(dim=-1))
    eR = (rotmat.double() - ref_R).abs().amax((1, 2)) * sin_phi / EPS           # in units of eps / sin(phi)
    Rk = rotmat.double()
    ref_v = roma_ref.rotmat_to_rotvec(Rk)                                        # the conversion alone, on the kernel's own matrix
    near_pi = (ref_v.norm(dim=-1) - math.pi).abs() < 1e-5
    ev = (rotvec.double() - ref_v).norm(dim=-1) / (EPS * ref_v.norm(dim=-1).clamp_min(1e-30))
    ev = torch.where(ref_v.norm(dim=-1) == 0, (rotvec.double().norm(dim=-1) > 0).double() * 1e30, ev)
    epi = (roma_ref.rotvec_to_rotmat(rotvec.double()) - roma_ref.rotvec_to_rotmat(ref_v)).abs().amax((1, 2)) / EPS
    ev = torch.where(near_pi, epi, ev)
    print(f"\n[{tag}] rotmat worst {float(eR.max()):.1f} eps/sin(phi) (joint {int(eR.argmax())}); rotvec worst {float(ev.max()):.1f} eps "
          f"relative (joint {int(ev.argmax())}), {int(near_pi.sum())} joints within 1e-5 of pi")
    return float(eR.max()), float(ev.max()), int(near_pi.sum())


@pytest.mark.parametrize("nb", [10, 11])
@pytest.mark.parametrize("nearness", [0, 1])
def test_hph_decode_battery(L, nb, nearness):
    """mhmr_hph_decode on 8 persons x 53 joints of chosen 6D read-outs (HPH layout: reshape(-1,2,3).permute(0,2,1), the first three
    numbers = column 0): rotmat vs roma special_gramschmidt in fp64 of the same input, in units of eps / sin(angle between the columns);
    rotvec vs roma rotmat_to_rotvec in fp64 of the kernel's own rotmat (within 1e-5 of pi: the rotations).  betas / expression /
    dist_pp are copies (bit-equal); dist against the fp64 formula with a different focal per image, both clamps reached.
    nb = 11 is the kid head's layout; a pitch above 318 + nb + 13 for nb = 11.  Measured: rotmat 1.4 eps / sin(phi), rotvec 2.5 eps,
    dist 0.34 eps (1 + |argument|) (gates 5, 8, 1.3)."""
    g = torch.Generator().manual_seed(nb * 2 + nearness)
    P, B = 8, 3
    ldd = 318 + nb + 13 + (5 if nb == 11 else 0)
    M32 = _battery(g, P * 53).float()                                           # [P*53, 3, 2]
    dec = torch.randn(P, ldd, generator=g)
    dec[:, :318] = M32.permute(0, 2, 1).reshape(P, 318)                         # (x0 x1 x2 y0 y1 y2) per joint
    K = torch.tensor([[900.0, 0, 300], [0, 900, 310], [0, 0, 1]]).repeat(B, 1, 1)
    K[:, 0, 0] = torch.tensor([900.0, 1400.0, 610.0])
    det_b = [0, 1, 2, 0, 1, 2, 2, 0]
    fn = 448 / (2 * math.tan(math.radians(30)))
    arg = torch.tensor([-40.0, -0.5, 0.7, 2.0, 3.5, 3.95, 60.0, 25.0], dtype=torch.float64)   # d0 * focal / fn
    focal = K[det_b, 0, 0].double()
    dec[:, 318 + nb] = (arg * np.float32(fn) / focal).float()
    outs = [torch.full(s, SENT, device=dev()) for s in ((P, 53, 3, 3), (P, 53, 3), (P, nb), (P, 10), (P,), (P,))]
    rotmat, rotvec, betas, expr, dist_pp, dist = outs
    decd, Kd, det_bd = dec.to(dev()), K.to(dev()), i32(det_b)
    _lib.check(L.mhmr_hph_decode(decd.data_ptr(), ldd, nb, Kd.data_ptr(), det_bd.data_ptr(), float(fn), nearness,
                                 *[t.data_ptr() for t in outs], P, stream()), "hph_decode")
    rotmat, rotvec, betas, expr, dist_pp, dist = [t.cpu() for t in outs]
    eR, ev, npi = _check_rotations(M32, rotmat.reshape(-1, 3, 3), rotvec.reshape(-1, 3), f"hph decode nb {nb} nearness {nearness}")
    assert npi >= 10
    assert eR < 5, eR
    assert ev < 8, ev
    assert torch.equal(betas, dec[:, 318:318 + nb]) and torch.equal(expr, dec[:, 318 + nb + 3:318 + nb + 13])
    assert torch.equal(dist_pp, dec[:, 318 + nb])
    d = dec[:, 318 + nb].double() * (focal / np.float32(fn))
    a = d.clone()
    if nearness:
        d = torch.exp(d) - 1e-10
    ref = d.clamp(0, 50)
    ed = (dist.double() - ref).abs() / (EPS * (1 + a.abs()) * ref.abs()).clamp_min(1e-300)
    ed = torch.where(ref == 0, (dist != 0).double() * 1e30, ed)
    print(f"[hph decode dist nearness {nearness}] worst {float(ed.max()):.2f} eps (1 + |arg|); clamped {int((ref == 0).sum())} x 0, "
          f"{int((ref == 50).sum())} x 50")
    assert float(ed.max()) < 1.3
    assert bool((ref == 0).any()) and bool((ref == 50).any())


def test_anny_decode_battery(L):
    """mhmr_anny_decode: J = 163 joints (not a multiple of 64) of 3 persons, Anny layout (reshape(-1,3,2): rows), a quarter of the joints
    useful = 0 (exactly I and a zero rotvec), shape = sigmoid, dist = focal / max(exp(d), 1e-5) with d reaching the clamp, loc, and
    transl = K^-1 [loc, 1] dist for a K with skew and an off-centre principal point, against torch.linalg.inv in fp64.
    Measured: rotmat 1.3 eps / sin(phi), rotvec 1.7 eps, shape 0.31, dist 0.58, loc 0.45, transl 0.62 eps (gates 5, 6, 1.2, 2, 1.8, 2.4)."""
    g = torch.Generator().manual_seed(163)
    P, J, nb, B, patch = 3, 163, 11, 2, 14
    M32 = _battery(g, P * J).float()
    rot6d = M32.reshape(P, J * 6)                                               # [3][2] rows: (e0 e1), (e2 e3), (e4 e5)
    useful = (torch.rand(J, generator=g) > 0.25).float()
    useful[0] = useful[J - 1] = 0.0
    shape_logit = torch.randn(P, nb, generator=g) * 8
    dist_logit = torch.tensor([-30.0, 0.3, 2.5])
    offset = torch.randn(P, 2, generator=g) * 0.3
    det_b, det_y, det_x = [1, 0, 1], [3, 17, 40], [25, 2, 63]
    K = torch.tensor([[[900.0, 35.0, 410.0], [0.0, 870.0, 530.0], [0.0, 0.0, 1.0]],
                      [[640.0, -12.5, 230.0], [0.0, 655.0, 270.0], [0.0, 0.0, 1.0]]])
    outs = [torch.full(s, SENT, device=dev()) for s in ((P, J, 3, 3), (P, J, 3), (P, nb), (P, 2), (P,), (P, 3))]
    d = lambda t: t.to(dev()).contiguous()
    keep = [d(rot6d), d(useful), d(shape_logit), d(dist_logit), d(offset), i32(det_b), i32(det_y), i32(det_x), d(K)]
    _lib.check(L.mhmr_anny_decode(keep[0].data_ptr(), keep[1].data_ptr(), J, keep[2].data_ptr(), nb, keep[3].data_ptr(), keep[4].data_ptr(),
                                  keep[5].data_ptr(), keep[6].data_ptr(), keep[7].data_ptr(), keep[8].data_ptr(), patch, P,
                                  *[t.data_ptr() for t in outs], stream()), "anny_decode")
    rotmat, rotvec, shape, loc, dist, transl = [t.cpu() for t in outs]
    use = useful.bool().repeat(P)
    Rk, vk = rotmat.reshape(-1, 3, 3), rotvec.reshape(-1, 3)
    assert bool((Rk[~use] == torch.eye(3)).all()) and bool((vk[~use] == 0).all())
    eR, ev, npi = _check_rotations(M32[use], Rk[use], vk[use], "anny decode")
    assert eR < 5, eR
    assert ev < 6, ev
    s_ref = torch.sigmoid(shape_logit.double())
    es = float(((shape.double() - s_ref).abs() / (EPS * s_ref * (1 + shape_logit.double().abs()))).max())
    f = K[det_b, 0, 0].double()
    dist_ref = f / torch.exp(dist_logit.double()).clamp_min(float(np.float32(1e-5)))
    edist = float(((dist.double() - dist_ref).abs() / (EPS * (1 + dist_logit.double().abs()) * dist_ref)).max())
    loc_ref = (torch.tensor([det_x, det_y], dtype=torch.float64).T + 0.5 + offset.double()) * patch
    eloc = float(((loc.double() - loc_ref).abs() / (EPS * loc_ref.abs())).max())
    Ki = torch.linalg.inv(K.double())[det_b]                                     # [P, 3, 3]
    h = torch.cat([loc_ref, torch.ones(P, 1, dtype=torch.float64)], 1)
    t_ref = (Ki @ h[:, :, None])[:, :, 0] * dist_ref[:, None]
    bound = ((Ki.abs() @ h.abs()[:, :, None])[:, :, 0] * dist_ref[:, None]).norm(dim=1)     # |K^-1| |[loc, 1]| dist
    et = float(((transl.double() - t_ref).norm(dim=1) / (EPS * bound)).max())
    print(f"[anny decode] shape {es:.2f}, dist {edist:.2f}, loc {eloc:.2f}, transl {et:.2f} eps")
    assert float(dist_ref[0]) == pytest.approx(float(f[0]) / 1e-5, rel=1e-6)       # the clamp was reached
    assert es < 1.2 and edist < 2 and eloc < 1.8 and et < 2.4, (es, edist, eloc, et)


# ------------------------------------------------------------------------------------------------------ (e) scores and camera
@pytest.mark.parametrize("dtname", ["f16", "bf16"])
@pytest.mark.parametrize("C", [384, 768, 1024])
def test_detection_and_anny_scores(L, dtname, C):
    """mhmr_detect_scores (clamped to [1e-4, 1 - 1e-4]) and mhmr_anny_scores (not clamped) on the same 16-bit hid: 203 rows (not a
    multiple of 4), a row pitch ld = C + 64, logits beyond +-9.3 on both sides.  Against fp64 on the same operands, the error of the
    logit bounded by eps sum |h w|.  Measured: logit 0.17, scores 0.65 eps (gates 0.6, 2.5)."""
    dt, tdt = {"f16": (_lib.DT_F16, torch.float16), "bf16": (_lib.DT_BF16, torch.bfloat16)}[dtname]
    g = torch.Generator().manual_seed(C + dt)
    rows, ld = 203, C + 64
    gain = torch.linspace(0.05, 1.0, rows)[:, None] * 30
    hid = (torch.randn(rows, ld, generator=g) * gain).to(tdt)
    hid[:, C:] = float("nan")                                                   # beyond C: never read
    w2 = torch.randn(C, generator=g) / math.sqrt(C)
    b2 = torch.tensor([-0.2])
    sc, sa, lg = (torch.full((rows + 1,), SENT, device=dev()) for _ in range(3))
    hd, wd, bd = hid.to(dev()), w2.to(dev()), b2.to(dev())
    _lib.check(L.mhmr_detect_scores(hd.data_ptr(), ld, wd.data_ptr(), bd.data_ptr(), sc.data_ptr(), rows, C, dt, stream()), "detect_scores")
    _lib.check(L.mhmr_anny_scores(hd.data_ptr(), ld, wd.data_ptr(), bd.data_ptr(), sa.data_ptr(), lg.data_ptr(), rows, C, dt, stream()),
               "anny_scores")
    sc, sa, lg = sc.cpu(), sa.cpu(), lg.cpu()
    assert float(sc[rows]) == SENT and float(sa[rows]) == SENT and float(lg[rows]) == SENT
    sc, sa, lg = sc[:rows].double(), sa[:rows].double(), lg[:rows].double()
    h = hid[:, :C].double()
    logit = h @ w2.double() + float(b2)
    mag = h.abs() @ w2.double().abs() + abs(float(b2))
    assert float(logit.max()) > 9.3 and float(logit.min()) < -9.3
    s = torch.sigmoid(logit)
    lo, hi = float(np.float32(1e-4)), float(np.float32(1) - np.float32(1e-4))
    el = float(((lg - logit).abs() / (EPS * mag)).max())
    ea = float(((sa - s).abs() / (EPS * (s * (1 - s) * mag + s))).max())
    sref = s.clamp(lo, hi)
    ec = float(((sc - sref).abs() / (EPS * (sref * (1 - sref) * mag + sref))).max())
    print(f"\n[scores {dtname} C {C}] logit {el:.2f}, anny score {ea:.2f}, detect score {ec:.2f} eps")
    assert el < 0.6 and ea < 2.5 and ec < 2.5, (el, ea, ec)
    assert float(sc.min()) == lo and float(sc.max()) == hi                    # the detection clamp, on both sides
    assert float(sa.min()) < lo and float(sa.max()) > hi                      # and none in the Anny path


def test_anny_camera(L):
    """mhmr_anny_camera: fov = pi sigmoid(logit), focal = (S/2) / tan(fov/2), K with the principal point at S/2, for logits -30 ... 30
    and S = 448 / 896.  At logit 30 fov is pi to fp32 and tan sits on its pole: the gate on focal scales with the condition number
    x (tan x + cot x) of tan at x = fov / 2.  Measured: fov 0.79 eps, focal 0.55 eps x cond (gates 3, 2)."""
    logit = torch.tensor([-30.0, -2.5, 0.0, 1.7, 30.0])
    fov_max = float(np.float32(math.pi))
    for S in (448, 896):
        B = len(logit)
        fov, K = torch.full((B,), SENT, device=dev()), torch.full((B, 3, 3), SENT, device=dev())
        ld = logit.to(dev())
        _lib.check(L.mhmr_anny_camera(ld.data_ptr(), B, S, fov_max, fov.data_ptr(), K.data_ptr(), stream()), "anny_camera")
        fov, K = fov.cpu().double(), K.cpu().double()
        fref = fov_max * torch.sigmoid(logit.double())
        ef = float(((fov - fref).abs() / (EPS * fref)).max())
        x = fref / 2
        focal = (S / 2) / torch.tan(x)
        cond = 2 + x * (torch.tan(x) + 1 / torch.tan(x)).abs()
        efo = float(((K[:, 0, 0] - focal).abs() / (EPS * cond * focal.abs())).max())
        print(f"\n[anny camera S {S}] fov {ef:.2f} eps, focal {efo:.2f} eps x cond")
        assert ef < 3 and efo < 2, (ef, efo)
        assert torch.equal(K[:, 0, 0], K[:, 1, 1])
        z = torch.zeros(B, dtype=torch.float64)
        for (r, c), v in {(0, 1): 0.0, (1, 0): 0.0, (2, 0): 0.0, (2, 1): 0.0, (0, 2): S / 2, (1, 2): S / 2, (2, 2): 1.0}.items():
            assert torch.equal(K[:, r, c], z + v), (r, c)


# ------------------------------------------------------------------------------------------------------ (f) a crowd end to end
def test_crowd_end_to_end_against_the_oracle(smplx_data, mean_params):
    """ViT-S depth 2 at 224^2 (G = 16), persons [130, 0, 1, 65] through the idx hook: the only test that runs a >64-person image
    through mhmr_person_groups -> mhmr_hph_forward -> LBS as the product does.  precision='f16x3' puts the backbone at fp32 accuracy,
    so the x3 contract of test_gpu_x3.py holds: every key of parity.CHECKED within 3e-4 rel-L2 of the CPU oracle.  Measured: 1.1e-4
    (scores), every other key <= 4.8e-5; worst single person 9.8e-5 (dist_postprocessed; gate 4e-4)."""
    import make_golden
    from multi_hmr_amd import Model
    from oracle.multihmr_ref import OracleModel
    from parity import CHECKED, rel
    cfg = dict(backbone="dinov2_vits14", img_size=224, depth_override=2, batch=4, persons=[130, 0, 1, 65], seed=51)
    sd = make_golden.case_state_dict(cfg)
    x, K, idx = make_golden.case_inputs(cfg)
    m = Model(backbone=cfg["backbone"], img_size=224, smplx_data=smplx_data, mean_params=mean_params, backbone_depth=2, precision="f16x3")
    m.load_state_dict(sd, strict=True)
    m = m.to(dev()).eval()
    out = m(x.to(dev()), idx=tuple(i.to(dev()) for i in idx), K=K.to(dev()), is_training=True)
    ref = OracleModel(sd, smplx_data, backbone=cfg["backbone"], img_size=224, depth_override=2).forward(x, idx=idx, K=K, is_training=True)
    errs, person = {}, {}
    for k in CHECKED:
        a, b = out[k].detach().cpu().double().numpy(), ref[k].double().numpy()
        errs[k] = rel(a, b)
        if a.ndim >= 1 and a.shape[0] == 196:
            pa, pb = a.reshape(196, -1), b.reshape(196, -1)
            pe = np.linalg.norm(pa - pb, axis=1) / np.maximum(np.linalg.norm(pb, axis=1), 1e-30)
            person[k] = (float(pe.max()), int(pe.argmax()))
    print("\n[crowd 224 f16x3] " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    print("[crowd 224 f16x3] worst person " + " ".join(f"{k}={v[0]:.1e}@{v[1]}" for k, v in person.items()))
    assert out["v3d"].shape[0] == 196
    for k, v in errs.items():
        assert v < 3e-4, (k, v)
    for k, (v, p) in person.items():
        assert v < 4e-4, (k, v, p)
