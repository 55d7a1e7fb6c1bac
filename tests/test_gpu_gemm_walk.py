"""-m gpu: the persistent 256x256 GEMM (csrc/gemm256.hip) where a workgroup walks MORE THAN ONE tile per launch, through the C ABI.

The launcher starts min(tiles, G) workgroups (G = compute units of the device), so every shape of tests/test_gpu_kernels.py but one gives
each workgroup exactly one tile.  Here the row-tile count R follows G so that a launch falls into a walk class:

    A   G < tiles < 2G     one full round + a partial one: nmine is 2 for some workgroups and 1 for the others
    B   2G < tiles < 3G    two full rounds + a partial one: nmine is 3 for some; tile r = 1 has a predecessor AND a successor

Every case asserts
    (a) the whole output against fp64 torch on the identical, already rounded operands (gates: DTYPES' tol in max-norm for 16-bit
        outputs, 2e-5 for fp32 outputs, 1e-5 for the block sums); a failure lists the failing 256x256 tiles as (row tile, column tile);
    (b) every output is filled with a sentinel first and whatever the launch must not write is bit-unchanged: guard rows / heads behind
        the matrix, skipped rows under the token-row map, masked columns, rows >= Mvalid;
    (c) walk invariance: bit-equal to the same output assembled from launches of the SAME entry over row slabs of at most G tiles (one
        tile per workgroup; pointer offsets on A / out, whole images under the row map and for V^T) -- a tile's arithmetic does not
        depend on the round that computes it and there are no atomics, so equality is exact;
    (d) two calls give bit-equal results.

Which case reaches which part of the tile walk (on a 256-CU device; on another CU count the shapes still follow G and the same
assertions hold, only the column-group remarks stop applying):
    nmine = 2 / partial round      every class A case          nmine = 3 (r = 1 between two tiles)   every class B case
    G % 8 XCD remap                every case (G = 256)        tile order without column groups      nbn = 1, 3, 4
    column groups, ncg = 2         nbn = 8: test_walk_plain_epilogues[8-*], the Q | K fold consumer at N = 2048
    column groups, ncg = 4         nbn = 16: test_walk_plain_epilogues[16-*], the GELU fold consumer at N = 4096
    strip handoff (fold consumers) test_walk_layernorm_fold_consumers (K = 256: the minimum; 384), test_walk_masked_width, test_walk_merged_qkv[fold]
    stagger_ticks != 0             test_walk_staggered_residual (>= 1024 tiles, residual epilogue, no row map)
    img_magic, 9 tiles per image   test_walk_token_row_map and the mapped halves of the two LayerNorm-fold tests
    K = 128: one k pair, the handoff IS the k loop       nbn = 16 and nbn = 1 plain cases, V^T, patch, row map class A, stagger
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from multi_hmr_amd import _lib, vit  # noqa: E402
from test_gpu_kernels import DTYPES, L, dev, maxrel, rel, stream, swap23  # noqa: E402,F401

GUARD = 256          # guard rows behind every row-major output: one whole row tile
NIMG, STRIDE = 2304, 2368      # token-row map: 9 row tiles per image (the 672^2 grid; a non-power-of-two reciprocal), 64 skipped rows behind them
FOLD_TRUE_TOL = {"f16": 2e-3, "bf16": 1.6e-2}      # test_layernorm_fold's gate against the real LayerNorm + linear (rel-L2)


def ncus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, device=dev())


def rand(g, *shape):
    return torch.rand(*shape, generator=g, device=dev())


def assert_class(tiles, G, cls):
    lo = G if cls == "A" else 2 * G
    assert lo < tiles < lo + G, (tiles, G, cls)


def walk_rows(G, nbn, cls):
    """The smallest row-tile count of walk class `cls` at nbn column tiles."""
    R = (G if cls == "A" else 2 * G) // nbn + 1
    assert_class(R * nbn, G, cls)
    return R


def mapped_images(G, nbn, cls):
    """The smallest image count of walk class `cls` under the row map (NIMG / 256 row tiles per image)."""
    per = (NIMG // 256) * nbn
    B = (G if cls == "A" else 2 * G) // per + 1
    assert_class(B * per, G, cls)
    return B


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def bad_tiles(got, want, thresh=0.0):
    """(row tile, column tile) of every 256x256 tile of a logical [M, N] matrix whose max |got - want| exceeds thresh (NaN counts)."""
    d = (got.double() - want.double()).abs()
    M, N = d.shape
    d = torch.nn.functional.pad(d, (0, -N % 256, 0, -M % 256))
    t = d.view(d.shape[0] // 256, 256, d.shape[1] // 256, 256).amax((1, 3))
    idx = (~(t <= thresh)).nonzero().tolist()
    return f"{len(idx)} of {t.numel()} tiles fail: {[tuple(i) for i in idx[:48]]}{' ...' if len(idx) > 48 else ''}"


def gate(label, got, want, tol, norm=maxrel):
    """(a): print the figure, then assert it; a failure names the tiles that miss the gate."""
    err = norm(got, want)
    print(f"WALK {label}: {err:.3e} (gate {tol:.1e})")
    assert err < tol, (label, err, bad_tiles(got, want, tol * float(want.double().abs().max())))


def walk(label, launch, fresh, units, per_slab, logical):
    """(c) + (d).  launch(outs, u0, nu) runs the entry over units [u0, u0 + nu) (row tiles or images) into the tuple of outputs `outs`;
    fresh() makes sentinel-filled outputs; logical(outs) -> the outputs as logical [M, N] matrices (for the failing-tile list).  Whole
    tensors are compared, sentinels included.  Returns the outputs of the one-launch walk."""
    assert per_slab >= 1
    one, two, slab = fresh(), fresh(), fresh()
    launch(one, 0, units)
    launch(two, 0, units)
    for u0 in range(0, units, per_slab):
        launch(slab, u0, min(per_slab, units - u0))
    torch.cuda.synchronize()
    for what, other in (("(d) second call", two), ("(c) slab launches", slab)):
        if not all(same_bits(a, b) for a, b in zip(one, other)):
            tiles = [bad_tiles(a, b) for a, b in zip(logical(one), logical(other))]
            pytest.fail(f"{label}: the walk is not bit-equal to {what}: {tiles}")
    return one


def vt_logical(vt, B, H, Tp, T):
    """[>= B*H, 64, Tp] key-permuted V^T -> logical [B * T, 64 H] (token t of an image is stored at column swap23(t))."""
    perm = swap23(torch.arange(T, device=vt.device))
    return vt[: B * H].view(B, H, 64, Tp)[..., perm].permute(0, 3, 1, 2).reshape(B * T, 64 * H)


def qscale(N, cols=None):
    sc = torch.ones(N, device=dev(), dtype=torch.float64)
    sc[: (N // 2 if cols is None else cols)] = _lib.ATTN_QSCALE
    return sc


gelu = torch.nn.functional.gelu


# ------------------------------------------------------------------------------------------------------ 1: plain epilogues
@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@pytest.mark.parametrize("nbn,cls,K", [(3, "A", 384), (3, "B", 384), (8, "A", 256), (8, "B", 256), (16, "A", 128), (16, "B", 128), (1, "A", 128)])
def test_walk_plain_epilogues(L, name, dt, tdt, tol, nbn, cls, K):
    """mhmr_gemm16, the six plain epilogues.  nbn = 3: XCD remap, no column groups, an odd number of k pairs; nbn = 8 / 16: column-group
    order with ncg = 2 / 4 in the full rounds and the plain order in the partial one; K = 128 (nbn = 16, 1): a single k pair."""
    G = ncus()
    R = walk_rows(G, nbn, cls)
    M, N = 256 * R, 256 * nbn
    g = gen(1000 * nbn + K + (cls == "B"))
    A = randn(g, M, K).to(tdt)
    W = (randn(g, N, K) / math.sqrt(K)).to(tdt)
    bias, gamma = randn(g, N), randn(g, N)
    res = randn(g, M + GUARD, N)
    ref = A.double() @ W.double().T + bias.double()
    cases = [("op16", _lib.EPI_OP16, tdt, lambda: ref), ("gelu", _lib.EPI_OP16_GELU, tdt, lambda: gelu(ref)),
             ("relu", _lib.EPI_OP16_RELU, tdt, lambda: torch.relu(ref)), ("qk", _lib.EPI_OP16_QK, tdt, lambda: ref * qscale(N)),
             ("f32", _lib.EPI_F32, torch.float32, lambda: ref), ("resid", _lib.EPI_RESID, torch.float32, lambda: res[:M].double() + gamma.double() * ref)]
    for ename, epi, odt, want in cases:
        resid = epi == _lib.EPI_RESID

        def fresh():
            return (res.clone() if resid else torch.full((M + GUARD, N), 7.0, dtype=odt, device=dev()),)

        def launch(outs, t0, nt):
            o = outs[0]
            _lib.check(L.mhmr_gemm16(A.data_ptr() + t0 * 256 * K * 2, K, W.data_ptr(), K, nt * 256, N, K, bias.data_ptr(), gamma.data_ptr() if resid else None,
                                     o.data_ptr() + t0 * 256 * N * o.element_size(), N, None, 0, 128, 1, nt * 256, epi, dt, stream()), ename)

        (o,) = walk(f"plain[{nbn}-{cls}-{K}-{name}] {ename}", launch, fresh, R, max(1, G // nbn), lambda outs: [outs[0][:M]])
        gate(f"plain[{nbn}-{cls}-{K}-{name}] {ename}", o[:M], want(), tol if odt == tdt else 2e-5)
        assert same_bits(o[M:], res[M:]) if resid else bool(torch.all(o[M:] == 7.0)), "guard rows behind the matrix"
        del o


# ------------------------------------------------------------------------------------------------------ 2: V^T and patch layouts
@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@pytest.mark.parametrize("Tp,K", [(256, 128), (320, 384)])
def test_walk_vt_layout(L, name, dt, tdt, tol, Tp, K):
    """mhmr_gemm16 with the V^T epilogue, class A (N = 256: nbn = 1).  Tp = 256: one tile per image.  Tp = 320: a multiple of 64 but not of
    256, so tiles straddle images (a slab is then a multiple of four images = five tiles)."""
    G = ncus()
    H, N = 4, 256
    group = 1 if Tp == 256 else 4                             # images per whole number of tiles
    tiles_per = group * Tp // 256
    B = group * (G // tiles_per + 1)
    R = B * Tp // 256
    assert B * Tp % 256 == 0
    assert_class(R, G, "A")
    g = gen(Tp + K)
    A = randn(g, B * Tp, K).to(tdt)
    W = (randn(g, N, K) / math.sqrt(K)).to(tdt)
    bias = randn(g, N)
    ref = A.double() @ W.double().T + bias.double()

    def fresh():
        return (torch.full(((B + 1) * H, 64, Tp), 7.0, dtype=tdt, device=dev()),)              # one guard image

    def launch(outs, b0, nb):
        _lib.check(L.mhmr_gemm16(A.data_ptr() + b0 * Tp * K * 2, K, W.data_ptr(), K, nb * Tp, N, K, bias.data_ptr(), None,
                                 outs[0].data_ptr() + b0 * H * 64 * Tp * 2, 0, None, 0, Tp, H, nb * Tp, _lib.EPI_VT, dt, stream()), "vt")

    per = group * (G // tiles_per)
    (vt,) = walk(f"vt[{Tp}-{name}]", launch, fresh, B, per, lambda outs: [vt_logical(outs[0], B, H, Tp, Tp)])
    gate(f"vt[{Tp}-{K}-{name}]", vt_logical(vt, B, H, Tp, Tp), ref, tol)
    assert bool(torch.all(vt[B * H:] == 7.0)), "guard image"


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
def test_walk_patch_scatter(L, name, dt, tdt, tol):
    """mhmr_gemm16 with the patch epilogue, class A: Np = 320 (no multiple of 256), rows >= Mvalid dropped, the class / padding rows of
    every image and a guard image stay at the sentinel.  Slabs: multiples of four images = five tiles (m restarts at 0 in a launch)."""
    G = ncus()
    Np, Tp, N, K = 320, 384, 256, 128
    R = G + 1 if (G + 1) % 5 else G + 2
    assert_class(R, G, "A")
    M = 256 * R
    B = M // Np
    Mvalid = B * Np
    assert Mvalid < M
    g = gen(5)
    A = randn(g, M, K).to(tdt)
    W = (randn(g, N, K) / math.sqrt(K)).to(tdt)
    bias, pos = randn(g, N), randn(g, 1 + Np, N)
    ref = (A.double() @ W.double().T + bias.double())[:Mvalid].view(B, Np, N) + pos[1:].double()

    def fresh():
        return (torch.full(((B + 1) * Tp, N), 7.0, device=dev()),)

    def launch(outs, u0, nu):
        t0 = 5 * u0
        nt = min(5 * nu, R - t0)
        m0 = t0 * 256
        _lib.check(L.mhmr_gemm16(A.data_ptr() + m0 * K * 2, K, W.data_ptr(), K, nt * 256, N, K, bias.data_ptr(), None,
                                 outs[0].data_ptr() + (m0 // Np) * Tp * N * 4, N, pos.data_ptr(), Np, Tp, 2, max(0, min(Mvalid - m0, nt * 256)),
                                 _lib.EPI_PATCH, dt, stream()), "patch")

    def logical(outs):
        lg = torch.zeros(M, N, device=dev())
        lg[:Mvalid] = outs[0].view(B + 1, Tp, N)[:B, :Np].reshape(Mvalid, N)
        return [lg]

    (out,) = walk(f"patch[{name}]", launch, fresh, -(-R // 5), G // 5, logical)
    want = torch.zeros(M, N, dtype=torch.float64, device=dev())
    want[:Mvalid] = ref.reshape(Mvalid, N)
    gate(f"patch[{name}]", logical((out,))[0], want, 2e-5)
    got = out.view(B + 1, Tp, N)
    assert bool(torch.all(got[:B, Np:] == 7.0)) and bool(torch.all(got[B] == 7.0)), "class / padding rows, dropped rows"


# ------------------------------------------------------------------------------------------------------ 3: token-row map
@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@pytest.mark.parametrize("cls,K", [("A", 128), ("B", 384)])
def test_walk_token_row_map(L, name, dt, tdt, tol, cls, K):
    """mhmr_gemm16_ex under the row map: img_rows = 2304 (9 tiles per image: img_magic, a partial last round under the map), img_stride =
    2368, NaN in the skipped rows of A.  G = 256: 29 images = 261 tiles (A), 58 = 522 (B).  Slabs are whole images."""
    G = ncus()
    N, H, Tp = 256, 4, STRIDE
    B = (G // 9 + 1) * (1 if cls == "A" else 2)
    assert_class(9 * B, G, cls)
    g = gen(K + 9)
    A = randn(g, B * Tp, K).to(tdt)
    A.view(B, Tp, K)[:, NIMG:] = float("nan")
    W = (randn(g, N, K) / math.sqrt(K)).to(tdt)
    bias, gamma = randn(g, N), randn(g, N)
    res = randn(g, B + 1, Tp, N)
    ref = (A.view(B, Tp, K)[:, :NIMG].double() @ W.double().T + bias.double()).reshape(B * NIMG, N)

    def run(ename, epi, fresh, obytes, ldo, logical, want, gtol):
        def launch(outs, b0, nb):
            _lib.check(L.mhmr_gemm16_ex(A.data_ptr() + b0 * Tp * K * 2, K, W.data_ptr(), K, nb * NIMG, N, K, bias.data_ptr(),
                                        gamma.data_ptr() if epi == _lib.EPI_RESID else None, outs[0].data_ptr() + b0 * Tp * N * obytes, ldo, None, 0,
                                        Tp, H, nb * NIMG, epi, dt, NIMG, Tp, 0, stream()), ename)
        (o,) = walk(f"rowmap[{cls}-{name}] {ename}", launch, fresh, B, G // 9, logical)
        gate(f"rowmap[{cls}-{K}-{name}] {ename}", logical((o,))[0], want, gtol)
        return o

    rows = lambda outs: [outs[0][:B, :NIMG].reshape(B * NIMG, N)]
    f16 = lambda: (torch.full((B + 1, Tp, N), 7.0, dtype=tdt, device=dev()),)
    for ename, epi, want in (("op16", _lib.EPI_OP16, ref), ("gelu", _lib.EPI_OP16_GELU, gelu(ref))):
        o = run(ename, epi, f16, 2, N, rows, want, tol)
        assert bool(torch.all(o[:B, NIMG:] == 7.0)) and bool(torch.all(o[B] == 7.0)), "skipped rows / guard image"
    o = run("resid", _lib.EPI_RESID, lambda: (res.clone(),), 4, N, rows, res[:B, :NIMG].reshape(B * NIMG, N).double() + gamma.double() * ref, 2e-5)
    assert same_bits(o[:B, NIMG:], res[:B, NIMG:]) and same_bits(o[B], res[B]), "skipped rows / guard image"
    # V^T: out + b0 * Tp * N elements is also image b0 of [B, H, 64, Tp] (H * 64 = N)
    vt = run("vt", _lib.EPI_VT, lambda: (torch.full(((B + 1) * H, 64, Tp), 7.0, dtype=tdt, device=dev()),), 2, 0,
             lambda outs: [vt_logical(outs[0], B, H, Tp, NIMG)], ref, tol)
    assert bool(torch.all(vt[: B * H, :, NIMG:] == 7.0)) and bool(torch.all(vt[B * H:] == 7.0)), "skipped token columns / guard image"


# ------------------------------------------------------------------------------------------------------ 4: LayerNorm fold
def _fold_rows(G, nbn, cls, mapped):
    """-> images B, row pitch of an image Tp, rows per image T (logical), slab size in images."""
    if mapped:
        return mapped_images(G, nbn, cls), STRIDE, NIMG, max(1, G // (9 * nbn))
    return walk_rows(G, nbn, cls), 256, 256, max(1, G // nbn)


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("cls", ["A", "B"])
@pytest.mark.parametrize("K", [256, 384])
def test_walk_layernorm_fold_producer(L, name, dt, tdt, tol, K, cls, mapped):
    """mhmr_gemm16_ln, the residual epilogue that also leaves x16 and the block sums (N = 768: nbn = 3), over all rows and under the row
    map of test_walk_token_row_map (one image = one 256-row tile otherwise)."""
    G = ncus()
    N, nbn = 768, 3
    B, Tp, T, per = _fold_rows(G, nbn, cls, mapped)
    H, M, P = N // 64, B * T, B * Tp
    g = gen(K + 2 * mapped + (cls == "B"))
    att = randn(g, P, K).to(tdt)
    att.view(B, Tp, K)[:, T:] = float("nan")
    Wp = (randn(g, N, K) / math.sqrt(K)).to(tdt)
    bp, gamma = randn(g, N), randn(g, N)
    res = randn(g, P + GUARD, N) * 2.0 + 0.3
    valid = torch.zeros(P + GUARD, dtype=torch.bool, device=dev())
    valid[:P].view(B, Tp)[:, :T] = True
    ref = res[valid].double() + gamma.double() * (att.view(B, Tp, K)[:, :T].reshape(M, K).double() @ Wp.double().T + bp.double())

    def fresh():
        return (res.clone(), torch.full((P + GUARD, N), 7.0, dtype=tdt, device=dev()), torch.full((P + GUARD, N // 64, 2), -1.0, device=dev()))

    def launch(outs, b0, nb):
        r0 = b0 * Tp
        _lib.check(L.mhmr_gemm16_ln(att.data_ptr() + r0 * K * 2, K, Wp.data_ptr(), K, nb * T, N, K, bp.data_ptr(), gamma.data_ptr(),
                                    outs[0].data_ptr() + r0 * N * 4, N, Tp, H, _lib.EPI_RESID, dt, T if mapped else 0, Tp if mapped else 0, 0,
                                    outs[1].data_ptr() + r0 * N * 2, outs[2].data_ptr() + r0 * (N // 64) * 8, None, None, None, stream()), "producer")

    label = f"producer[{K}-{cls}-{'map' if mapped else 'all'}-{name}]"
    out, x16, pst = walk(label, launch, fresh, B, per, lambda outs: [outs[0][valid], outs[1][valid], outs[2][valid].reshape(M, -1)])
    gate(label + " out", out[valid], ref, 2e-5)
    assert same_bits(out[~valid], res[~valid]), "skipped / guard rows of the residual"
    assert same_bits(x16[valid], out[valid].to(tdt)), ("x16 is not the rounded residual", bad_tiles(x16[valid], out[valid].to(tdt)))
    assert bool(torch.all(x16[~valid] == 7.0)) and bool(torch.all(pst[~valid] == -1.0)), "skipped / guard rows of x16 / pstats"
    blocks = out[valid].double().view(M, N // 64, 64)
    gate(label + " sums", pst[valid][..., 0], blocks.sum(-1), 1e-5)
    gate(label + " squares", pst[valid][..., 1], (blocks * blocks).sum(-1), 1e-5)


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("cls", ["A", "B"])
@pytest.mark.parametrize("K", [256, 384])
@pytest.mark.parametrize("ename,N", [("gelu", 4096), ("qk", 2048), ("vt", 768)])
def test_walk_layernorm_fold_consumers(L, name, dt, tdt, tol, ename, N, K, cls, mapped):
    """mhmr_gemm16_ln, the consumers whose (colsum, fbias, mean, rstd) strip of tile r + 1 is LDS-DMA'd during the last k pair of tile r + 1
    while other waves may still be in the epilogue of tile r, which read the strip (K = 256: exactly one barrier-separated k pair between
    them).  Rows x = s_m z + mu_m with s_m in [1, 3], mu_m in [-0.5, 0.5] random PER ROW, (mean, rstd) taken from the fp32 rows as
    mhmr_ln_stats leaves them -- distinct per row, and the comparison with the real LayerNorm + linear keeps test_layernorm_fold's gate
    (|mu| / s <= 0.5 inflates the 16-bit rounding of the raw rows by at most sqrt(1.25) against unit rows)."""
    G = ncus()
    epi = {"gelu": _lib.EPI_OP16_GELU, "qk": _lib.EPI_OP16_QK, "vt": _lib.EPI_VT}[ename]
    nbn = N // 256
    B, Tp, T, per = _fold_rows(G, nbn, cls, mapped)
    H, M, P = N // 64, B * T, B * Tp
    g = gen(N + K + 2 * mapped + (cls == "B"))
    valid = torch.zeros(P, dtype=torch.bool, device=dev())
    valid.view(B, Tp)[:, :T] = True
    x = randn(g, P, K) * (1.0 + 2.0 * rand(g, P, 1)) + (rand(g, P, 1) - 0.5)
    rowstats = torch.stack([x.double().mean(-1), 1.0 / torch.sqrt(x.double().var(-1, unbiased=False) + 1e-6)], 1).float().contiguous()
    x16 = x.to(tdt)
    x16[~valid] = float("nan")
    rowstats[~valid] = float("nan")
    ln_w, ln_b = 1.0 + 0.2 * randn(g, K), 0.1 * randn(g, K)
    W, b = randn(g, N, K) / math.sqrt(K), randn(g, N)
    Wf = (W * ln_w).to(tdt)
    colsum = Wf.double().sum(1).float()
    fb = (b.double() + W.double() @ ln_b.double()).float()
    rs = rowstats[valid].double()
    want = rs[:, 1:2] * (x16[valid].double() @ Wf.double().T - rs[:, 0:1] * colsum.double()) + fb.double()                   # the kernel's formula
    true = torch.nn.functional.layer_norm(x[valid], (K,), ln_w, ln_b, 1e-6).double() @ W.double().T + b.double()          # what it stands for
    if ename == "gelu":
        want, true = gelu(want), gelu(true)
    elif ename == "qk":
        want, true = want * qscale(N), true * qscale(N)
    vtf = ename == "vt"

    def fresh():
        return (torch.full(((B + 1) * H, 64, Tp) if vtf else (P + GUARD, N), 7.0, dtype=tdt, device=dev()),)

    def launch(outs, b0, nb):
        r0 = b0 * Tp
        _lib.check(L.mhmr_gemm16_ln(x16.data_ptr() + r0 * K * 2, K, Wf.data_ptr(), K, nb * T, N, K, None, None, outs[0].data_ptr() + r0 * N * 2,
                                    0 if vtf else N, Tp, H, epi, dt, T if mapped else 0, Tp if mapped else 0, 0, None, None,
                                    rowstats.data_ptr() + r0 * 8, colsum.data_ptr(), fb.data_ptr(), stream()), ename)

    logical = (lambda outs: [vt_logical(outs[0], B, H, Tp, T)]) if vtf else (lambda outs: [outs[0][:P][valid]])
    label = f"consumer[{ename}-{N}-{K}-{cls}-{'map' if mapped else 'all'}-{name}]"
    (o,) = walk(label, launch, fresh, B, per, logical)
    got = logical((o,))[0]
    gate(label, got, want, tol)                                                    # same 16-bit operands: accumulation order + output rounding
    gate(label + " vs LayerNorm + linear", got, true, FOLD_TRUE_TOL[name], rel)
    if vtf:
        assert bool(torch.all(o[: B * H, :, T:] == 7.0)) and bool(torch.all(o[B * H:] == 7.0)), "skipped token columns / guard image"
    else:
        assert bool(torch.all(o[:P][~valid] == 7.0)) and bool(torch.all(o[P:] == 7.0)), "skipped / guard rows"


# ------------------------------------------------------------------------------------------------------ 5: low-half k ranges
@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
def test_walk_low_half_k_range(L, name, dt, tdt, tol):
    """mhmr_gemm16_ex with a_k = 128, K = 256 (the activation's k index wraps inside the handoff pair of every tile), residual and V^T
    epilogues, class A."""
    G = ncus()
    a_k, K, N, H, Tp = 128, 256, 256, 4, 256
    R = walk_rows(G, 1, "A")
    M = 256 * R
    g = gen(77)
    A = randn(g, M, a_k).to(tdt)
    W = randn(g, N, K) / math.sqrt(a_k)
    W[:, a_k:] *= 2.0 ** -11                                     # a low half's magnitude
    W = W.to(tdt)
    bias, gamma = randn(g, N), 0.5 + rand(g, N)
    res = randn(g, M + GUARD, N)
    ref = torch.cat([A, A], 1).double() @ W.double().T + bias.double()

    def launch_r(outs, t0, nt):
        _lib.check(L.mhmr_gemm16_ex(A.data_ptr() + t0 * 256 * a_k * 2, a_k, W.data_ptr(), K, nt * 256, N, K, bias.data_ptr(), gamma.data_ptr(),
                                    outs[0].data_ptr() + t0 * 256 * N * 4, N, None, 0, 128, 1, nt * 256, _lib.EPI_RESID, dt, 0, 0, a_k, stream()), "lo resid")

    (o,) = walk(f"lowhalf[{name}] resid", launch_r, lambda: (res.clone(),), R, G, lambda outs: [outs[0][:M]])
    gate(f"lowhalf[{name}] resid", o[:M], res[:M].double() + gamma.double() * ref, 2e-5)
    assert same_bits(o[M:], res[M:]), "guard rows"

    def launch_v(outs, t0, nt):
        _lib.check(L.mhmr_gemm16_ex(A.data_ptr() + t0 * 256 * a_k * 2, a_k, W.data_ptr(), K, nt * 256, N, K, bias.data_ptr(), None,
                                    outs[0].data_ptr() + t0 * H * 64 * Tp * 2, 0, None, 0, Tp, H, nt * 256, _lib.EPI_VT, dt, 0, 0, a_k, stream()), "lo vt")

    (vt,) = walk(f"lowhalf[{name}] vt", launch_v, lambda: (torch.full(((R + 1) * H, 64, Tp), 7.0, dtype=tdt, device=dev()),), R, G,
                 lambda outs: [vt_logical(outs[0], R, H, Tp, Tp)])
    gate(f"lowhalf[{name}] vt", vt_logical(vt, R, H, Tp, Tp), ref, tol)
    assert bool(torch.all(vt[R * H:] == 7.0)), "guard image"


@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
def test_walk_fp8_low_half(L, name, dt, tdt, tol):
    """mhmr_gemm16_lo8 at a_k = 256 (its smallest: one pair of 16-bit k tiles, then one pair of fp8 k tiles, which is the handoff pair),
    class A, after test_gemm_fp8_low_half_range: the residual epilogue with the pitched x16, its bf8 copy and the block sums, and the V^T
    epilogue plain and as a fold consumer -- against the term-by-term fp64 emulation of what the kernel multiplies.  The folded V^T keeps
    that test's 3e-3 for f16 (the hot channel of A makes acc - mean colsum a difference of larger terms)."""
    G = ncus()
    K, N, H, Tp = 256, 256, 4, 256
    R = walk_rows(G, 1, "A")
    M = 256 * R
    g = gen(88)
    A32 = randn(g, M, K)
    A32[:, 5] *= 60.0                                            # a massive-activation channel: bf8 (e5m2) has the range for it
    W32 = randn(g, N, K) * 0.03
    A16, A8 = A32.to(tdt), A32.to(torch.float8_e5m2)
    Arow = torch.cat([A16.view(torch.uint8).reshape(M, 2 * K), A8.view(torch.uint8)], 1).contiguous()          # [M, 3K] bytes
    W16 = W32.to(tdt)
    Wrow, scale, lo_deq = vit.lo8_rows(W16.cpu(), W32.cpu())          # (a 256 x 256 weight: packed on the host like the model's)
    Wrow, lo_deq = Wrow.to(dev()), lo_deq.to(dev())
    emul = A16.double() @ W16.double().T + A8.float().double() @ lo_deq.T
    bias, gamma = randn(g, N), 0.5 + rand(g, N)
    ld, pit = K + K // 2, N + N // 2
    res = randn(g, M + GUARD, N)

    def fresh():
        return (res.clone(), torch.full((M + GUARD, pit), 7.0, dtype=tdt, device=dev()), torch.full((M + GUARD, N // 64, 2), -1.0, device=dev()))

    def launch_r(outs, t0, nt):
        r0 = t0 * 256
        _lib.check(L.mhmr_gemm16_lo8(Arow.data_ptr() + r0 * 3 * K, ld, Wrow.data_ptr(), ld, nt * 256, N, K, 1, scale, bias.data_ptr(), gamma.data_ptr(),
                                     outs[0].data_ptr() + r0 * N * 4, N, 128, 1, _lib.EPI_RESID, dt, 0, 0, outs[1].data_ptr() + r0 * pit * 2, pit, 2 * N,
                                     outs[2].data_ptr() + r0 * (N // 64) * 8, None, None, None, stream()), "lo8 resid")

    def x8_of(x16):
        return x16[:M].contiguous().view(torch.uint8).reshape(M, 2 * pit)[:, 2 * N:3 * N].contiguous()

    out, x16, pst = walk(f"lo8[{name}] resid", launch_r, fresh, R, G,
                         lambda outs: [outs[0][:M], outs[1][:M, :N], x8_of(outs[1]).float(), outs[2][:M].reshape(M, -1)])
    gate(f"lo8[{name}] resid", out[:M], res[:M].double() + gamma.double() * (emul + bias.double()), 2e-5)
    assert same_bits(out[M:], res[M:]) and bool(torch.all(x16[M:] == 7.0)) and bool(torch.all(pst[M:] == -1.0)), "guard rows"
    assert same_bits(x16[:M, :N], out[:M].to(tdt)), ("x16 is not the rounded residual", bad_tiles(x16[:M, :N], out[:M].to(tdt)))
    x8 = x8_of(x16)
    want8 = out[:M].to(torch.float8_e5m2)
    assert float((x8 == want8.view(torch.uint8)).float().mean()) > 0.999
    assert float((x8.view(torch.float8_e5m2).float() - out[:M]).abs().max() / out[:M].abs().max()) < 0.13
    blocks = out[:M].double().view(M, N // 64, 64)
    gate(f"lo8[{name}] sums", pst[:M, :, 0], blocks.sum(-1), 1e-5)
    gate(f"lo8[{name}] squares", pst[:M, :, 1], (blocks * blocks).sum(-1), 1e-5)
    # V^T, plain and as the consumer of a folded LayerNorm
    rs = torch.stack([randn(g, M) * 0.3, 0.5 + rand(g, M)], 1).contiguous()
    colsum = (W16.double().sum(1) + lo_deq.sum(1)).float().contiguous()
    for fold in (False, True):
        def launch_v(outs, t0, nt):
            r0 = t0 * 256
            st = (rs.data_ptr() + r0 * 8, colsum.data_ptr(), bias.data_ptr()) if fold else (None, None, None)
            _lib.check(L.mhmr_gemm16_lo8(Arow.data_ptr() + r0 * 3 * K, ld, Wrow.data_ptr(), ld, nt * 256, N, K, 1, scale, None if fold else bias.data_ptr(), None,
                                         outs[0].data_ptr() + t0 * H * 64 * Tp * 2, 0, Tp, H, _lib.EPI_VT, dt, 0, 0, None, 0, 0, None, *st, stream()), "lo8 vt")

        label = f"lo8[{name}] vt{' fold' if fold else ''}"
        (vt,) = walk(label, launch_v, lambda: (torch.full(((R + 1) * H, 64, Tp), 7.0, dtype=tdt, device=dev()),), R, G,
                     lambda outs: [vt_logical(outs[0], R, H, Tp, Tp)])
        want = (rs[:, 1:2].double() * (emul - rs[:, 0:1].double() * colsum.double()) + bias.double()) if fold else emul + bias.double()
        gate(label, vt_logical(vt, R, H, Tp, Tp), want, max(tol, 3e-3) if fold else tol)
        assert bool(torch.all(vt[R * H:] == 7.0)), "guard image"


# ------------------------------------------------------------------------------------------------------ 6: masked output width
@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
def test_walk_masked_width(L, name, dt, tdt, tol):
    """mhmr_gemm16_masked: N = 512 with n_valid = 384, R = G / 2 + 1 row tiles (class A; every second tile of a workgroup's walk has a dead
    half): the residual epilogue with the producer outputs at the real width, and the V^T epilogue plain and folded (strip handoff);
    a guard row tile / guard image, and nothing behind column 384 / head 6 (the outputs have the real width, so a store there lands in
    the next row or head and fails (a))."""
    G = ncus()
    Nv, Np, Tp, K = 384, 512, 256, 384
    R = walk_rows(G, 2, "A")
    M, B, H = 256 * R, R, Nv // 64
    g = gen(66)
    A = randn(g, M, K).to(tdt)

    def padded(t):
        return torch.cat([t, torch.zeros(Np - Nv, *t.shape[1:], dtype=t.dtype, device=t.device)], 0).contiguous()

    W = (randn(g, Nv, K) / math.sqrt(K)).to(tdt)
    bias, gamma = randn(g, Nv), 0.5 + rand(g, Nv)
    Wp, bp, gp = padded(W), padded(bias), padded(gamma)
    lin = A.double() @ W.double().T
    res = randn(g, M + GUARD, Nv)

    def fresh():
        return (res.clone(), torch.full((M + GUARD, Nv), 7.0, dtype=tdt, device=dev()), torch.full((M + GUARD, Nv // 64, 2), -1.0, device=dev()))

    def launch_r(outs, t0, nt):
        r0 = t0 * 256
        _lib.check(L.mhmr_gemm16_masked(A.data_ptr() + r0 * K * 2, K, Wp.data_ptr(), K, nt * 256, Np, Nv, K, 0, bp.data_ptr(), gp.data_ptr(),
                                        outs[0].data_ptr() + r0 * Nv * 4, Nv, Tp, H, _lib.EPI_RESID, dt, outs[1].data_ptr() + r0 * Nv * 2,
                                        outs[2].data_ptr() + r0 * (Nv // 64) * 8, None, None, None, stream()), "masked resid")

    out, x16, pst = walk(f"masked[{name}] resid", launch_r, fresh, R, G // 2, lambda outs: [outs[0][:M], outs[1][:M], outs[2][:M].reshape(M, -1)])
    gate(f"masked[{name}] resid", out[:M], res[:M].double() + gamma.double() * (lin + bias.double()), 2e-5)
    assert same_bits(out[M:], res[M:]) and bool(torch.all(x16[M:] == 7.0)) and bool(torch.all(pst[M:] == -1.0)), "guard rows"
    assert same_bits(x16[:M], out[:M].to(tdt)), ("x16 is not the rounded residual", bad_tiles(x16[:M], out[:M].to(tdt)))
    blocks = out[:M].double().view(M, Nv // 64, 64)
    gate(f"masked[{name}] sums", pst[:M, :, 0], blocks.sum(-1), 1e-5)
    gate(f"masked[{name}] squares", pst[:M, :, 1], (blocks * blocks).sum(-1), 1e-5)
    rs = torch.stack([randn(g, M) * 0.3, 0.5 + rand(g, M)], 1).contiguous()
    colsum = padded(W.double().sum(1).float())
    for fold in (False, True):
        def launch_v(outs, t0, nt):
            r0 = t0 * 256
            st = (rs.data_ptr() + r0 * 8, colsum.data_ptr(), bp.data_ptr()) if fold else (None, None, None)
            _lib.check(L.mhmr_gemm16_masked(A.data_ptr() + r0 * K * 2, K, Wp.data_ptr(), K, nt * 256, Np, Nv, K, 0, None if fold else bp.data_ptr(), None,
                                            outs[0].data_ptr() + t0 * H * 64 * Tp * 2, 0, Tp, H, _lib.EPI_VT, dt, None, None, *st, stream()), "masked vt")

        label = f"masked[{name}] vt{' fold' if fold else ''}"
        (vt,) = walk(label, launch_v, lambda: (torch.full(((B + 1) * H, 64, Tp), 7.0, dtype=tdt, device=dev()),), R, G // 2,
                     lambda outs: [vt_logical(outs[0], B, H, Tp, Tp)])
        want = (rs[:, 1:2].double() * (lin - rs[:, 0:1].double() * W.double().sum(1)) + bias.double()) if fold else lin + bias.double()
        gate(label, vt_logical(vt, B, H, Tp, Tp), want, tol)
        assert bool(torch.all(vt[B * H:] == 7.0)), "guard image"


# ------------------------------------------------------------------------------------------------------ 7: merged qkv
@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
def test_walk_merged_qkv(L, name, dt, tdt, tol, fold):
    """mhmr_qkv16 at C = 256 (three column tiles: Q, K, V), B Tp / 256 = G / 3 + 1 row tiles (86 at G = 256: 258 tiles, class A).  The
    entry takes more than one round of tiles, so the walk itself is tested (qk, the row-major V scratch and the transposed V)."""
    G = ncus()
    C, H, Tp = 256, 4, 256
    B = walk_rows(G, 3, "A")
    M = B * Tp
    g = gen(11 + fold)
    A = randn(g, M, C).to(tdt)
    W = (randn(g, 3 * C, C) / math.sqrt(C)).to(tdt)
    b = randn(g, 3 * C)
    rs = torch.stack([randn(g, M) * 0.3, 0.5 + rand(g, M)], 1).contiguous()
    colsum = W.double().sum(1).float().contiguous()

    def fresh():
        return tuple(torch.full(s, 7.0, dtype=tdt, device=dev()) for s in ((M + GUARD, 2 * C), (M + GUARD, C), ((B + 1) * H, 64, Tp)))

    def launch(outs, b0, nb):
        r0 = b0 * Tp
        st = (rs.data_ptr() + r0 * 8, colsum.data_ptr(), b.data_ptr()) if fold else (None, None, None)
        _lib.check(L.mhmr_qkv16(A.data_ptr() + r0 * C * 2, C, W.data_ptr(), C, nb, Tp, C, H, None if fold else b.data_ptr(), outs[0].data_ptr() + r0 * 2 * C * 2,
                                outs[1].data_ptr() + r0 * C * 2, outs[2].data_ptr() + b0 * H * 64 * Tp * 2, dt, *st, stream()), "qkv16")

    label = f"qkv[{'fold' if fold else 'plain'}-{name}]"
    qk, v16, vt = walk(label, launch, fresh, B, G // 3, lambda outs: [outs[0][:M], outs[1][:M], vt_logical(outs[2], B, H, Tp, Tp)])
    lin = A.double() @ W.double().T
    want = (rs[:, 1:2].double() * (lin - rs[:, 0:1].double() * colsum.double()) + b.double()) if fold else lin + b.double()
    want[:, :C] *= _lib.ATTN_QSCALE
    gate(label + " qk", qk[:M], want[:, :2 * C], tol)
    gate(label + " v", v16[:M], want[:, 2 * C:], tol)
    gate(label + " vt", vt_logical(vt, B, H, Tp, Tp), want[:, 2 * C:], tol)
    assert bool(torch.all(qk[M:] == 7.0)) and bool(torch.all(v16[M:] == 7.0)) and bool(torch.all(vt[B * H:] == 7.0)), "guard rows / guard image"


# ------------------------------------------------------------------------------------------------------ 8: staggered start
@pytest.mark.parametrize("name,dt,tdt,tol", DTYPES)
def test_walk_staggered_residual(L, name, dt, tdt, tol):
    """The residual epilogue over all rows with >= 1024 tiles (N = 1024, R = G + 1: 1028 tiles at G = 256, four full rounds + four tiles):
    the launcher sets stagger_ticks and the CU quarters start late.  K = 128.  The slab launches (G tiles each) are not staggered."""
    G = ncus()
    N, K, R = 1024, 128, G + 1
    M = 256 * R
    g = gen(8)
    A = randn(g, M, K).to(tdt)
    W = (randn(g, N, K) / math.sqrt(K)).to(tdt)
    bias, gamma = randn(g, N), randn(g, N)
    res = randn(g, M + GUARD, N)

    def launch(outs, t0, nt):
        _lib.check(L.mhmr_gemm16(A.data_ptr() + t0 * 256 * K * 2, K, W.data_ptr(), K, nt * 256, N, K, bias.data_ptr(), gamma.data_ptr(),
                                 outs[0].data_ptr() + t0 * 256 * N * 4, N, None, 0, 128, 1, nt * 256, _lib.EPI_RESID, dt, stream()), "stagger")

    (o,) = walk(f"stagger[{name}]", launch, lambda: (res.clone(),), R, G // 4, lambda outs: [outs[0][:M]])
    gate(f"stagger[{name}]", o[:M], res[:M].double() + gamma.double() * (A.double() @ W.double().T + bias.double()), 2e-5)
    assert same_bits(o[M:], res[M:]), "guard rows"
