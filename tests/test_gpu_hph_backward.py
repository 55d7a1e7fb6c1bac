"""-m gpu: the backward of the person-head decoder (csrc/hph_bwd.hip) against float64 torch on the operands the
kernels see.  Gate: the 4x rule of DESIGN.md section 16 -- for every gradient tensor separately the kernel's maximum absolute error
against fp64 is at most 4x that of the same computation in fp32 torch on the CPU (tests/hph_bwd_oracle.py).  Every test prints kernel
error, yardstick and ratio per tensor before it asserts."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import hph_bwd_oracle as ho  # noqa: E402
from multi_hmr_amd import _lib  # noqa: E402

SCALE = 32 ** -0.5
ACTS = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "gelu": _lib.ACT_GELU}


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


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())


def rn(g, *shape, std=1.0):
    return torch.empty(*shape).normal_(0, 1, generator=g) * std


def report(tag, rows):
    """rows: (tensor name, (err, yard, ratio, ok)).  Print all, then assert all."""
    for name, (err, yard, ratio, ok) in rows:
        print(f"[{tag}] {name}: kernel {err:.3e} yardstick {yard:.3e} ratio {ratio:.2f}{'' if ok else '  <-- FAILS'}")
    bad = [name for name, r in rows if not r[3]]
    assert not bad, (tag, bad)


def _act(z, act):
    return z if act == "none" else F.relu(z) if act == "relu" else F.gelu(z)


# ------------------------------------------------------------------------------------------------------ (1) building blocks
def _linear_ref(dY, Z, W, X, act, dtype):
    """dX, dW, db of Y = act(Z) with Z TAKEN AS GIVEN (the taped pre-activation), in `dtype` through autograd."""
    z = Z.to(dtype).requires_grad_()
    (dZ,) = torch.autograd.grad((_act(z, act) * dY.to(dtype)).sum(), z)
    return dZ @ W.to(dtype), dZ.T @ X.to(dtype), dZ.sum(0)


@pytest.mark.parametrize("act", ["none", "relu", "gelu"])
@pytest.mark.parametrize("NK", [(2, 384), (352, 1024), (1024, 256)])
def test_linear_backward(L, NK, act):
    """M in {1, 17, 130}; input side with and without residual cotangent and row gather; weight side with the fp64 bias sum.  Outputs
    are NaN-filled first: every element is written."""
    N, K = NK
    g = torch.Generator().manual_seed(100 + N + len(act))
    rows = []
    for M in (1, 17, 130):
        Mbig = M + 5
        W, X = rn(g, N, K, std=K ** -0.5), rn(g, Mbig, K)
        Zall, dYall, dR = rn(g, Mbig, N), rn(g, Mbig, N), rn(g, M, K)
        idx = torch.randperm(Mbig, generator=g)[:M]
        for gather, resid in ((False, False), (True, True)):
            sel = idx if gather else torch.arange(M)
            dX64, dW64, db64 = _linear_ref(dYall[sel], Zall[sel], W, X[:M], act, torch.float64)
            dX32, dW32, db32 = _linear_ref(dYall[sel], Zall[sel], W, X[:M], act, torch.float32)
            if resid:
                dX64, dX32 = dX64 + dR.double(), dX32 + dR
            dYd, Zd, Wd, Xd, dRd = (t.to(dev()).contiguous() for t in (dYall, Zall, W, X, dR))
            if not gather:
                dYd, Zd = dYd[:M].contiguous(), Zd[:M].contiguous()
            dX, dW, db, idx_d = nan(M, K), nan(N, K), nan(N), i32(idx.tolist())
            _lib.check(L.mhmr_linear_f32_backward_input(dYd.data_ptr(), N, idx_d.data_ptr() if gather else None, Zd.data_ptr(), N,
                                                        Wd.data_ptr(), K, dRd.data_ptr() if resid else None, K, dX.data_ptr(), K, M, N, K,
                                                        ACTS[act], stream()), "mhmr_linear_f32_backward_input")
            tag = f"M {M}{' gather+resid' if gather else ''}"
            rows.append((f"dX {tag}", ho.four_x(dX, dX64, dX32)))
            if not gather:
                _lib.check(L.mhmr_linear_f32_backward_weight(dYd.data_ptr(), N, Zd.data_ptr(), N, Xd.data_ptr(), K, dW.data_ptr(), K,
                                                             db.data_ptr(), M, N, K, ACTS[act], stream()), "mhmr_linear_f32_backward_weight")
                rows.append((f"dW {tag}", ho.four_x(dW, dW64, dW32)))
                rows.append((f"db {tag}", ho.four_x(db, db64, db32)))
    report(f"linear bwd N {N} K {K} {act}", rows)


@pytest.mark.parametrize("C_", [64, 1024, 2048])
def test_layernorm_backward(L, C_):
    g = torch.Generator().manual_seed(200 + C_)
    rows = []
    for R in (1, 5, 130):
        x, w, b, dy, dR = rn(g, R, C_) * 2 + 0.3, 1 + 0.1 * rn(g, C_), 0.05 * rn(g, C_), rn(g, R, C_), rn(g, R, C_)

        def ref(dtype):
            xx, ww, bb = x.to(dtype).requires_grad_(), w.to(dtype).requires_grad_(), b.to(dtype).requires_grad_()
            gx, gw, gb = torch.autograd.grad((F.layer_norm(xx, (C_,), ww, bb, 1e-5) * dy.to(dtype)).sum(), (xx, ww, bb))
            return gx + dR.to(dtype), gw, gb
        r64, r32 = ref(torch.float64), ref(torch.float32)
        nbytes = L.mhmr_layernorm_f32_backward_workspace_bytes(R, C_)
        assert nbytes > 0
        ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev())
        dx, dw, db = nan(R, C_), nan(C_), nan(C_)
        xd, wd, dyd, dRd = (t.to(dev()).contiguous() for t in (x, w, dy, dR))
        _lib.check(L.mhmr_layernorm_f32_backward(xd.data_ptr(), wd.data_ptr(), dyd.data_ptr(), dRd.data_ptr(), dx.data_ptr(), dw.data_ptr(),
                                                 db.data_ptr(), R, C_, 1e-5, ws.data_ptr(), nbytes, stream()), "mhmr_layernorm_f32_backward")
        for name, got, a, b_ in zip(("dx", "dgamma", "dbeta"), (dx, dw, db), r64, r32):
            rows.append((f"{name} rows {R}", ho.four_x(got, a, b_)))
    report(f"layernorm bwd C {C_}", rows)


def _attn(q, k, v):
    return torch.softmax(q @ k.T * SCALE, dim=-1) @ v


@pytest.mark.parametrize("heads", [8, 16])
def test_self_attention_backward(L, heads):
    """Groups (1, 0, 65, 130): a group of one, an empty group (a repeated gstart entry), two and three query tiles."""
    inner, counts = 32 * heads, (1, 0, 65, 130)
    P = sum(counts)
    g = torch.Generator().manual_seed(300 + heads)
    qkv, dO = rn(g, P, 3 * inner, std=1.5), rn(g, P, inner)
    gstart = [0]
    for c in counts:
        gstart.append(gstart[-1] + c)

    def ref(dtype):
        t = qkv.to(dtype).requires_grad_()
        s = 0
        for a, b in zip(gstart[:-1], gstart[1:]):
            for h in range(heads):
                c = slice(h * 32, h * 32 + 32)
                o = _attn(t[a:b, c], t[a:b, inner:][:, c], t[a:b, 2 * inner:][:, c])
                s = s + (o * dO[a:b, c].to(dtype)).sum()
        return torch.autograd.grad(s, t)[0]
    r64, r32 = ref(torch.float64), ref(torch.float32)
    dqkv, lse = nan(P, 3 * inner), nan(P, heads, 2)
    qkv_d, dO_d, gs_d = qkv.to(dev()), dO.to(dev()), i32(gstart)
    _lib.check(L.mhmr_hph_self_attn_backward(qkv_d.data_ptr(), dO_d.data_ptr(), gs_d.data_ptr(), dqkv.data_ptr(),
                                             lse.data_ptr(), len(counts), max(counts), heads, stream()), "mhmr_hph_self_attn_backward")
    report(f"self-attn bwd heads {heads}", [(n, ho.four_x(dqkv[:, i * inner:(i + 1) * inner], r64[:, i * inner:(i + 1) * inner],
                                                           r32[:, i * inner:(i + 1) * inner])) for i, n in enumerate(("dq", "dk", "dv"))])


def _cross_attention_case(L, N, heads, counts):
    """Work items of at most 8 queries per image plus two count-0 padding items at the tail; dq, dk, dv under the 4x rule, the dkv rows of
    images without queries exact zeros; -> the number of work items."""
    inner, B, P = 32 * heads, len(counts), sum(counts)
    g = torch.Generator().manual_seed(400 + N)
    q, kv, dO = rn(g, P, inner, std=1.5), rn(g, B * N, 2 * inner, std=1.5), rn(g, P, inner)
    chunks, start = [], 0
    for b, c in enumerate(counts):
        for q0 in range(0, c, 8):
            chunks += [b, start + q0, min(8, c - q0)]
        start += c
    chunks += [0, 0, 0] * 2

    def ref(dtype):
        qq, kk = q.to(dtype).requires_grad_(), kv.to(dtype).requires_grad_()
        s, a = 0, 0
        for b, c in enumerate(counts):
            for h in range(heads):
                cs = slice(h * 32, h * 32 + 32)
                o = _attn(qq[a:a + c, cs], kk[b * N:(b + 1) * N, :inner][:, cs], kk[b * N:(b + 1) * N, inner:][:, cs])
                s = s + (o * dO[a:a + c, cs].to(dtype)).sum()
            a += c
        return torch.autograd.grad(s, (qq, kk))
    r64, r32 = ref(torch.float64), ref(torch.float32)
    dq, dkv, lse = nan(P, inner), nan(B * N, 2 * inner), nan(P, heads, 2)
    q_d, kv_d, dO_d, ch_d = q.to(dev()), kv.to(dev()), dO.to(dev()), i32(chunks)
    _lib.check(L.mhmr_hph_cross_attn_backward(q_d.data_ptr(), kv_d.data_ptr(), dO_d.data_ptr(), ch_d.data_ptr(),
                                              len(chunks) // 3, dq.data_ptr(), dkv.data_ptr(), lse.data_ptr(), heads, N, B, stream()),
               "mhmr_hph_cross_attn_backward")
    for b, c in enumerate(counts):
        if c == 0:
            assert bool((dkv[b * N:(b + 1) * N] == 0).all()), "rows of an image without queries are zeros"
    report(f"cross-attn bwd N {N} heads {heads} items {len(chunks) // 3}", [("dq", ho.four_x(dq, r64[0], r32[0])),
                                     ("dk", ho.four_x(dkv[:, :inner], r64[1][:, :inner], r32[1][:, :inner])),
                                     ("dv", ho.four_x(dkv[:, inner:], r64[1][:, inner:], r32[1][:, inner:]))])
    return len(chunks) // 3


@pytest.mark.parametrize("N", [64, 256, 4096])
def test_cross_attention_backward(L, N):
    """Counts (9, 0, 1, 17): full chunks, one-query tails, an image without queries and two count-0 padding items."""
    _cross_attention_case(L, N, 8, (9, 0, 1, 17))


def test_cross_attention_backward_more_than_512_work_items(L):
    """519 one-query images, an empty one and a last image of 9 queries: 523 work items with the padding, so the statistics and dq
    kernels take a second launch that starts at item 512 and holds one-query items, a full chunk, a one-query tail and the padding."""
    assert _cross_attention_case(L, 64, 2, (1,) * 519 + (0, 9)) == 523


def _one_hot_rows(P, heads, r):
    """dOut[q, h, :] one-hot at d = (q + h + r) % 32 -> (dOut [P, heads * 32], the flat column of the hot element per (q, h))."""
    q, h = torch.meshgrid(torch.arange(P), torch.arange(heads), indexing="ij")
    col = h * 32 + (q + h + r) % 32
    dO = torch.zeros(P, heads * 32)
    dO[q.reshape(-1), col.reshape(-1)] = 1.0
    return dO.to(dev()), col.to(dev())


def test_self_attention_backward_recomputes_the_forward_bits(L):
    """With a one-hot dOut row, D = dOut . O as the backward accumulates it IS the backward's own O[d] (zeros add exactly, 1 * x is exact
    under an FMA): lse_d[q, h, 1] must equal the forward's output element bit for bit, for every d.  Groups of 1, 3, 64 and 65 queries
    (65 crosses the 64-query block), 2 heads."""
    heads, counts = 2, (1, 3, 64, 65)
    inner, P = 32 * heads, sum(counts)
    g = torch.Generator().manual_seed(310)
    qkv_d = rn(g, P, 3 * inner, std=1.5).to(dev())
    gstart = [0]
    for c in counts:
        gstart.append(gstart[-1] + c)
    gs_d, out = i32(gstart), nan(P, inner)
    _lib.check(L.mhmr_hph_self_attn(qkv_d.data_ptr(), gs_d.data_ptr(), out.data_ptr(), len(counts), max(counts), heads, stream()),
               "mhmr_hph_self_attn")
    assert bool(torch.isfinite(out).all())
    for r in range(32):
        dO_d, col = _one_hot_rows(P, heads, r)
        dqkv, lse = nan(P, 3 * inner), nan(P, heads, 2)
        _lib.check(L.mhmr_hph_self_attn_backward(qkv_d.data_ptr(), dO_d.data_ptr(), gs_d.data_ptr(), dqkv.data_ptr(), lse.data_ptr(),
                                                 len(counts), max(counts), heads, stream()), "mhmr_hph_self_attn_backward")
        assert torch.equal(lse[:, :, 1], out.gather(1, col)), f"r {r}"


@pytest.mark.parametrize("N", [1, 7, 64, 65, 130])
def test_cross_attention_backward_recomputes_the_forward_bits(L, N):
    """The same identity for the cross-attention statistics kernel.  Two images, work items of 8, 1 and 5 queries, 2 heads; N = 1 and 7
    leave whole key slices and whole waves at m = -inf (the guarded branches of the two merges), 65 and 130 give uneven trips."""
    heads, counts = 2, (9, 5)
    inner, B, P = 32 * heads, len(counts), sum(counts)
    g = torch.Generator().manual_seed(410 + N)
    q_d, kv_d = rn(g, P, inner, std=1.5).to(dev()), rn(g, B * N, 2 * inner, std=1.5).to(dev())
    chunks = [0, 0, 8, 0, 8, 1, 1, 9, 5]
    ch_d, out = i32(chunks), nan(P, inner)
    _lib.check(L.mhmr_hph_cross_attn(q_d.data_ptr(), kv_d.data_ptr(), ch_d.data_ptr(), 3, out.data_ptr(), heads, N, stream()),
               "mhmr_hph_cross_attn")
    assert bool(torch.isfinite(out).all())
    for r in range(32):
        dO_d, col = _one_hot_rows(P, heads, r)
        dq, lse = nan(P, inner), nan(P, heads, 2)
        _lib.check(L.mhmr_hph_cross_attn_backward(q_d.data_ptr(), kv_d.data_ptr(), dO_d.data_ptr(), ch_d.data_ptr(), 3, dq.data_ptr(), None,
                                                  lse.data_ptr(), heads, N, B, stream()), "mhmr_hph_cross_attn_backward")
        assert torch.equal(lse[:, :, 1], out.gather(1, col)), f"r {r}"


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("Kc", [512, 1152])
def test_context_gemm(L, Kc, precision):
    """rows in {128, 1280, 4096} (1, 3 and 8 row slices) and 8300 (the 16-slice cap, a last MFMA step of fewer than four rows); NaN-filled
    output and workspace: every element is written, and the padding columns c >= cvalid are exact zeros."""
    tdt, Nn = ho.TDT[precision], 192
    cvalid = Kc if Kc == 512 else 1024 + 99
    g = torch.Generator().manual_seed(500 + Kc)
    rows_ = []
    for rows in (128, 1280, 4096, 8300):
        G, ctx = rn(g, rows, Nn), rn(g, rows, Kc).to(tdt)
        ctx[:, cvalid:] = 0
        r64 = G.double().T @ ctx.double()
        r32 = G.T @ ctx.float()
        nbytes = L.mhmr_grad_ctx_gemm_workspace_bytes(rows, Nn, Kc)
        assert nbytes > 0
        ws, dW = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev()), nan(Nn, Kc)
        G_d, ctx_d = G.to(dev()), ctx.to(dev())
        _lib.check(L.mhmr_grad_ctx_gemm(G_d.data_ptr(), Nn, ctx_d.data_ptr(), Kc, dW.data_ptr(), rows, Nn, Kc, cvalid,
                                        ho_dt(precision), ws.data_ptr(), nbytes, stream()), "mhmr_grad_ctx_gemm")
        assert bool(torch.isfinite(dW).all())
        assert bool((dW[:, cvalid:] == 0).all())
        rows_.append((f"dW rows {rows}", ho.four_x(dW, r64, r32)))
    report(f"ctx gemm Kc {Kc} {precision}", rows_)


def ho_dt(precision):
    return {"f16": _lib.DT_F16, "bf16": _lib.DT_BF16}[precision]


# ------------------------------------------------------------------------------------------------------ (2) the stack
_REF = {}


def _stack_ref(name, precision):
    """fp64 and fp32 oracle gradients, computed once per (case, precision) and left unchanged."""
    key = (name, precision)
    if key not in _REF:
        case = ho.stack_case(name)
        _REF[key] = (case, ho.stack_grads(case, precision, torch.float64), ho.stack_grads(case, precision, torch.float32))
    return _REF[key]


STACK_RUNS = [("small", "f16"), ("multihmr", "f16"), ("anny", "f16"), ("long", "f16"), ("small", "bf16"), ("multihmr", "bf16")]


@pytest.mark.parametrize("name,precision", STACK_RUNS)
def test_stack_through_differentiable(name, precision):
    """HPH.differentiable: forward values bit-equal to HPH.forward, the 4x rule on g_x and on every parameter, two backward calls give
    the same bits."""
    from multi_hmr_amd.anny_hph import HPH
    case, g64, g32 = _stack_ref(name, precision)
    m = HPH(dim=case["dim"], depth=case["depth"], heads=case["heads"], dim_head=32, mlp_dim=case["mlp"], dropout=0.0, precision=precision)
    m.load_state_dict(case["sd"], strict=True)
    m = m.to(dev()).eval()
    for p in m.parameters():
        p.requires_grad_(True)
    x, ctx, mask, cot = (case[k].to(dev()) for k in ("x", "context", "mask", "cot"))
    y0 = m(x, ctx, mask)

    def run():
        for p in m.parameters():
            p.grad = None
        xx = x.clone().requires_grad_()
        y = m.differentiable(xx, ctx, mask)
        assert torch.equal(y.detach(), y0), "forward values are those of HPH.forward, bit for bit"
        (y * cot).sum().backward()
        return {"x": xx.grad, **{k: p.grad for k, p in m.named_parameters()}}
    got, again = run(), run()
    assert set(got) == set(g64)
    for k in got:
        assert got[k] is not None and got[k].shape == g64[k].shape, k
        assert torch.equal(got[k], again[k]), f"{k}: two backward calls differ"
    rows = [(k, ho.four_x(got[k], g64[k], g32[k])) for k in got]
    worst = max(rows, key=lambda r: r[1][2])
    print(f"[stack {name} {precision}] worst ratio {worst[1][2]:.2f} at {worst[0]}")
    report(f"stack {name} {precision}", rows)


def test_stack_without_queries():
    """P == 0: the output is zeros and every gradient is zero (not None)."""
    from multi_hmr_amd.anny_hph import HPH
    m = HPH(dim=256, depth=1, heads=8, dim_head=32, mlp_dim=512, precision="f16").to(dev())
    for p in m.parameters():
        p.requires_grad_(True)
    x = torch.zeros(2, 3, 256, device=dev(), requires_grad=True)
    y = m.differentiable(x, torch.randn(2, 64, 256, device=dev()), torch.zeros(2, 3, device=dev()))
    assert bool((y == 0).all())
    y.sum().backward()
    assert bool((x.grad == 0).all()) and all(p.grad is not None and bool((p.grad == 0).all()) for p in m.parameters())


def test_differentiable_rejects_cpu_tensors():
    from multi_hmr_amd.anny_hph import HPH
    m = HPH(dim=256, depth=1, heads=8, dim_head=32, mlp_dim=512)
    with pytest.raises(_lib.MhmrError):
        m.differentiable(torch.zeros(1, 1, 256), torch.zeros(1, 64, 256))


def test_person_cotangents_do_not_depend_on_the_other_images():
    """Invariant: the cotangent of a person's query row (g_x here; g_zc / g_token in the model) -- self-attention is per image,
    cross-attention per image, linears and LayerNorms per row -- keeps its bits when another image with its own persons joins the batch.
    NOT invariant: the weight gradients, which are sums over all persons."""
    from multi_hmr_amd.anny_hph import HPH
    case = ho.stack_case("small")
    m = HPH(dim=case["dim"], depth=case["depth"], heads=case["heads"], dim_head=32, mlp_dim=case["mlp"], precision="f16")
    m.load_state_dict(case["sd"], strict=True)
    m = m.to(dev()).eval()
    for p in m.parameters():
        p.requires_grad_(True)
    x, ctx, mask, cot = (case[k].to(dev()) for k in ("x", "context", "mask", "cot"))      # counts (9, 0, 1, 17)

    def run(images):
        for p in m.parameters():
            p.grad = None
        xx = x[images].clone().requires_grad_()
        (m.differentiable(xx, ctx[images], mask[images]) * cot[images]).sum().backward()
        return xx.grad, m.transformer.layers[0][2].fn.net[0].weight.grad.clone()
    gx_alone, gw_alone = run([0])
    gx_both, gw_both = run([0, 3])
    assert torch.equal(gx_both[0], gx_alone[0])
    assert not torch.equal(gw_both, gw_alone)


# ------------------------------------------------------------------------------------------------------ (3) - (5) the whole head
import functools  # noqa: E402

S, GRID, NB, NAME = 224, 16, 10, "dinov2_vits14"


@functools.lru_cache(maxsize=None)
def _assets():
    import synthetic
    data, mean = synthetic.make_smplx_data(seed=0), synthetic.make_mean_params(seed=0)
    sd = synthetic.make_state_dict(NAME, S, seed=42, depth_override=4, mean_params=mean)
    return dict(data=data, mean=mean, sd=sd)


def _new_model():
    """A model of this module's own (the training step changes its parameters): ViT-S, 224^2, backbone depth 4, synthetic weights."""
    from multi_hmr_amd import Model
    a = _assets()
    m = Model(backbone=NAME, img_size=S, smplx_data=a["data"], mean_params=a["mean"], backbone_depth=4, precision="f16")
    m.load_state_dict(a["sd"], strict=True)
    return m.to(dev()).eval()


@functools.lru_cache(maxsize=None)
def _model():
    return _new_model().train_heads_(True)


def _scene(persons, seed):
    """Images, intrinsics and distinct cells for `persons` per image, sorted by (image, y, x) as torch.where leaves them."""
    g = torch.Generator().manual_seed(seed)
    B = len(persons)
    x = torch.randn(B, 3, S, S, generator=g)
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = torch.tensor([1.1 * S + 7 * b for b in range(B)])
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = S / 2 + 1.5, S / 2 - 2.0, 1.0
    bs, ys, xs = [], [], []
    for b, n in enumerate(persons):
        cells = sorted(torch.randperm(GRID * GRID, generator=g)[:n].tolist())
        bs += [b] * n
        ys += [c // GRID for c in cells]
        xs += [c % GRID for c in cells]
    return x, K, tuple(torch.tensor(v, dtype=torch.long) for v in (bs, ys, xs))


def _head_run(m, x, K, idx, cr, co):
    """forward(train_heads) + backward of sum(cr * readout) + sum(co * offset) -> (named gradients, g_zc, g_token, out)."""
    for p in m.parameters():
        p.grad = None
    out = m(x.to(dev()), idx=tuple(i.to(dev()) for i in idx), K=K.to(dev()), is_training=True, return_readout=True, train_heads=True)
    ((out["readout"] * cr.to(dev())).sum() + (out["offset"] * co.to(dev())).sum()).backward()
    named = {k: p.grad for k, p in m.named_parameters()}
    return named, m.heads_feature_grads["g_zc"], m.heads_feature_grads["g_token"], out


@pytest.mark.parametrize("persons", [(2, 1), (9, 0, 1)])
def test_whole_head_against_fp64(persons):
    """mhmr_hph_backward through Model: the 4x rule on every parameter of heads_parameters(), on g_zc and on g_token, with cotangents on
    the read-out and the offset together and each alone.  The oracle takes the device's feat32 and K as given."""
    from multi_hmr_amd.heads_train import head_parameter_names
    m, a = _model(), _assets()
    x, K, idx = _scene(persons, seed=700 + len(persons))
    Pn, Ndec = sum(persons), 318 + NB + 13
    g = torch.Generator().manual_seed(710)
    cr_all, co_all = rn(g, Pn, Ndec), rn(g, Pn, 2)
    names = head_parameter_names(2)
    assert set(names) == {k for k, _ in m.named_parameters() if k.startswith(("mlp_offset.", "x_attention_head."))}
    for which in ("both", "readout", "offset"):
        cr = cr_all if which != "offset" else torch.zeros_like(cr_all)
        co = co_all if which != "readout" else torch.zeros_like(co_all)
        named, g_zc, g_token, out = _head_run(m, x, K, idx, cr, co)
        feat = m.backbone_features(x.to(dev())).clone().cpu()                      # what the forward above read (the backbone is deterministic)
        ref = {}
        for dt in (torch.float64, torch.float32):
            ref[dt], r_ro, r_off = ho.head_grads(a["sd"], feat, K, idx, cr, co, 2, 8, GRID, "f16", dt)
        rel = float((out["readout"].detach().cpu().double() - r_ro).abs().max() / r_ro.abs().max())
        print(f"[head {persons} {which}] forward read-out vs fp64: {rel:.2e} of its largest element")
        assert rel < 1e-4                                                              # the oracle restates THIS forward
        got = dict(named, g_zc=g_zc, g_token=g_token)
        rows = [(k, ho.four_x(got[k], ref[torch.float64][k], ref[torch.float32][k])) for k in names + ["g_zc", "g_token"]]
        report(f"head {persons} {which}", rows)
        # .grad on exactly heads_parameters(), in the parameters' shapes
        params = dict(m.named_parameters())
        assert all((named[k] is not None) == (k in names) for k in named)
        assert all(named[k].shape == params[k].shape for k in names)
        # rows of the tables nobody indexes are exact zeros (the *_x tables are indexed by the row y, the *_y tables by the column x)
        for t, key in (("cross_queries_x", 1), ("cross_queries_y", 2), ("cross_values_x", 1), ("cross_values_y", 2)):
            unused = torch.ones(GRID, dtype=torch.bool)
            unused[idx[key]] = False
            assert bool((named["x_attention_head." + t][unused.to(dev())] == 0).all()), t
        assert torch.equal(named["x_attention_head.transformer.pos_embedding"][0, 0], named["x_attention_head.transformer.to_token_embedding.bias"])


def test_plumbing_values_keys_reproducibility_and_generation():
    m = _model()
    x, K, idx = _scene((2, 1), seed=720)
    xd, Kd, idxd = x.to(dev()), K.to(dev()), tuple(i.to(dev()) for i in idx)
    plain = m(xd, idx=idxd, K=Kd, is_training=True, return_readout=True)
    out = m(xd, idx=idxd, K=Kd, is_training=True, return_readout=True, train_heads=True)
    assert list(out) == list(plain) and len(plain) == 16                 # scores + the fourteen training-mode values + readout
    assert all(torch.equal(plain[k], out[k].detach()) for k in plain)
    assert out["readout"].requires_grad and out["offset"].requires_grad and not plain["readout"].requires_grad
    with pytest.raises(ValueError):
        m(xd, idx=idxd, K=Kd, is_training=True, train_heads=True)
    with pytest.raises(ValueError):
        m(xd, idx=idxd, K=Kd, return_readout=True, train_heads=True)
    # two forward + backward rounds give the same bits
    g = torch.Generator().manual_seed(721)
    cr, co = rn(g, 3, 318 + NB + 13), rn(g, 3, 2)
    n1, zc1, tk1, _ = _head_run(m, x, K, idx, cr, co)
    n1 = {k: v.clone() for k, v in n1.items() if v is not None}
    n2, zc2, tk2, _ = _head_run(m, x, K, idx, cr, co)
    assert all(torch.equal(n1[k], n2[k]) for k in n1) and torch.equal(zc1, zc2) and torch.equal(tk1, tk2)
    # a second forward before backward: the workspace has moved
    out = m(xd, idx=idxd, K=Kd, is_training=True, return_readout=True, train_heads=True)
    m(xd, idx=idxd, K=Kd, is_training=True)
    with pytest.raises(_lib.MhmrError, match="before the next forward"):
        out["readout"].sum().backward()
    # no person: the same keys as without train_heads, zero gradients
    none = tuple(torch.zeros(0, dtype=torch.long, device=dev()) for _ in range(3))
    p0 = m(xd, idx=none, K=Kd, is_training=True, return_readout=True)
    o0 = m(xd, idx=none, K=Kd, is_training=True, return_readout=True, train_heads=True)
    assert list(o0) == list(p0) and tuple(o0["readout"].shape) == (0, 318 + NB + 13)
    for p in m.parameters():
        p.grad = None
    o0["readout"].sum().backward()
    assert all(p.grad is not None and bool((p.grad == 0).all()) for p in m.heads_parameters())


def test_repack_heads_equals_repack():
    """After an in-place change of the head parameters, repack_heads() + forward gives the bits of repack() + forward."""
    m = _new_model()
    x, K, idx = _scene((2, 1), seed=730)
    args = dict(idx=tuple(i.to(dev()) for i in idx), K=K.to(dev()), is_training=True, return_readout=True)
    before = m(x.to(dev()), **args)
    g = torch.Generator().manual_seed(731)
    with torch.no_grad():
        for p in m.heads_parameters():
            p.add_(0.01 * rn(g, *p.shape).to(dev()))
    m.repack_heads()
    a = m(x.to(dev()), **args)
    m.repack()
    b = m(x.to(dev()), **args)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["readout"], before["readout"])


def test_one_training_step_lowers_the_loss():
    """Loss on decode_readout of the attached read-out, a plain SGD step theta <- theta - eps g on heads_parameters() with
    eps = 1e-3 L / |g|^2 (halved until the fp64 oracle's own decrease lies within 0.9 .. 1.1 of eps |g|^2), repack_heads(), forward:
    the loss strictly decreases, by an amount within a factor 2 of eps |g|^2.  Sign and magnitude; accuracy is the tests above."""
    import gt_oracle as go
    import heads_oracle as hdo
    import loss_oracle as lo
    from multi_hmr_amd import BodyModel, GroundTruth, Loss
    from multi_hmr_amd.heads_train import head_parameter_names
    m, a = _new_model().train_heads_(True), _assets()
    builder = GroundTruth(S, patch_size=14, smplx_neutral=BodyModel(a["data"], "smplx", num_betas=11))
    y = go.make_y("smplx", 51, S, [2, 1], depth=2.6)
    gt = builder.prepare({k: (v.to(dev()) if isinstance(v, torch.Tensor) else v) for k, v in y.items()})
    x = torch.randn(2, 3, S, S, generator=torch.Generator().manual_seed(0)).to(dev())
    args, epoch = lo.default_args(), lo.DEFAULTS["start_2d_epoch"]
    loss = Loss(args)

    def device_loss(backward):
        out = m(x, idx=gt["idx"], K=gt["K"], is_training=True, return_readout=True, train_heads=backward)
        d = m.decode_readout(out["readout"], out["offset"], gt["idx"], gt["K"])
        total, _ = loss(dict(d, scores=out["scores"]), gt, epoch=epoch, img_size=S)
        if backward:
            total.backward()
        return total.detach(), out
    names = head_parameter_names(2)
    params = dict(m.named_parameters())
    t0, out = device_loss(True)
    grads = {k: params[k].grad.detach().clone() for k in names}
    g2 = float(sum((v.double() ** 2).sum() for v in grads.values()))
    assert g2 > 0 and all(bool(torch.isfinite(v).all()) for v in grads.values())

    # the fp64 oracle of the whole chain: head (features and K as given) -> decode -> loss
    feat = m.backbone_features(x).clone().cpu()
    idx = tuple(i.cpu() for i in gt["idx"][:3])
    K, gnp = gt["K"].cpu(), {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in gt.items()}
    scores = out["scores"].detach().cpu().numpy()
    o64 = go.OracleBody(a["data"], "smplx", NB, dtype=torch.float64)
    rows = idx[1] * GRID + idx[2]

    def oracle_loss(eps):
        sd = {k: v.clone() for k, v in a["sd"].items()}
        for k in names:
            sd[k] = sd[k].double() - eps * grads[k].cpu().double()
        sd = ho.head_operands(sd, "f16", torch.float64)
        f64 = feat.double()
        z_K = ho.embedd_camera(K.double(), GRID).reshape(2, GRID * GRID, -1)
        with torch.no_grad():
            ro, off = ho.head_forward(sd, f64[idx[0], rows], torch.cat([f64[idx[0], rows], z_K[idx[0], rows]], 1), f64, K, idx, 2, 8, GRID, "f16")
        o, _ = hdo.decode(ro, off, tuple(gt["idx"][i].cpu() for i in range(len(gt["idx"]))), K, o64, nb=NB, img_size=S, nearness=True, center=15,
                          dtype=torch.float64)
        h = {k: v.detach().numpy() for k, v in o.items()}
        h["scores"] = scores
        return lo.loss_ref(h, gnp, epoch, float(S), args)["values"]["total"]
    l0 = oracle_loss(0.0)
    eps, ratio = 1e-3 * float(t0) / g2, float("nan")
    for _ in range(30):
        ratio = (l0 - oracle_loss(eps)) / (eps * g2)
        print(f"epsilon {eps:.3e}: oracle ratio {ratio:.4f}")
        if 0.9 <= ratio <= 1.1:
            break
        eps /= 2
    assert 0.9 <= ratio <= 1.1, (eps, ratio)
    print(f"recorded epsilon {eps:.3e}; loss {float(t0):.6g}; first-order decrease {eps * g2:.6e}")
    with torch.no_grad():
        for k in names:
            params[k].sub_(eps * grads[k])
    m.repack_heads()
    t1, _ = device_loss(False)
    dec = float(t0.double() - t1.double())
    print(f"device: total {float(t0):.9g} -> {float(t1):.9g}, decrease {dec:.6e}, ratio to first order {dec / (eps * g2):.4f}")
    assert dec > 0 and 0.5 <= dec / (eps * g2) <= 2.0
