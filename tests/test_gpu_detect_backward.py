"""-m gpu: the backward of the detection head (csrc/detect_bwd.hip, multi_hmr_amd/detect_train.py) against float64
torch on the operands the kernels see (tests/detect_bwd_oracle.py).  Gate: the 4x rule of DESIGN.md section 16, no floor -- for every
gradient tensor separately the kernel's maximum absolute error against fp64 is at most 4x that of the same computation in fp32 torch on
the CPU.  Every test prints kernel error, yardstick and ratio per tensor before it asserts.

Input rules of the building-block cases: hid16 with about half exact zeros (a ReLU output); rows pushed beyond the clamp on each side
(|logit| > 9.3; three and three where rows >= 16, one and one at rows == 5, none at rows == 1) among ordinary rows; no row whose fp64 p is
within a relative 1e-3 of a clamp bound (asserted: a condition on the inputs, not a tolerance); outputs NaN-filled first."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import detect_bwd_oracle as do  # noqa: E402
from multi_hmr_amd import _lib  # noqa: E402

NAMES = ("dW1", "db1", "dw2", "db2")
DT = {"f16": _lib.DT_F16, "bf16": _lib.DT_BF16}
SENTINEL_ROWS = 5


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def rn(g, *shape, std=1.0):
    return torch.empty(*shape).normal_(0, 1, generator=g) * std


def report(tag, rows):
    """rows: (tensor name, (err, yard, ratio, ok)).  Print all, then assert all."""
    for name, (err, yard, ratio, ok) in rows:
        print(f"[{tag}] {name}: kernel {err:.3e} yardstick {yard:.3e} ratio {ratio:.2f}{'' if ok else '  <-- FAILS'}")
    bad = [name for name, r in rows if not r[3]]
    assert not bad, (tag, bad)


# ------------------------------------------------------------------------------------------------------ inputs
def _beyond(rows):
    """Row indices pushed beyond the upper / the lower clamp bound."""
    if rows >= 16:
        return [1, rows // 2, rows - 1], [0, rows // 3, rows - 2]
    if rows >= 5:
        return [1], [3]
    return [], []


@functools.lru_cache(maxsize=None)
def _case(rows, C_, precision, all_beyond=False):
    """CPU operands, computed once per case and left unchanged: hid16, ctx16 (16-bit values), w2, b2, gs (fp32); column 5 of hid16 is zero
    in every row; rows 3, 10, 17, ... have gs == 0."""
    tdt = do.TDT[precision]
    g = torch.Generator().manual_seed(1000 + rows + C_ + (7 if precision == "bf16" else 0))
    w2, b2 = rn(g, C_, std=C_ ** -0.5), rn(g, 1, std=0.2)
    hid, ctx, gs = torch.relu(rn(g, rows, C_)), rn(g, rows, C_), rn(g, rows)
    hi, lo = _beyond(rows)
    if all_beyond:
        hi, lo = list(range(0, rows, 2)), list(range(1, rows, 2))
    for j, (r, sign) in enumerate([(r, 1.0) for r in hi] + [(r, -1.0) for r in lo]):
        pos = (sign * w2) > 0
        k = (12.0 + 0.3 * (j % 5)) / float((w2[pos] ** 2).sum())
        hid[r] = torch.where(pos, k * sign * w2, torch.zeros(()))
    hid[:, 5] = 0
    gs[3::7] = 0
    if all_beyond:
        gs = gs.abs() + 0.5
    hid16, ctx16 = hid.to(tdt), ctx.to(tdt)
    s, p = do.logits64(hid16, w2, b2)
    assert float(do.clamp_margin(p).min()) > 1e-3, "an input row lies within a relative 1e-3 of a clamp bound"
    if all_beyond:
        assert bool((s.abs() > 9.3).all())
    else:
        assert int((s > 9.3).sum()) == len(hi) and int((s < -9.3).sum()) == len(lo)
        assert 0.4 < float((hid16 == 0).float().mean()) < 0.6 or rows < 16
    return dict(hid16=hid16, ctx16=ctx16, w2=w2, b2=b2, gs=gs, rows=rows, C=C_, precision=precision)


@functools.lru_cache(maxsize=None)
def _ref(rows, C_, precision, clamped, all_beyond=False):
    """(fp64, fp32) oracle gradients of a case, computed once and left unchanged."""
    c = _case(rows, C_, precision, all_beyond)
    return tuple(do.grads(c["ctx16"], c["hid16"], torch.zeros(C_, C_), torch.zeros(C_), c["w2"], c["b2"], c["gs"], clamped, dt)
                 for dt in (torch.float64, torch.float32))


def _device_operands(c, ldh, ldx, sentinel):
    """hid16 / ctx16 on the device with row pitches ldh / ldx and SENTINEL_ROWS extra rows; the pitch padding and the extra rows hold
    `sentinel` (a huge finite value: reading it would show)."""
    rows, C_, tdt = c["rows"], c["C"], do.TDT[c["precision"]]
    hid = torch.full((rows + SENTINEL_ROWS, ldh), sentinel, dtype=tdt, device=dev())
    ctx = torch.full((rows + SENTINEL_ROWS, ldx), sentinel, dtype=tdt, device=dev())
    hid[:rows, :C_] = c["hid16"].to(dev())
    ctx[:rows, :C_] = c["ctx16"].to(dev())
    return hid, ctx


def _run(L, c, hid, ctx, clamped, gs=None, rows=None):
    """mhmr_detect_backward into NaN-filled outputs and a 0xFF-filled workspace -> (dW1, db1, dw2, db2)."""
    rows, C_ = c["rows"] if rows is None else rows, c["C"]
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev())
    out = nan(C_, C_), nan(C_), nan(C_), nan(1)
    nbytes = L.mhmr_detect_backward_workspace_bytes(rows, C_)
    assert nbytes >= 0
    ws = torch.full((max(nbytes, 1),), 255, dtype=torch.uint8, device=dev())
    w2, b2, gs = c["w2"].to(dev()), c["b2"].to(dev()), (c["gs"] if gs is None else gs).to(dev())
    ptr = lambda t: t.data_ptr() if rows > 0 else None
    _lib.check(L.mhmr_detect_backward(ptr(hid), hid.stride(0), ptr(ctx), ctx.stride(0), w2.data_ptr(), b2.data_ptr(), ptr(gs), rows, C_,
                                      clamped, DT[c["precision"]], *(t.data_ptr() for t in out), ws.data_ptr() if nbytes else None, nbytes,
                                      stream()), "mhmr_detect_backward")
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------------ (1) building blocks
CASES = [(rows, C_, pr) for pr in ("f16", "bf16") for C_ in (128, 384) for rows in (1, 5, 203, 515, 8300)] + [(515, 1024, "f16")]
# rows > 8 C C: the fp64 copy of dl no longer fits the region of the dW1 partials at once, so the row pass and the first stage of the
# column sums run in two chunks (131072 rows + 515)
CASES += [(8 * 128 * 128 + 515, 128, "f16")]


@pytest.mark.parametrize("rows,C_,precision", CASES)
def test_kernels_against_fp64(L, rows, C_, precision):
    """rows 1 and 5: not a multiple of the four rows of one MFMA; 515: two slices with a three-row tail; 8300: the 16-slice cap, uneven
    slices.  Both layouts (ldh = C, ldx = C + 128: the model's; ldh = C + 10, ldx = C + 72) and both clamp modes; a second call and a call
    with other sentinel values behind the rows and in the pitch padding give the same bits."""
    c = _case(rows, C_, precision)
    rows_ = []
    for ldh, ldx in ((C_, C_ + 128), (C_ + 10, C_ + 72)):
        hid, ctx = _device_operands(c, ldh, ldx, 60000.0)
        hid_b, ctx_b = _device_operands(c, ldh, ldx, -123.0)
        for clamped in (1, 0):
            got = _run(L, c, hid, ctx, clamped)
            assert all(bool(torch.isfinite(t).all()) for t in got), "every element is written"
            again, other = _run(L, c, hid, ctx, clamped), _run(L, c, hid_b, ctx_b, clamped)
            assert all(torch.equal(a, b) for a, b in zip(got, again)), "two calls differ"
            assert all(torch.equal(a, b) for a, b in zip(got, other)), "values behind the rows or in the pitch padding were read"
            assert bool((got[0][5] == 0).all()) and float(got[1][5]) == 0.0 and float(got[2][5]) == 0.0, "a column of zeros in hid16"
            r64, r32 = _ref(rows, C_, precision, bool(clamped))
            rows_ += [(f"{n} ldh {ldh} ldx {ldx} clamped {clamped}", do.four_x(t.reshape(a.shape), a, b)) for n, t, a, b in zip(NAMES, got, r64, r32)]
    worst = max(rows_, key=lambda r: r[1][2] if r[1][2] != float("inf") else -1.0)
    print(f"[detect bwd rows {rows} C {C_} {precision}] worst ratio {worst[1][2]:.2f} at {worst[0]}")
    report(f"detect bwd rows {rows} C {C_} {precision}", rows_)


def test_clamp_and_zero_cotangent_rows_are_exact(L):
    rows, C_ = 203, 128
    # every row beyond the clamp: four outputs of exact zeros; the same inputs unclamped: nonzero, and under the 4x rule
    c = _case(rows, C_, "f16", True)
    hid, ctx = _device_operands(c, C_, C_ + 64, 60000.0)
    got = _run(L, c, hid, ctx, 1)
    assert all(bool((t == 0).all()) for t in got)
    got = _run(L, c, hid, ctx, 0)
    assert all(bool((t != 0).any()) for t in got)
    r64, r32 = _ref(rows, C_, "f16", False, True)
    report("all rows beyond the clamp, unclamped", [(n, do.four_x(t.reshape(a.shape), a, b)) for n, t, a, b in zip(NAMES, got, r64, r32)])
    # rows with gs == 0 contribute exact zeros: other (finite) contents in those rows change no bit; gs == 0 everywhere gives zeros
    c = _case(rows, C_, "f16")
    hid, ctx = _device_operands(c, C_, C_ + 64, 60000.0)
    got = _run(L, c, hid, ctx, 1)
    zero = c["gs"] == 0
    assert int(zero.sum()) == 29
    g = torch.Generator().manual_seed(5)
    hid2, ctx2 = hid.clone(), ctx.clone()
    hid2[:rows, :C_][zero.to(dev())] = torch.relu(rn(g, 29, C_) * 3).to(hid.dtype).to(dev())
    ctx2[:rows, :C_][zero.to(dev())] = (rn(g, 29, C_) * 100).to(ctx.dtype).to(dev())
    other = _run(L, c, hid2, ctx2, 1)
    assert all(torch.equal(a, b) for a, b in zip(got, other))
    none = _run(L, c, hid, ctx, 1, gs=torch.zeros(rows))
    assert all(bool((t == 0).all()) for t in none)
    # rows == 0: zeros, nothing is read
    empty = _run(L, c, hid, ctx, 1, rows=0)
    assert all(bool((t == 0).all()) for t in empty)


@pytest.mark.parametrize("ldx", [128, 128 + 72])
@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("rows", [5, 515, 8300])
def test_dw1_is_the_context_gemm_on_the_materialised_left_operand(L, rows, precision, ldx):
    """The dW1 product and mhmr_grad_ctx_gemm are ONE sliced outer product (csrc/row_sums.h): on the left operand written out as fp32,
    G[m][n] = hid16[m][n] > 0 ? dl_m : 0, the context GEMM gives the bits of dW1 (up to the exact factor w2[n] = +-1).  The inputs let the
    host know dl exactly: b2 = 0, w2 = (+1, -1, +1, ...) and hid16[m][2j] = hid16[m][2j + 1] = h, a small integer, so score_dot is exactly 0
    in any order, p = 0.5 lies inside the clamp and dl_m = 0.25 gs_m exactly, in fp64 and after the fp32 rounding.  rows 5: a partial MFMA
    step; 515: two slices with a three-row tail; 8300: the 16-slice cap with uneven slices."""
    C_ = 128
    g = torch.Generator().manual_seed(4000 + rows + (7 if precision == "bf16" else 0))
    h = torch.randint(1, 4, (rows, C_ // 2), generator=g) * (torch.rand(rows, C_ // 2, generator=g) < 0.5)
    hid = h.repeat_interleave(2, dim=1).float()
    assert 0.4 < float((hid == 0).float().mean()) < 0.6 or rows < 16
    w2 = torch.ones(C_)
    w2[1::2] = -1
    gs = rn(g, rows)
    gs[3::7] = 0
    tdt = do.TDT[precision]
    c = dict(hid16=hid.to(tdt), ctx16=rn(g, rows, C_).to(tdt), w2=w2, b2=torch.zeros(1), gs=gs, rows=rows, C=C_, precision=precision)
    hid_d, ctx_d = _device_operands(c, C_, ldx, 60000.0)
    G = torch.where(hid > 0, (0.25 * gs)[:, None].expand(rows, C_), torch.zeros(())).contiguous().to(dev())
    nbytes = L.mhmr_grad_ctx_gemm_workspace_bytes(rows, C_, C_)
    assert nbytes > 0
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=dev())
    dW = torch.full((C_, C_), float("nan"), dtype=torch.float32, device=dev())
    _lib.check(L.mhmr_grad_ctx_gemm(G.data_ptr(), C_, ctx_d.data_ptr(), ldx, dW.data_ptr(), rows, C_, C_, C_, DT[precision], ws.data_ptr(),
                                    nbytes, stream()), "mhmr_grad_ctx_gemm")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dW).all()) and bool((dW != 0).any())
    want = w2.to(dev())[:, None] * dW
    for clamped in (1, 0):
        g_w1 = _run(L, c, hid_d, ctx_d, clamped)[0]
        differ = (g_w1 != want).nonzero()
        print(f"[dW1 == ctx gemm rows {rows} {precision} ldx {ldx} clamped {clamped}] elements that differ: {len(differ)}"
              + (f", first at {differ[0].tolist()}" if len(differ) else ""))
        assert torch.equal(g_w1, want)


# ------------------------------------------------------------------------------------------------------ (2) through Model
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
    return _new_model().train_detection_(True)


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
    return x.to(dev()), K.to(dev()), tuple(torch.tensor(v, dtype=torch.long, device=dev()) for v in (bs, ys, xs))


def _named_grads(m):
    return {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


def _clear(m):
    for p in m.parameters():
        p.grad = None


@pytest.mark.parametrize("persons", [(2, 1), (0, 0)])
def test_through_model_against_fp64(persons):
    """forward(train_detection=True) + backward of sum(cotangent * scores): the 4x rule on the four parameters.  The oracle takes the
    device's ctx16[:, :C] and hid_cls as given.  Without a person the gradients are not zeros: every cell is a negative."""
    m = _model()
    x, K, idx = _scene(persons, seed=800 + sum(persons))
    B, C_ = len(persons), m.embed_dim
    _clear(m)
    out = m(x, idx=idx, K=K, is_training=True, train_detection=True)
    assert out["scores"].requires_grad and tuple(out["scores"].shape) == (B, GRID, GRID, 1)
    assert (len(out) == 1) == (sum(persons) == 0)
    cot = rn(torch.Generator().manual_seed(801), B, GRID, GRID, 1)
    (out["scores"] * cot.to(dev())).sum().backward()
    P = m._packed
    ws = m._workspace(P, B)
    rows = B * GRID * GRID
    X, hidden = ws["ctx16"][:rows, :C_].cpu(), ws["hid_cls"][:rows].cpu()
    w2, b2 = P["cls2_w"].cpu(), P["cls2_b"].cpu()
    s, p = do.logits64(hidden, w2, b2)
    fwd_err = float((torch.clamp(p, do.CLAMP_LO, do.CLAMP_HI) - out["scores"].detach().cpu().double().reshape(-1)).abs().max())
    print(f"[model persons {persons}] forward scores vs fp64 on the device's hidden layer: {fwd_err:.2e}")
    assert fwd_err < 1e-5                                                              # the oracle restates THIS forward
    assert float(do.clamp_margin(p).min()) > 1e-3
    r64, r32 = (do.grads(X, hidden, P["cls0_w"].cpu(), P["cls0_b"].cpu(), w2, b2, cot.reshape(-1), True, dt) for dt in (torch.float64, torch.float32))
    got = [q.grad for q in m.detection_parameters()]
    assert all(t is not None and t.shape == q.shape for t, q in zip(got, m.detection_parameters()))
    assert all(bool((t != 0).any()) for t in got)
    report(f"model persons {persons}", [(n, do.four_x(t.reshape(a.shape), a, b)) for n, t, a, b in zip(NAMES, got, r64, r32)])


def test_plumbing_values_keys_and_generation():
    from multi_hmr_amd.detect_train import DETECTION_PARAMETERS
    m = _model()
    x, K, idx = _scene((2, 1), seed=820)
    plain = m(x, idx=idx, K=K, is_training=True)
    out = m(x, idx=idx, K=K, is_training=True, train_detection=True)
    assert list(out) == list(plain) and len(plain) == 15                  # scores + the fourteen training-mode values
    assert all(torch.equal(plain[k], out[k].detach()) for k in plain)
    assert out["scores"].requires_grad and not plain["scores"].requires_grad and not out["offset"].requires_grad
    with pytest.raises(ValueError):
        m(x, K=K, train_detection=True)
    # .grad lands on exactly detection_parameters(); two rounds give the same bits
    cot = rn(torch.Generator().manual_seed(821), 2, GRID, GRID, 1).to(dev())
    rounds = []
    for _ in range(2):
        _clear(m)
        (m(x, idx=idx, K=K, is_training=True, train_detection=True)["scores"] * cot).sum().backward()
        rounds.append(_named_grads(m))
    assert {k for k, v in rounds[0].items() if v is not None} == set(DETECTION_PARAMETERS)
    assert all(torch.equal(rounds[0][k], rounds[1][k]) for k in DETECTION_PARAMETERS)
    # a forward in between: the workspace has moved
    out = m(x, idx=idx, K=K, is_training=True, train_detection=True)
    m(x, idx=idx, K=K, is_training=True)
    with pytest.raises(_lib.MhmrError, match="before the next forward"):
        out["scores"].sum().backward()
    # repack_heads() in between: the packed second-layer row has moved
    out = m(x, idx=idx, K=K, is_training=True, train_detection=True)
    m.repack_heads()
    with pytest.raises(_lib.MhmrError, match="before the next forward"):
        out["scores"].sum().backward()


def test_composes_with_train_heads():
    """Two independent autograd nodes over one workspace: .grad lands on exactly the union, and the head gradients are bit-equal to a run
    without train_detection."""
    from multi_hmr_amd.detect_train import DETECTION_PARAMETERS
    from multi_hmr_amd.heads_train import head_parameter_names
    m = _new_model().train_heads_(True).train_detection_(True)
    x, K, idx = _scene((2, 1), seed=830)
    g = torch.Generator().manual_seed(831)
    cr, co, cs = rn(g, 3, 318 + NB + 13).to(dev()), rn(g, 3, 2).to(dev()), rn(g, 2, GRID, GRID, 1).to(dev())
    heads = head_parameter_names(2)

    def run(detection):
        _clear(m)
        out = m(x, idx=idx, K=K, is_training=True, return_readout=True, train_heads=True, train_detection=detection)
        total = (out["readout"] * cr).sum() + (out["offset"] * co).sum()
        if detection:
            total = total + (out["scores"] * cs).sum()
        total.backward()
        return _named_grads(m), out
    without, o0 = run(False)
    both, o1 = run(True)
    assert list(o0) == list(o1) and all(torch.equal(o0[k].detach(), o1[k].detach()) for k in o0)
    assert {k for k, v in without.items() if v is not None} == set(heads)
    assert {k for k, v in both.items() if v is not None} == set(heads) | set(DETECTION_PARAMETERS)
    assert all(torch.equal(without[k], both[k]) for k in heads)
    # the detection gradients are those of a run without train_heads
    _clear(m)
    (m(x, idx=idx, K=K, is_training=True, train_detection=True)["scores"] * cs).sum().backward()
    alone = _named_grads(m)
    assert all(torch.equal(alone[k], both[k]) for k in DETECTION_PARAMETERS)


def test_repack_heads_equals_repack_after_a_change_of_mlp_classif():
    m = _new_model()
    x, K, idx = _scene((2, 1), seed=840)
    args = dict(idx=idx, K=K, is_training=True, return_readout=True)
    before = m(x, **args)
    g = torch.Generator().manual_seed(841)
    with torch.no_grad():
        for p in m.detection_parameters():
            p.add_(0.01 * rn(g, *p.shape).to(dev()))
    m.repack_heads()
    a = m(x, **args)
    m.repack()
    b = m(x, **args)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["scores"], before["scores"]) and torch.equal(a["readout"], before["readout"])


def test_one_training_step_on_the_detection_head_lowers_the_loss():
    """Loss total with the predicted persons held fixed (only scores carries a graph), a plain SGD step theta <- theta - eps g on
    detection_parameters() with eps = 1e-3 L / |g|^2 (halved until the fp64 oracle's own decrease lies within 0.9 .. 1.1 of eps |g|^2),
    repack_heads(), forward: the loss strictly decreases, by an amount within a factor 2 of eps |g|^2.  The oracle restates the two
    layers as the device runs them (16-bit first-layer weight and hidden layer) on the device's ctx16."""
    import gt_oracle as go
    import loss_oracle as lo
    from multi_hmr_amd import BodyModel, GroundTruth, Loss
    from multi_hmr_amd.detect_train import DETECTION_PARAMETERS as names
    m, a = _new_model().train_detection_(True), _assets()
    builder = GroundTruth(S, patch_size=14, smplx_neutral=BodyModel(a["data"], "smplx", num_betas=11))
    y = go.make_y("smplx", 51, S, [2, 1], depth=2.6)
    gt = builder.prepare({k: (v.to(dev()) if isinstance(v, torch.Tensor) else v) for k, v in y.items()})
    x = torch.randn(2, 3, S, S, generator=torch.Generator().manual_seed(0)).to(dev())
    args, epoch = lo.default_args(), lo.DEFAULTS["start_2d_epoch"]
    loss = Loss(args)

    def device_loss(backward):
        out = m(x, idx=gt["idx"], K=gt["K"], is_training=True, train_detection=backward)
        total, _ = loss(out, gt, epoch=epoch, img_size=S)
        if backward:
            total.backward()
        return total.detach(), out
    params = dict(m.named_parameters())
    t0, out = device_loss(True)
    grads = {k: params[k].grad.detach().clone() for k in names}
    assert all(p.grad is None for k, p in params.items() if k not in names)
    g2 = float(sum((v.double() ** 2).sum() for v in grads.values()))
    assert g2 > 0 and all(bool(torch.isfinite(v).all()) for v in grads.values())

    P = m._packed
    rows, C_ = 2 * GRID * GRID, m.embed_dim
    X = m._workspace(P, 2)["ctx16"][:rows, :C_].cpu().double()
    gnp = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in gt.items()}
    fixed = {k: v.detach().cpu().numpy() for k, v in out.items() if k != "scores"}
    r16 = lambda t: t.to(torch.float16).double()

    def oracle_loss(eps):
        W1, b1, w2, b2 = (a["sd"][k].double() - eps * grads[k].cpu().double() for k in names)
        hid = r16(torch.relu(X @ r16(W1.float()).T + b1.float().double()))
        p = torch.clamp(torch.sigmoid(hid @ w2.float().double().reshape(-1) + b2.float().double()), 1e-4, 1 - 1e-4)
        return lo.loss_ref(dict(fixed, scores=p.reshape(2, GRID, GRID, 1).numpy()), gnp, epoch, float(S), args)["values"]["total"]
    l0 = oracle_loss(0.0)
    print(f"device total {float(t0):.9g}, oracle total {l0:.9g}")
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
