"""-m gpu: heads from stored features (``Model.forward_features``, csrc/feature_grad.hip) -- the values against
``Model.forward`` bit for bit, the product ``mhmr_rows_times_weight`` and the detector's term against float64, and ``features.grad``
through the whole path against fp64 autograd of tests/feature_grad_oracle.py.  Accuracy gate: the 4x rule of DESIGN.md section 16 (the
kernel's maximum absolute error against fp64 is at most 4x that of the same computation in fp32 torch on the CPU; a yardstick of exactly
zero demands the exact bits).  Every test prints kernel error, yardstick and ratio per tensor before it asserts."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import detect_bwd_oracle as do  # noqa: E402
import feature_grad_oracle as fo  # noqa: E402
import hph_bwd_oracle as ho  # noqa: E402
from multi_hmr_amd import _lib  # noqa: E402

S, GRID, NB, NAME = 224, 16, 10, "dinov2_vits14"
NDEC = 318 + NB + 13
ROWS = (1, 5, 203, 515)           # one row; less than one MFMA's 16; four row tiles with a tail of 11; nine with a tail of 3
BIG = 6.0e4                       # sentinel of the 16-bit pitch padding: finite in f16, reading it would show


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


# ------------------------------------------------------------------------------------------------------ (2) the product alone
def _pitched(t, ld, fill, extra_rows=3):
    """t [rows, cols] on the device inside a [rows + extra_rows, ld] buffer filled with `fill`; -> (buffer, view of the data)."""
    buf = torch.full((t.shape[0] + extra_rows, ld), fill, dtype=t.dtype, device=dev())
    buf[:t.shape[0], :t.shape[1]] = t.to(dev())
    return buf, buf[:t.shape[0], :t.shape[1]]


def _rtw(L, left_buf, w_buf, out_buf, rows, n, C_, acc, precision):
    dt = _lib.DT_F16 if precision == "f16" else _lib.DT_BF16
    _lib.check(L.mhmr_rows_times_weight(left_buf.data_ptr(), left_buf.stride(0), w_buf.data_ptr(), w_buf.stride(0), out_buf.data_ptr(),
                                        out_buf.stride(0), rows, n, C_, int(acc), dt, stream()), "mhmr_rows_times_weight")


@functools.lru_cache(maxsize=None)
def _product_case(n, C_, precision):
    """CPU operands for the largest row count (smaller runs take its first rows) and the fp64 / fp32 references, computed once."""
    g = torch.Generator().manual_seed(3000 + n + C_ + (7 if precision == "bf16" else 0))
    left, w16 = rn(g, max(ROWS), n), rn(g, n, C_, std=n ** -0.5).to(ho.TDT[precision])
    return left, w16, fo.product(left, w16, torch.float64), fo.product(left, w16, torch.float32)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("C_", [128, 384, 1024])
@pytest.mark.parametrize("n", [64, 512])
def test_product_against_fp64(L, n, C_, precision):
    """mhmr_rows_times_weight with pitches wider than the rows, into sentinel-filled buffers: the 4x rule; nothing outside the rows x C
    block changes; other sentinel values change no bit; two calls give the same bits; the rows are independent (the first rows of a longer
    run are the shorter run); the accumulate form is a write followed by an fp32 add."""
    left, w16, r64, r32 = _product_case(n, C_, precision)
    results, table = {}, []
    for rows in ROWS:
        runs = []
        for s_in, s_out in ((BIG, float("nan")), (-3.0e4, 777.0)):
            lb, _ = _pitched(left[:rows], n + 8, s_in)
            wb, _ = _pitched(w16, C_ + 16, s_in)
            ob = torch.full((rows + 3, C_ + 4), s_out, dtype=torch.float32, device=dev())
            _rtw(L, lb, wb, ob, rows, n, C_, False, precision)
            pad = torch.ones_like(ob, dtype=torch.bool)
            pad[:rows, :C_] = False
            assert bool((ob[pad] == s_out).all() if s_out == s_out else torch.isnan(ob[pad]).all()), "a write outside the rows x C block"
            runs.append(ob[:rows, :C_].clone())
            _rtw(L, lb, wb, ob, rows, n, C_, False, precision)
            assert torch.equal(runs[-1], ob[:rows, :C_]), "two calls differ"
        assert torch.equal(runs[0], runs[1]), "the sentinels reached the result"
        # the pitches above allow vector loads and stores; odd ones take the element-by-element form of the kernel: the same bits
        lb, _ = _pitched(left[:rows], n + 1, BIG)
        wb, _ = _pitched(w16, C_ + 2, BIG)
        ob = torch.full((rows + 3, C_ + 1), float("nan"), dtype=torch.float32, device=dev())
        _rtw(L, lb, wb, ob, rows, n, C_, False, precision)
        assert torch.equal(ob[:rows, :C_], runs[0]) and bool(torch.isnan(ob[:, C_:]).all()) and bool(torch.isnan(ob[rows:]).all()), "odd pitches"
        ob[:rows, :C_] = base = rn(torch.Generator().manual_seed(rows + 1), rows, C_).to(dev())
        _rtw(L, lb, wb, ob, rows, n, C_, True, precision)
        assert torch.equal(ob[:rows, :C_], base + runs[0]) and bool(torch.isnan(ob[:, C_:]).all()), "odd pitches, accumulate"
        results[rows] = runs[0]
        table.append((f"rows {rows}", ho.four_x(runs[0], r64[:rows], r32[:rows])))
        # accumulate: out = out + product
        base = rn(torch.Generator().manual_seed(rows), rows, C_).to(dev())
        lb, _ = _pitched(left[:rows], n, 0.0, 0)
        wb, _ = _pitched(w16, C_, 0.0, 0)
        ob = base.clone()
        _rtw(L, lb, wb, ob, rows, n, C_, True, precision)
        assert torch.equal(ob, base + runs[0]), "accumulate is not write + add"
    for short, long in ((1, 5), (5, 203), (203, 515)):
        assert torch.equal(results[long][:short], results[short]), (short, long)
    report(f"product n {n} C {C_} {precision}", table)


# ------------------------------------------------------------------------------------------------------ (3) the detector's term
@functools.lru_cache(maxsize=None)
def _detect_case(rows, C_, precision):
    """test_gpu_detect_backward._case (half the hidden entries exact zeros, rows beyond both clamp bounds, rows with a zero cotangent)
    plus a first-layer weight in the 16-bit type; computed once and left unchanged."""
    import test_gpu_detect_backward as tdb
    c = dict(tdb._case(rows, C_, precision))
    g = torch.Generator().manual_seed(4000 + rows + C_)
    c["w16"] = rn(g, C_, C_, std=C_ ** -0.5).to(ho.TDT[precision])
    c["beyond"] = sorted(sum(tdb._beyond(rows), []))
    return c


@functools.lru_cache(maxsize=None)
def _detect_ref(rows, C_, precision, clamped):
    c = _detect_case(rows, C_, precision)
    return tuple(fo.detector_term(c["hid16"], c["w16"], c["w2"], c["b2"], c["gs"], clamped, dt) for dt in (torch.float64, torch.float32))


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("C_", [128, 384])
@pytest.mark.parametrize("rows", ROWS)
def test_detector_term_against_fp64(L, rows, C_, precision):
    """mhmr_detect_feature_grad, clamped and unclamped: the 4x rule; rows beyond the clamp (clamped) and rows with a zero cotangent are
    exact zeros; and it IS the plain product on the hidden layer's cotangent written out in fp32 (dl read back from the workspace)."""
    from multi_hmr_amd.detect_train import detect_feature_grad
    c = _detect_case(rows, C_, precision)
    dt = _lib.DT_F16 if precision == "f16" else _lib.DT_BF16
    hb, hid = _pitched(c["hid16"], C_ + 10, BIG)
    wb, w16 = _pitched(c["w16"], C_ + 6, BIG)
    w2, b2, gs = c["w2"].to(dev()), c["b2"].to(dev()), c["gs"].to(dev())
    table = []
    for clamped in (True, False):
        ob = torch.full((rows + 3, C_ + 4), float("nan"), dtype=torch.float32, device=dev())
        got, dl = detect_feature_grad(hid, w16, w2, b2, gs, rows, C_, clamped, dt, stream(), g_feat=ob[:rows, :C_])
        pad = torch.ones_like(ob, dtype=torch.bool)
        pad[:rows, :C_] = False
        assert bool(torch.isnan(ob[pad]).all()) and not bool(torch.isnan(got).any())
        r64, r32 = _detect_ref(rows, C_, precision, clamped)
        table.append((f"clamped {clamped}", ho.four_x(got, r64, r32)))
        zero_rows = sorted(set(range(3, rows, 7)) | (set(c["beyond"]) if clamped else set()))
        assert bool((got[zero_rows] == 0).all()), "a clamped or zero-cotangent row is not exact zeros"
        assert bool((r64[zero_rows] == 0).all())
        live = sorted(set(range(rows)) - set(zero_rows))
        assert not live or bool((got[live] != 0).any())
        if not clamped and c["beyond"]:
            assert bool((got[[r for r in c["beyond"] if r not in range(3, rows, 7)]] != 0).any())
        # the same bits from the plain product on the materialised left operand
        hc = torch.where(hid.float() > 0, dl[:, None] * w2[None, :], torch.zeros((), device=dev())).contiguous()
        plain = torch.full((rows, C_), float("nan"), dtype=torch.float32, device=dev())
        _lib.check(L.mhmr_rows_times_weight(hc.data_ptr(), C_, w16.data_ptr(), w16.stride(0), plain.data_ptr(), C_, rows, C_, C_, 0, dt, stream()),
                   "mhmr_rows_times_weight")
        assert torch.equal(plain, got), "the fused left operand differs from the stored one"
        again, _ = detect_feature_grad(hid, w16, w2, b2, gs, rows, C_, clamped, dt, stream())
        assert torch.equal(again, got)
        # contiguous operands (the model's layout: vector loads and stores) give the bits of the pitched ones (element by element)
        packed, _ = detect_feature_grad(hid.contiguous(), w16.contiguous(), w2, b2, gs, rows, C_, clamped, dt, stream())
        assert torch.equal(packed, got)
    report(f"detector rows {rows} C {C_} {precision}", table)


# ------------------------------------------------------------------------------------------------------ the model
@functools.lru_cache(maxsize=None)
def _assets():
    import synthetic
    data, mean = synthetic.make_smplx_data(seed=0), synthetic.make_mean_params(seed=0)
    sd = synthetic.make_state_dict(NAME, S, seed=42, depth_override=4, mean_params=mean)
    return dict(data=data, mean=mean, sd=sd)


def _new_model(precision="f16"):
    """The fixture of tests/test_gpu_hph_backward.py: ViT-S, 224^2, backbone depth 4, synthetic weights; every parameter frozen."""
    from multi_hmr_amd import Model
    a = _assets()
    m = Model(backbone=NAME, img_size=S, smplx_data=a["data"], mean_params=a["mean"], backbone_depth=4, precision=precision)
    m.load_state_dict(a["sd"], strict=True)
    return m.to(dev()).eval()


@functools.lru_cache(maxsize=None)
def _model(precision="f16"):
    return _new_model(precision)


def _scene(persons, seed):
    """Images, intrinsics and distinct cells for `persons` per image, sorted by (image, y, x) as torch.where leaves them (on the device)."""
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


def _clear(m):
    for p in m.parameters():
        p.grad = None


def _same(a, b):
    assert list(a) == list(b), (list(a), list(b))
    for k in a:
        assert torch.equal(a[k].detach(), b[k].detach()), k


# ------------------------------------------------------------------------------------------------------ (1) values
@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_values_equal_forward_bit_for_bit(precision):
    """Features stored, another batch of the same size run in between (nothing stale can help), then forward_features(f) == forward(x) in
    every key: training mode with the read-out, inference as a person list and batched; the workspace view itself as the input; and a
    half-size store, f.half(), equals its widened copy."""
    m = _model(precision)
    assert m.packed_precision in (None, precision)
    x, K, idx = _scene((2, 1), seed=900)
    x2, K2, idx2 = _scene((1, 2), seed=901)
    train = dict(idx=idx, K=K, is_training=True, return_readout=True)
    want = m(x, **train)
    assert m.packed_precision == precision and len(want) == 16
    # a threshold that lets a few cells through, from the scores themselves (the weights are synthetic)
    thr = float(want["scores"].flatten().sort().values[-6]) - 1e-6
    persons_x = m(x, K=K, det_thresh=thr)
    batched_x, ids_x = m(x, K=K, det_thresh=thr, return_batched=True)
    assert 1 <= len(persons_x) <= 6
    f = m.backbone_features(x).clone()
    assert tuple(f.shape) == (2, GRID * GRID, 384) and f.dtype == torch.float32

    def other():
        m(x2, idx=idx2, K=K2, is_training=True, return_readout=True)
        assert not torch.equal(m.backbone_features(x2), f)
    other()
    f_before = f.clone()
    _same(want, m.forward_features(f, **train))
    other()
    _same(want, m.forward_features(f.reshape(-1, 384), **train))                       # [B N, C]
    other()
    persons_f, ids_f = m.forward_features(f, K=K, det_thresh=thr, return_image_index=True)
    assert len(persons_f) == len(persons_x) and torch.equal(ids_f, ids_x)
    for a, b in zip(persons_x, persons_f):
        _same(a, b)
    assert list(persons_f[0]) == list(m.PERSON_KEYS)
    other()
    batched_f, ids_b = m.forward_features(f, K=K, det_thresh=thr, return_batched=True)
    _same(batched_x, batched_f)
    assert torch.equal(ids_b, ids_x)
    assert torch.equal(f, f_before), "features were written to"
    # the workspace view, passed in directly (forward has since overwritten the context rows of the detected cells)
    view = m.backbone_features(x)
    m(x, **train)
    _same(want, m.forward_features(view, **train))
    assert view.data_ptr() == m.backbone_features(x).data_ptr()
    # a half-size store: the 16-bit tensor and its widened copy give the same result (and one that differs from the fp32 features')
    tdt = ho.TDT[precision]
    other()
    a = m.forward_features(f.to(tdt).float(), **train)
    other()
    b = m.forward_features(f.to(tdt), **train)
    _same(a, b)
    other()
    _same(a, m.forward_features(f.half().float() if precision == "f16" else f.to(tdt).double(), **train))
    assert not torch.equal(a["readout"], want["readout"])


# ------------------------------------------------------------------------------------------------------ (4) the whole path
def _feature_run(m, f, K, idx, cr, co, cs, **kw):
    """forward_features + backward of sum(cr readout) + sum(co offset) + sum(cs scores) (None: left out) -> (f.grad, out)."""
    _clear(m)
    f = f.detach().clone().requires_grad_()
    out = m.forward_features(f, idx=idx, K=K, is_training=True, return_readout=True, **kw)
    total = 0
    if cr is not None and out["readout"].numel():
        total = total + (out["readout"] * cr).sum() + (out["offset"] * co).sum()
    if cs is not None:
        total = total + (out["scores"] * cs).sum()
    total.backward()
    return f.grad, out


def _oracle(m, f, K, idx, cr, co, cs, B, precision="f16"):
    """fp64 and fp32 oracle parts for the device's features, K and stored hidden layer."""
    a = _assets()
    hid16 = m._workspace(m._packed, B)["hid_cls"][:B * GRID * GRID].cpu()
    cpu = lambda t: None if t is None else t.cpu()
    return {dt: fo.feature_grads(a["sd"], f.cpu(), K.cpu(), tuple(i.cpu() for i in idx), cpu(cr), cpu(co), cpu(cs), hid16, 2, 8, GRID, precision, dt)
            for dt in (torch.float64, torch.float32)}


@pytest.mark.parametrize("persons", [(2, 1), (9, 0, 1)])
def test_feature_gradient_against_fp64(persons):
    """features.grad through forward_features against fp64 autograd: the 4x rule on the whole [B, N, C] tensor, on the persons' rows and
    on the rows of the image without persons (which receive the detector's term alone: checked on the oracle's parts); with the scores
    left out the heads' term alone, with only the scores the detector's term alone."""
    m = _model()
    x, K, idx = _scene(persons, seed=910 + len(persons))
    B, Pn = len(persons), sum(persons)
    g = torch.Generator().manual_seed(911)
    cr, co, cs = rn(g, Pn, NDEC).to(dev()), rn(g, Pn, 2).to(dev()), rn(g, B, GRID, GRID, 1).to(dev())
    f = m.backbone_features(x).clone()
    prow = (idx[0].cpu(), (idx[1] * GRID + idx[2]).cpu())
    empty = [b for b, n in enumerate(persons) if n == 0]
    table = []
    for which, (r_, o_, s_) in (("all", (cr, co, cs)), ("heads", (cr, co, None)), ("detector", (None, None, cs))):
        got, out = _feature_run(m, f, K, idx, r_, o_, s_)
        assert got is not None and got.shape == f.shape and bool(torch.isfinite(got).all())
        ref = _oracle(m, f, K, idx, r_, o_, s_, B)
        key = {"all": "total", "heads": "heads", "detector": "detector"}[which]
        r64, r32 = ref[torch.float64][key], ref[torch.float32][key]
        if which != "detector":
            ro = ho.head_forward(ho.head_operands(_assets()["sd"], "f16", torch.float64), f.cpu().double()[prow], torch.cat(
                [f.cpu().double()[prow], ho.embedd_camera(K.cpu().double(), GRID).reshape(B, GRID * GRID, -1)[prow]], 1), f.cpu().double(), K.cpu(),
                tuple(i.cpu() for i in idx), 2, 8, GRID, "f16")[0]
            rel = float((out["readout"].detach().cpu().double() - ro).abs().max() / ro.abs().max())
            print(f"[features {persons} {which}] forward read-out vs fp64: {rel:.2e} of its largest element")
            assert rel < 1e-4                                                          # the oracle restates THIS forward
        gc = got.cpu()
        table.append((f"{which}: whole tensor", ho.four_x(gc, r64, r32)))
        table.append((f"{which}: persons' rows", ho.four_x(gc[prow], r64[prow], r32[prow])))
        for b in empty:
            table.append((f"{which}: image {b} (no person)", ho.four_x(gc[b], r64[b], r32[b])))
            assert bool((ref[torch.float64]["heads"][b] == 0).all())                   # only the detector reaches these rows
            if which == "heads":
                assert bool((gc[b] == 0).all())
            else:
                assert torch.equal(ref[torch.float64]["total"][b], ref[torch.float64]["detector"][b]) and bool((gc[b] != 0).any())
        assert all(p.grad is None for p in m.parameters())
    report(f"features {persons}", table)


def test_feature_gradient_against_fp64_bf16():
    """The bf16 operand type through the same path (context, to_kv16 and the detector's weight and hidden layer in bf16): all cotangents."""
    m = _model("bf16")
    x, K, idx = _scene((2, 1), seed=915)
    g = torch.Generator().manual_seed(916)
    cr, co, cs = rn(g, 3, NDEC).to(dev()), rn(g, 3, 2).to(dev()), rn(g, 2, GRID, GRID, 1).to(dev())
    f = m.backbone_features(x).clone()
    got, _ = _feature_run(m, f, K, idx, cr, co, cs)
    assert m.packed_precision == "bf16"
    ref = _oracle(m, f, K, idx, cr, co, cs, 2, "bf16")
    prow = (idx[0].cpu(), (idx[1] * GRID + idx[2]).cpu())
    gc, r64, r32 = got.cpu(), ref[torch.float64]["total"], ref[torch.float32]["total"]
    other = torch.ones(2, GRID * GRID, dtype=torch.bool)
    other[prow] = False
    report("features (2, 1) bf16", [("whole tensor", ho.four_x(gc, r64, r32)), ("persons' rows", ho.four_x(gc[prow], r64[prow], r32[prow])),
                                    ("the other rows", ho.four_x(gc[other], r64[other], r32[other]))])


# ------------------------------------------------------------------------------------------------------ (5) composition
def test_composition_with_the_parameter_gradients():
    from multi_hmr_amd.detect_train import DETECTION_PARAMETERS
    from multi_hmr_amd.heads_train import head_parameter_names
    m = _new_model().train_heads_(True).train_detection_(True)
    x, K, idx = _scene((2, 1), seed=920)
    g = torch.Generator().manual_seed(921)
    cr, co, cs = rn(g, 3, NDEC).to(dev()), rn(g, 3, 2).to(dev()), rn(g, 2, GRID, GRID, 1).to(dev())
    names = head_parameter_names(2) + list(DETECTION_PARAMETERS)
    grads = lambda: {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}
    # from images
    _clear(m)
    out = m(x, idx=idx, K=K, is_training=True, return_readout=True, train_heads=True, train_detection=True)
    ((out["readout"] * cr).sum() + (out["offset"] * co).sum() + (out["scores"] * cs).sum()).backward()
    from_images = grads()
    zc, tk = m.heads_feature_grads["g_zc"].clone(), m.heads_feature_grads["g_token"].clone()
    f = m.backbone_features(x).clone()
    # from the stored features, the features a leaf as well
    m.heads_feature_grads = None
    g1, out_f = _feature_run(m, f, K, idx, cr, co, cs, train_heads=True, train_detection=True)
    from_features = grads()
    _same(out, out_f)
    assert {k for k, v in from_features.items() if v is not None} == set(names)
    assert all(torch.equal(from_images[k], from_features[k]) for k in names)
    assert torch.equal(m.heads_feature_grads["g_zc"], zc) and torch.equal(m.heads_feature_grads["g_token"], tk)
    # and without requires_grad on the features: the same parameter gradients, nothing else
    _clear(m)
    o2 = m.forward_features(f, idx=idx, K=K, is_training=True, return_readout=True, train_heads=True, train_detection=True)
    ((o2["readout"] * cr).sum() + (o2["offset"] * co).sum() + (o2["scores"] * cs).sum()).backward()
    assert all(torch.equal(from_images[k], grads()[k]) for k in names) and f.grad is None
    # all parameters frozen, only f requires grad: the same f.grad, no parameter gradient; a second run gives the same bits
    m.train_heads_(False).train_detection_(False)
    g2, _ = _feature_run(m, f, K, idx, cr, co, cs)
    assert torch.equal(g1, g2) and all(p.grad is None for p in m.parameters())
    g3, _ = _feature_run(m, f, K, idx, cr, co, cs, train_heads=True, train_detection=True)      # the flags on, nothing to train
    assert torch.equal(g1, g3) and all(p.grad is None for p in m.parameters())
    # the two nodes' contributions add up
    gh, _ = _feature_run(m, f, K, idx, cr, co, None)
    gd, _ = _feature_run(m, f, K, idx, None, None, cs)
    assert torch.equal(gh + gd, g1)
    # without return_readout only the scores are attached
    fl = f.clone().requires_grad_()
    o3 = m.forward_features(fl, idx=idx, K=K, is_training=True)
    assert o3["scores"].requires_grad and not o3["offset"].requires_grad and "readout" not in o3
    (o3["scores"] * cs).sum().backward()
    assert torch.equal(fl.grad, gd)
    # inference mode attaches nothing
    assert not any(t.requires_grad for p in m.forward_features(fl, K=K, det_thresh=0.0)[:2] for t in p.values())


def test_no_person_leaves_the_detectors_term():
    m = _model()
    x, K, _ = _scene((0, 0), seed=930)
    none = tuple(torch.zeros(0, dtype=torch.long, device=dev()) for _ in range(3))
    cs = rn(torch.Generator().manual_seed(931), 2, GRID, GRID, 1).to(dev())
    f = m.backbone_features(x).clone()
    plain = m(x, idx=none, K=K, is_training=True, return_readout=True)
    got, out = _feature_run(m, f, K, none, None, None, cs)
    _same(plain, out)
    assert out["scores"].requires_grad and out["readout"].requires_grad and tuple(out["readout"].shape) == (0, NDEC)
    ref = _oracle(m, f, K, none, None, None, cs, 2)
    assert bool((got != 0).any())
    report("features no person", [("detector", ho.four_x(got.cpu(), ref[torch.float64]["detector"], ref[torch.float32]["detector"]))])
    # the empty read-out alone: a backward through it gives the features no gradient at all (autograd's zero)
    fl = f.clone().requires_grad_()
    o = m.forward_features(fl, idx=none, K=K, is_training=True, return_readout=True)
    o["readout"].sum().backward()
    assert fl.grad is None or bool((fl.grad == 0).all())


def test_descriptors_write_zeros_without_persons(L):
    """The C level with P == 0: mhmr_hph_backward and mhmr_xattn_layers_backward launch nothing else, but a given g_feat is written -- exact
    zeros in the B N rows x C block, nothing outside it; NULL leaves the call the no-op it was."""
    import ctypes as C
    B, N, C_ = 2, 256, 384
    f = _lib.HphDesc()
    f.dtype, f.C, f.G, f.N, f.Kc, f.dim, f.heads, f.mlp, f.depth, f.nb, f.Ktok, f.Ndec, f.patch, f.nearness = (
        _lib.DT_F16, C_, 16, N, 512, 1024, 8, 1024, 2, 10, 816, 341, 14, 1)
    f.cam_dim = 99
    d = _lib.HphBackwardDesc()
    d.fwd, d.P, d.B, d.ldg = C.pointer(f), 0, B, 341
    assert L.mhmr_hph_backward(C.byref(d), stream()) == 0                              # NULL g_feat: nothing happens
    sd = _lib.XattnBackwardDesc()
    sd.depth, sd.dim, sd.heads, sd.mlp, sd.Kc, sd.N, sd.B, sd.dtype, sd.P = 2, 1024, 8, 1024, 512, N, B, _lib.DT_F16, 0
    for call, desc in ((L.mhmr_hph_backward, d), (L.mhmr_xattn_layers_backward, sd)):
        buf = torch.full((B * N + 2, C_ + 4), float("nan"), dtype=torch.float32, device=dev())
        desc.g_feat, desc.ld_feat = _lib.f32p(buf), C_ + 4
        if desc is sd:
            desc.feat_cols = C_
        assert call(C.byref(desc), stream()) == 0
        assert bool((buf[:B * N, :C_] == 0).all()) and bool(torch.isnan(buf[B * N:]).all()) and bool(torch.isnan(buf[:, C_:]).all())


# ------------------------------------------------------------------------------------------------------ (6) guards
def test_guards():
    m = _model()
    x, K, idx = _scene((2, 1), seed=940)
    f = m.backbone_features(x).clone()
    train = dict(idx=idx, K=K, is_training=True, return_readout=True)
    msg = "before the next forward"
    # a backward after another forward_features of the same batch size
    fl = f.clone().requires_grad_()
    out = m.forward_features(fl, **train)
    m.forward_features(f, **train)
    with pytest.raises(_lib.MhmrError, match=msg):
        out["readout"].sum().backward()
    out = m.forward_features(fl, **train)
    m.forward_features(f, **train)
    with pytest.raises(_lib.MhmrError, match=msg):
        out["scores"].sum().backward()
    # forward invalidates forward_features' pending backward ...
    out = m.forward_features(fl, **train)
    m(x, **train)
    with pytest.raises(_lib.MhmrError, match=msg):
        out["readout"].sum().backward()
    # ... and forward_features invalidates forward's
    mt = _new_model().train_heads_(True)
    out = mt(x, train_heads=True, **train)
    mt.forward_features(f, **train)
    with pytest.raises(_lib.MhmrError, match=msg):
        out["readout"].sum().backward()
    # repack_heads() as well
    out = m.forward_features(fl, **train)
    m.repack_heads()
    with pytest.raises(_lib.MhmrError, match=msg):
        out["scores"].sum().backward()
    assert fl.grad is None
    # 16-bit features must not require grad; any float dtype without it is fine
    with pytest.raises(ValueError, match="float32"):
        m.forward_features(f.half().requires_grad_(), **train)
    with pytest.raises(ValueError, match="float32"):
        m.forward_features(f.double().requires_grad_(), **train)
    # wrong shapes, a CPU tensor, the keyword rules of forward, K of another batch size
    for bad in (f[:, :-1], f[:, :, :-1], f.reshape(-1), f.reshape(-1, 384)[:-1], f[None], f.long()):
        with pytest.raises(ValueError):
            m.forward_features(bad, **train)
    with pytest.raises(_lib.MhmrError, match="no CPU fallback"):
        m.forward_features(f.cpu(), **train)
    with pytest.raises(ValueError):
        m.forward_features(f, idx=idx, K=K, is_training=True, train_heads=True)
    with pytest.raises(ValueError):
        m.forward_features(f, K=K, return_readout=True, train_heads=True)
    with pytest.raises(ValueError):
        m.forward_features(f, K=K, train_detection=True)
    with pytest.raises(AssertionError):
        m.forward_features(f, idx=idx, K=K[:1], is_training=True)
    with pytest.raises(AssertionError):
        m(x, idx=idx, K=K[:1], is_training=True)                                        # (as forward does)


# ------------------------------------------------------------------------------------------------------ (7) one use
def test_ten_adam_steps_from_stored_features_lower_the_loss():
    """The backbone runs once; ten Adam steps on heads_parameters() from the stored features lower the training loss of the fixture
    scene, and the first step's loss is, bit for bit, the loss of the same step from the images."""
    import gt_oracle as go
    import loss_oracle as lo
    from multi_hmr_amd import BodyModel, GroundTruth, Loss
    a = _assets()
    m = _new_model().train_heads_(True)
    builder = GroundTruth(S, patch_size=14, smplx_neutral=BodyModel(a["data"], "smplx", num_betas=11))
    y = go.make_y("smplx", 51, S, [2, 1], depth=2.6)
    gt = builder.prepare({k: (v.to(dev()) if isinstance(v, torch.Tensor) else v) for k, v in y.items()})
    x = torch.randn(2, 3, S, S, generator=torch.Generator().manual_seed(0)).to(dev())
    loss, epoch = Loss(lo.default_args()), lo.DEFAULTS["start_2d_epoch"]

    def total(out):
        d = m.decode_readout(out["readout"], out["offset"], gt["idx"], gt["K"])
        return loss(dict(d, scores=out["scores"]), gt, epoch=epoch, img_size=S)[0]
    kw = dict(idx=gt["idx"], K=gt["K"], is_training=True, return_readout=True, train_heads=True)
    t_img = total(m(x, **kw))
    t_img.backward()
    g_img = [p.grad.clone() for p in m.heads_parameters()]
    f = m.backbone_features(x).clone()
    opt = torch.optim.Adam(m.heads_parameters(), lr=1e-4)
    losses = []
    for step in range(11):
        opt.zero_grad(set_to_none=True)
        t = total(m.forward_features(f, **kw))
        losses.append(float(t.detach()))
        if step == 0:
            assert torch.equal(t.detach(), t_img.detach()), (float(t), float(t_img))
        if step == 10:
            break
        t.backward()
        if step == 0:
            assert all(torch.equal(p.grad, g) for p, g in zip(m.heads_parameters(), g_img))
        opt.step()
        m.repack_heads()
    print("loss from stored features, steps 0..10: " + " ".join(f"{v:.6g}" for v in losses))
    assert all(v == v for v in losses) and losses[10] < losses[0]
