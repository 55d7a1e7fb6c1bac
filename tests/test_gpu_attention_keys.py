"""-m gpu: the ViT attention forms key by key, at every tail length, against fp64.

A one-hot V reads out the softmax weight of ONE key per output element (tests/attn_oracle.py), so a key that a mask drops, lets in or counts
twice moves an element by its whole size.  The gate is the 4x rule per element: |got - ref| <= 4 Y ref with Y the worst
relative error of a torch model of the 16-bit computation on the same inputs (checked against fp64 on the CPU by
tests/test_attention_oracle_host.py).  Padding -- key rows, V^T columns and query rows >= T, whatever `out` and `flags` held -- must not
reach a real row: bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from multi_hmr_amd import _lib  # noqa: E402
import attn_oracle as ao  # noqa: E402

DTYPES = [("f16", _lib.DT_F16), ("bf16", _lib.DT_BF16)]
#: the shipped forms: the self-contained banded form, variant 6 as mhmr_vit_forward runs it, variant 6 with (nearly) every workgroup handed
#: to the gated textbook pass, the textbook form alone, variant 6 into pitched rows with the bf8 copy (its 16-bit half is gated here)
FORMS = ["attention16", "variant6", "variant6_limit0", "variant1", "pitch"]
H, C = ao.H, ao.H * 64


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _lib.lib()


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def pads(T):
    """Tp = T rounded up to 64 and to 128 (once where both agree)."""
    return sorted({ao.roundup(T, 64), ao.roundup(T, 128)})


def run_form(L, form, qk, vt, B, T, Tp, dt, out_fill=0.0, flag_fill=7):
    """-> (out [B, Tp, C] as stored, flags or None).  `out` is pre-filled with out_fill, `flags` with flag_fill."""
    tdt = qk.dtype
    ldo = C + C // 2 if form == "pitch" else C
    out = torch.full((B * Tp, ldo), out_fill, dtype=tdt, device=dev())
    flags = None
    if form == "attention16":
        _lib.check(L.mhmr_attention16(qk.data_ptr(), vt.data_ptr(), out.data_ptr(), B, T, Tp, C, H, dt, stream()), form)
    elif form == "pitch":
        flags = torch.full((L.mhmr_attention_flag_count(B, Tp, H),), flag_fill, dtype=torch.int32, device=dev())
        _lib.check(L.mhmr_attention16_pitch(qk.data_ptr(), vt.data_ptr(), out.data_ptr(), B, T, Tp, C, H, dt, flags.data_ptr(), ldo, 2 * C, stream()), form)
    else:
        variant, limit = {"variant6": (6, 15.0), "variant6_limit0": (6, 0.0), "variant1": (1, 15.0)}[form]
        if variant == 6:
            flags = torch.full((L.mhmr_attention_flag_count(B, Tp, H),), flag_fill, dtype=torch.int32, device=dev())
        _lib.check(L.mhmr_attention16_ex(qk.data_ptr(), vt.data_ptr(), out.data_ptr(), B, T, Tp, C, H, dt, limit, variant,
                                         flags.data_ptr() if flags is not None else None, stream()), form)
    return out[:, :C].reshape(B, Tp, C), flags


def operands(q, k, v, T, Tp, fill=None):
    """q, k [T, H, 64] (shared by the images), v [B, Tp or T, H, 64] -> qk [B * Tp, 2 C], vt [B, H, 64, Tp] on the device.  fill = None: zeros
    in all padding; else a generator: K rows and V rows of keys >= T at +-3e4, Q rows >= T at +-2 (finite in both operand types, and no fp32
    score of theirs can overflow)."""
    B, tdt = v.shape[0], q.dtype
    qp, kp, vp = torch.zeros(B, Tp, H, 64), torch.zeros(B, Tp, H, 64), torch.zeros(B, Tp, H, 64)
    if fill is not None and Tp > T:
        sign = lambda: torch.randint(0, 2, (B, Tp - T, H, 64), generator=fill).float() * 2 - 1
        qp[:, T:], kp[:, T:], vp[:, T:] = 2.0 * sign(), 3e4 * sign(), 3e4 * sign()
    qp[:, :T], kp[:, :T], vp[:, :T] = q.float(), k.float(), v[:, :T].float()
    qk = torch.cat([qp.reshape(B * Tp, C), kp.reshape(B * Tp, C)], dim=1).to(tdt).contiguous().to(dev())
    return qk, ao.vt_layout(vp.to(tdt)).contiguous().to(dev())


def report(tag, rows):
    """rows: (name, kernel error, yardstick error, ratio, where, ok).  Print all, then assert all."""
    for name, err, yard, ratio, where, ok in rows:
        print(f"[{tag}] {name}: kernel {err:.3e} yardstick {yard:.3e} ratio {ratio:.2f} at {where}{'' if ok else '  <-- FAILS'}")
    bad = [(name, where) for name, _, _, _, where, ok in rows if not ok]
    assert not bad, (tag, bad)


def ratio_of(err, yard):
    return err / yard if yard > 0 else float("inf") if err > 0 else 0.0


# ------------------------------------------------------------------------------------------------------ (1) every key, every tail length
@pytest.mark.parametrize("name,dt", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_key_weights_at_every_tail_length(L, name, dt, form):
    """T = 1 ... 192 and the lengths of attn_oracle.T_KEYS, Tp = T rounded up to 64 and to 128: EVERY weight of every real query within 4 Y(T) of
    fp64, relatively; columns whose key does not exist are exact zeros; Y = 0 at T = 1 demands the exact bits."""
    tdt = ao.TDT[name]
    worst = dict(err=0.0, yard=0.0, ratio=0.0, where="-")
    failed = []
    for T in ao.T_KEYS:
        c = ao.key_case(T, name)
        ref = ao.expected_readout(c["w"], T, ao.E16)                       # [windows, T, C]
        for Tp in pads(T):
            v = ao.window_v(T, Tp, tdt, ao.E16)
            qk, vt = operands(c["q"], c["k"], v, T, Tp)
            out, _ = run_form(L, form, qk, vt, v.shape[0], T, Tp, dt)
            got = out[:, :T].double().cpu()
            assert torch.isfinite(got).all(), (T, Tp)
            diff = (got - ref).abs()
            err = ao.worst_rel(got, ref)
            ok = bool((diff <= 4 * c["Y"] * ref).all())
            r = ratio_of(err, c["Y"])
            if r > worst["ratio"] or (r == worst["ratio"] and err > worst["err"]):
                worst = dict(err=err, yard=c["Y"], ratio=r, where=f"T {T} Tp {Tp}")
            if not ok:
                failed.append((T, Tp, err, c["Y"], int((diff > 4 * c["Y"] * ref).sum())))
    print(f"[attention keys {form} {name}] failing (T, Tp, kernel, yardstick, elements): {failed[:40]}{' ...' if len(failed) > 40 else ''}")
    report(f"attention keys {form} {name}", [("weights", worst["err"], worst["yard"], worst["ratio"], worst["where"], not failed)])


# ------------------------------------------------------------------------------------------------------ (2) padding
@pytest.mark.parametrize("name,dt", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_padding_cannot_reach_a_real_row(L, name, dt, form):
    """Run A: zeros in all padding, `out` zeroed.  Run B: K and V padding at +-3e4, Q padding rows at +-2, `out` full of NaN, `flags` full of 7.
    The real rows of B are the bits of A (a masked score is -inf behind the MFMA, so its p is an exact 0), finite, and every flag is written."""
    tdt = ao.TDT[name]
    unequal, stale, nonfinite = [], [], []
    for T in ao.T_PAD:
        c = ao.key_case(T, name)
        v = ao.v_inputs(T, name, 2)
        for Tp in pads(T):
            qkA, vtA = operands(c["q"], c["k"], v, T, Tp)
            qkB, vtB = operands(c["q"], c["k"], v, T, Tp, fill=torch.Generator().manual_seed(T + Tp))
            a, _ = run_form(L, form, qkA, vtA, 2, T, Tp, dt)
            b, flags = run_form(L, form, qkB, vtB, 2, T, Tp, dt, out_fill=float("nan"), flag_fill=7)
            a, b = a[:, :T], b[:, :T]
            if not torch.equal(a.view(torch.int16), b.view(torch.int16)):
                unequal.append((T, Tp, int((a.view(torch.int16) != b.view(torch.int16)).any(-1).sum())))
            if not bool(torch.isfinite(b.float()).all()):
                nonfinite.append((T, Tp))
            if flags is not None and int((flags == 7).sum()) > 0:
                stale.append((T, Tp))
    print(f"[attention padding {form} {name}] rows that differ (T, Tp, rows): {unequal}; non-finite: {nonfinite}; stale flags: {stale}")
    assert not unequal and not nonfinite and not stale


# ------------------------------------------------------------------------------------------------------ (3) ordinary V
@pytest.mark.parametrize("name,dt", DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_ordinary_values_under_the_4x_rule(L, name, dt, form):
    """Random V: the maximum absolute error of the tensor <= 4x the yardstick's on the same operands (next to the flat bounds of
    test_gpu_kernels.py::test_attention, which stay)."""
    rows = []
    for T in ao.T_PLAIN:
        c = ao.key_case(T, name)
        v = ao.v_inputs(T, name, 2, seed=1)
        ref = ao.attention64(c["q"], c["k"], v)
        yard = float((ao.yardstick16(c["q"], c["k"], v).double() - ref).abs().max())
        for Tp in pads(T):
            qk, vt = operands(c["q"], c["k"], v, T, Tp)
            out, _ = run_form(L, form, qk, vt, 2, T, Tp, dt)
            err = float((out[:, :T].double().cpu() - ref).abs().max())
            rows.append((f"T {T}", err, yard, ratio_of(err, yard), f"Tp {Tp}", err <= 4 * yard))
    report(f"attention values {form} {name}", rows)


# ------------------------------------------------------------------------------------------------------ (4) mhmr_attention_f32
def run_f32(L, q, k, v, T, Tp, dt, tdt, fill=None):
    """q, k [T, H, 64] fp32 un-scaled, v [B, Tp, H, 64] -> out [B, Tp, 2 C] (the [hi | lo] pair), `out` pre-filled with NaN."""
    B = v.shape[0]
    x = torch.zeros(B, Tp, 3, H, 64)
    if fill is not None and Tp > T:
        sign = lambda: torch.randint(0, 2, (B, Tp - T, H, 64), generator=fill).float() * 2 - 1
        x[:, T:, 0], x[:, T:, 1], x[:, T:, 2] = 2.0 * sign(), 3e4 * sign(), 3e4 * sign()
    x[:, :T, 0], x[:, :T, 1], x[:, :T, 2] = q, k, v[:, :T].float()
    qkv = x.reshape(B * Tp, 3 * C).contiguous().to(dev())
    out = torch.full((B * Tp, 2 * C), float("nan"), dtype=tdt, device=dev())
    _lib.check(L.mhmr_attention_f32(qkv.data_ptr(), out.data_ptr(), B, T, Tp, C, H, dt, stream()), "attention_f32")
    return out.reshape(B, Tp, 2 * C)


@pytest.mark.parametrize("name,dt", DTYPES)
def test_f32_key_weights_at_every_tail_length(L, name, dt):
    """mhmr_attention_f32, T = 1 ... 130 and 257: every weight (hi + lo) within 4 Y(T) of fp64, Y from plain fp32 torch stored as the same
    pair; `out` starts as NaN and every row of it, padding included, ends finite."""
    tdt = ao.TDT[name]
    worst = dict(err=0.0, yard=0.0, ratio=0.0, where="-")
    failed = []
    for T in ao.T_F32:
        c = ao.key_case32(T, name)
        ref = ao.expected_readout(c["w"], T, ao.E32)
        for Tp in pads(T):
            v = ao.window_v(T, Tp, torch.float32, ao.E32)
            out = run_f32(L, c["q"], c["k"], v, T, Tp, dt, tdt)
            assert bool(torch.isfinite(out.float()).all()), (T, Tp)
            got = (out[:, :T, :C].double() + out[:, :T, C:].double()).cpu()
            diff = (got - ref).abs()
            err = ao.worst_rel(got, ref)
            ok = bool((diff <= 4 * c["Y"] * ref).all())
            r = ratio_of(err, c["Y"])
            if r > worst["ratio"] or (r == worst["ratio"] and err > worst["err"]):
                worst = dict(err=err, yard=c["Y"], ratio=r, where=f"T {T} Tp {Tp}")
            if not ok:
                failed.append((T, Tp, err, c["Y"], int((diff > 4 * c["Y"] * ref).sum())))
    print(f"[attention_f32 keys {name}] failing (T, Tp, kernel, yardstick, elements): {failed[:40]}{' ...' if len(failed) > 40 else ''}")
    report(f"attention_f32 keys {name}", [("weights", worst["err"], worst["yard"], worst["ratio"], worst["where"], not failed)])


@pytest.mark.parametrize("name,dt", DTYPES)
def test_f32_padding_cannot_reach_a_real_row(L, name, dt):
    """mhmr_attention_f32 with zeros against +-3e4 / +-2 in the padding rows of K, V / Q: the real rows are the same bits, the whole buffer
    (it started as NaN) is finite."""
    tdt = ao.TDT[name]
    unequal, nonfinite = [], []
    for T in ao.T_F32:
        c = ao.key_case32(T, name)
        v = ao.v_inputs(T, "f16", 2, seed=2).float()
        for Tp in pads(T):
            a = run_f32(L, c["q"], c["k"], v, T, Tp, dt, tdt)
            b = run_f32(L, c["q"], c["k"], v, T, Tp, dt, tdt, fill=torch.Generator().manual_seed(T + Tp))
            if not torch.equal(a[:, :T].view(torch.int16), b[:, :T].view(torch.int16)):
                unequal.append((T, Tp))
            if not bool(torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all()):
                nonfinite.append((T, Tp))
    print(f"[attention_f32 padding {name}] rows that differ (T, Tp): {unequal}; non-finite: {nonfinite}")
    assert not unequal and not nonfinite
