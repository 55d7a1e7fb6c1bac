"""-m gpu: the device re-pack of the derived encoder operands through the C ABI (csrc/encoder_pack.hip, mhmr_vit_repack; DESIGN.md
section 34), every target between sentinels and with sentinels in its padding.

Row job: the 16-bit operand, the [hi | lo] rows and the triple are bit-equal to the cast / ``vit.hi_lo`` / ``vit.triple`` of the folded
weight as ``vit.pack_block`` forms it; the f16 column sum is bit-equal to ``pack_block``'s formula; the folded bias and the bf16 column sum
are bit-equal to the fixed-order oracle (tests/encoder_pack_oracle.py) and within one fp32 ulp of the fp64 torch value.  Position job:
bit-equal to the oracle, within one ulp of ``packing.interpolate_pos_embed``."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import encoder_pack_oracle as eo  # noqa: E402
import optim_oracle as oo  # noqa: E402
from multi_hmr_amd import _lib, packing, vit  # noqa: E402

GUARD, SENT = 16, 77.0
TDT = {"f16": torch.float16, "bf16": torch.bfloat16}
KIND = {"f16": _lib.ADAM_PACK_F16, "bf16": _lib.ADAM_PACK_BF16}
FORM = {None: _lib.PACK_LO_NONE, "pair": _lib.PACK_LO_PAIR, "triple": _lib.PACK_LO_TRIPLE}
SHAPES = [(7, 64), (33, 384), (16, 1024), (5, 1536)]


def dev():
    return torch.device("cuda:0")


class Buf:
    """n elements between sentinels; ``mis`` moves the data off its 16-byte boundary by that many elements."""

    def __init__(self, n, dtype, mis=0, init=None):
        self.t = torch.full((n + 2 * GUARD + 4,), SENT, dtype=dtype, device=dev())
        self.o, self.n = GUARD + mis, n
        if init is not None:
            self.t[self.o:self.o + n] = init.reshape(-1).to(dev())

    @property
    def ptr(self):
        return self.t.data_ptr() + self.o * self.t.element_size()

    def data(self):
        return self.t[self.o:self.o + self.n]

    def guards_ok(self):
        return bool((self.t[:self.o] == SENT).all()) and bool((self.t[self.o + self.n:] == SENT).all())


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _launch(L, jobs):
    host = (_lib.PackJob * len(jobs))(*jobs)
    table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev())
    rc = L.mhmr_vit_repack(host, table.data_ptr(), len(jobs), torch.cuda.current_stream(dev()).cuda_stream)
    torch.cuda.synchronize()
    return rc


def _values(N, K, seed):
    """N(0, 0.02) weights, LayerNorm weights around 1; row 1 a thousand times smaller (its low half is far below the f16 normal range),
    row 2 a hundred thousand times smaller (its HIGH half is subnormal in f16), the last row zero."""
    g = torch.Generator().manual_seed(seed)
    W = 0.02 * torch.randn(N, K, generator=g)
    W[1] *= 1e-3
    W[2] *= 1e-5
    W[N - 1] = 0.0
    return W, 1.0 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(N, generator=g)


def run_row(L, N, K, tdt, fold, form, mis=0, seed=3):
    """One row job.  -> the bit patterns of every target (data between the sentinels), after every check against the references."""
    W, lw, lb, b = _values(N, K, seed + N)
    pitch, row_off, sec = K + 8, 2, K + 8
    sections = {None: 0, "pair": 2, "triple": 3}[form]
    lo_rows = (1, N - 2) if form == "pair" else (0, N)                   # the pair on a sub-range of the rows, the triple on all
    lo_pitch = sections * sec + 8
    bw, blw, blb, bb = Buf(N * K, torch.float32, mis, W), Buf(K, torch.float32, mis, lw), Buf(K, torch.float32, mis, lb), Buf(N, torch.float32, 0, b)
    t16 = Buf((N + row_off + 1) * pitch, TDT[tdt])
    tlo = Buf(max(lo_rows[1] * lo_pitch, 1), TDT[tdt])
    tb, tc = Buf(N, torch.float32), Buf(N, torch.float32)
    j = _lib.PackJob()
    j.kind, j.dtype, j.N, j.K, j.pitch16 = _lib.PACK_ROW, KIND[tdt], N, K, pitch
    j.w, j.w16, j.colsum = bw.ptr, t16.ptr + row_off * pitch * 2, tc.ptr
    if fold:
        j.ln_w, j.ln_b, j.bias, j.bias_out = blw.ptr, blb.ptr, bb.ptr, tb.ptr
    if form:
        j.lo, j.lo_form, j.lo_row0, j.lo_rows, j.lo_section, j.lo_pitch = tlo.ptr, FORM[form], lo_rows[0], lo_rows[1], sec, lo_pitch
    assert _launch(L, [j]) == 0
    for x in (bw, blw, blb, bb, t16, tlo, tb, tc):
        assert x.guards_ok()
    # ---- pack_block's formulas on the same tensors
    Wf = (W.double() * lw.double()[None, :]).float() if fold else W
    W16 = Wf.to(TDT[tdt])
    got16 = t16.data().reshape(N + row_off + 1, pitch).cpu()
    assert np.array_equal(oo.bits(got16[row_off:row_off + N, :K]), oo.bits(W16)), "16-bit operand"
    untouched = torch.ones_like(got16, dtype=torch.bool)
    untouched[row_off:row_off + N, :K] = False
    assert bool((got16[untouched] == SENT).all()), "padding of the 16-bit operand written"
    colsum = W16.double().sum(1)
    if form:
        r0, n = lo_rows
        want = (vit.hi_lo if form == "pair" else vit.triple)(Wf[r0:r0 + n], TDT[tdt])
        got = tlo.data().reshape(n, lo_pitch).cpu()
        for s in range(sections):
            assert np.array_equal(oo.bits(got[:, s * sec:s * sec + K]), oo.bits(want[:, s * K:(s + 1) * K])), ("low half", s)
            assert bool((got[:, s * sec + K:(s + 1) * sec] == SENT).all())
        assert bool((got[:, sections * sec:] == SENT).all())
        if form == "pair":
            colsum[r0:r0 + n] = want.double().sum(1)
    else:
        assert bool((tlo.t == SENT).all())
    ref = eo.row_job(W.numpy(), TDT[tdt], ln_w=lw.numpy() if fold else None, ln_b=lb.numpy() if fold else None, bias=b.numpy() if fold else None,
                     lo_form=form, lo_rows=lo_rows if form else None, want_sums=True)
    got_c = tc.data().cpu().numpy()
    assert np.array_equal(got_c.view(np.int32), ref["colsum"].view(np.int32)), "column sum against the oracle"
    d = eo.ulp_distance(got_c, colsum.float().numpy())
    assert d.max() <= (0 if tdt == "f16" else 1), ("column sum against pack_block", int(d.max()))
    off = dict(colsum=int((d > 0).sum()), bias=0)
    if fold:
        got_b = tb.data().cpu().numpy()
        assert np.array_equal(got_b.view(np.int32), ref["bias"].view(np.int32)), "folded bias against the oracle"
        d = eo.ulp_distance(got_b, (b.double() + W.double() @ lb.double()).float().numpy())
        assert d.max() <= 1, ("folded bias against torch", int(d.max()))
        off["bias"] = int((d > 0).sum())
    else:
        assert bool((tb.t == SENT).all())
    return [oo.bits(x.data()) for x in (t16, tlo, tb, tc)], off


@pytest.mark.parametrize("tdt", ["f16", "bf16"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_row_job(L, N, K, tdt):
    """Fold on and off; no low half, a pair on rows 1 .. N-2, the triple; a pitch 8 wider than K at a row offset of 2; two calls and a
    weight 4 bytes off its 16-byte boundary give the same bits."""
    moved = dict(colsum=0, bias=0)
    for fold in (False, True):
        for form in (None, "pair", "triple"):
            a, off = run_row(L, N, K, tdt, fold, form)
            b, _ = run_row(L, N, K, tdt, fold, form)
            c, _ = run_row(L, N, K, tdt, fold, form, mis=1)
            for x, y, z in zip(a, b, c):
                assert np.array_equal(x, y) and np.array_equal(x, z), (fold, form)
            moved = {k: moved[k] + off[k] for k in moved}
    print(f"\nrow job {N}x{K} {tdt}: elements one ulp from pack_block's order: {moved}")


def test_low_half_values_are_subnormal_and_kept(L):
    """The fixture does hold f16 low halves below the normal range that are not zero, and a subnormal high half: they come out bit-equal
    (inside run_row); this test pins that the case is present."""
    W, _, _, _ = _values(7, 64, 3 + 7)
    pair = vit.hi_lo(W, torch.float16)
    lo, hi = pair[:, 64:].float().abs(), pair[:, :64].float().abs()
    assert int(((lo > 0) & (lo < 6.1035e-5)).sum()) > 100 and int(((hi[2] > 0) & (hi[2] < 6.1035e-5)).sum()) > 10 and not pair[6].any()


def test_two_jobs_in_one_table(L):
    """Jobs of different lengths share one launch: rows 0..6 of the first, 7..39 of the second (a workgroup of four waves straddles them)."""
    outs = []
    for seed in (0, 1):
        jobs, bufs = [], []
        row0 = 0
        for N, K in ((7, 64), (33, 384)):
            W, lw, lb, b = _values(N, K, 11 + N)
            bw, t16, tc = Buf(N * K, torch.float32, 0, W), Buf(N * K, torch.float16), Buf(N, torch.float32)
            j = _lib.PackJob()
            j.kind, j.dtype, j.N, j.K, j.pitch16, j.row0 = _lib.PACK_ROW, _lib.ADAM_PACK_F16, N, K, K, row0
            j.w, j.w16, j.colsum = bw.ptr, t16.ptr, tc.ptr
            row0 += N
            jobs.append(j)
            bufs.append((W, bw, t16, tc))
        assert _launch(L, jobs) == 0
        for W, bw, t16, tc in bufs:
            assert t16.guards_ok() and tc.guards_ok()
            assert np.array_equal(oo.bits(t16.data()), oo.bits(W.to(torch.float16)))
            assert np.array_equal(oo.bits(tc.data()), oo.bits(W.to(torch.float16).double().sum(1).float()))
        outs.append([oo.bits(x[2].data()) for x in bufs])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("M,G,Cd", [(37, 16, 384), (37, 5, 64), (16, 16, 64)])
def test_position_job(L, M, G, Cd):
    g = torch.Generator().manual_seed(M + G)
    pe, cls = 0.02 * torch.randn(1, 1 + M * M, Cd, generator=g), torch.randn(1, 1, Cd, generator=g)
    w, idx = packing._cubic_taps(M, G)
    bpe, bcls = Buf(pe.numel(), torch.float32, 0, pe), Buf(Cd, torch.float32, 0, cls)
    tw, ti = torch.from_numpy(w).to(dev()).contiguous(), torch.from_numpy(idx.astype(np.int32)).to(dev()).contiguous()
    outs = []
    for _ in range(2):
        tpos, tcls = Buf((1 + G * G) * Cd, torch.float32), Buf(Cd, torch.float32)
        j = _lib.PackJob()
        j.kind, j.M, j.G, j.C = _lib.PACK_POS, M, G, Cd
        j.pos_embed, j.cls_token, j.pos, j.cls_pos0 = bpe.ptr, bcls.ptr, tpos.ptr, tcls.ptr
        if G != M:
            j.tap_w, j.tap_i = tw.data_ptr(), ti.data_ptr()
        assert _launch(L, [j]) == 0
        assert all(x.guards_ok() for x in (bpe, bcls, tpos, tcls))
        outs.append((oo.bits(tpos.data()), oo.bits(tcls.data())))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    pos, cls0 = eo.pos_job(pe.numpy(), cls.numpy(), G)
    assert np.array_equal(outs[0][0], pos.reshape(-1).view(np.int32)) and np.array_equal(outs[0][1], cls0.view(np.int32))
    ref = packing.interpolate_pos_embed(pe.numpy(), G)
    d = eo.ulp_distance(outs[0][0].view(np.float32), ref.reshape(-1))
    assert d.max() <= (0 if G == M else 1)
    assert np.array_equal(outs[0][1], (cls.reshape(-1).numpy() + ref[0]).view(np.int32))
    print(f"\nposition job M={M} G={G} C={Cd}: {int((d > 0).sum())} of {d.size} elements one ulp from interpolate_pos_embed")


def test_bad_arguments_leave_every_buffer_alone(L):
    """A low-half form without its target, a K that is no multiple of four, two targets that overlap: the documented code, no byte changes."""
    N, K = 8, 64
    W = torch.randn(N, K)
    bufs = dict(w=Buf(N * K, torch.float32, 0, W), w16=Buf(N * K, torch.float16), lo=Buf(2 * N * K, torch.float16), colsum=Buf(N, torch.float32))
    before = {k: oo.bits(b.t) for k, b in bufs.items()}

    def job(**kw):
        j = _lib.PackJob()
        j.kind, j.dtype, j.N, j.K, j.pitch16 = _lib.PACK_ROW, _lib.ADAM_PACK_F16, N, K, K
        j.w, j.w16, j.colsum = bufs["w"].ptr, bufs["w16"].ptr, bufs["colsum"].ptr
        for k, v in kw.items():
            setattr(j, k, v)
        return j
    lo = dict(lo_form=_lib.PACK_LO_PAIR, lo_rows=N, lo_section=K, lo_pitch=2 * K)
    for kw, want in ((dict(lo, lo=None), -1), (dict(K=62, pitch16=62), -2), (dict(lo, lo=bufs["w16"].ptr + 2 * K), -1),
                     (dict(colsum=bufs["w16"].ptr), -1)):
        assert _launch(L, [job(**kw)]) == want, kw
    assert _launch(L, [job(), job(row0=N, w16=bufs["lo"].ptr, colsum=bufs["colsum"].ptr + 4)]) == -1
    assert all(np.array_equal(oo.bits(b.t), before[k]) for k, b in bufs.items())
