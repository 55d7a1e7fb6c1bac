"""-m gpu: the fused Adam step (csrc/optim.hip through the C ABI, then ``HeadsAdam`` on the ViT-S fixture).

Kernel alone, on synthetic segments: element counts 1, 3, 255, 256, 257 and 4099 (one element; less than a 16-byte group; around one
workgroup's 256 threads; three chunks with a tail of 3), a pitch of 8 with 5 columns at a row offset into a larger buffer, f16 and bf16
copies, two pair segments, a constant addend, a skipped segment, per-tensor step counts, gradients with exact zeros, subnormal second
moments (an fp32 square root is never subnormal -- sqrt(2^-149) is 3.7e-23 -- so the case is the moment itself: the root, the division and
the products must not flush it), every buffer between sentinels, and every pointer once on 16 bytes and once 4 (2) bytes off it.

Accuracy gate: the 4x rule of DESIGN.md section 16 -- the maximum absolute error of parameter and moments against the fp64 oracle
(tests/optim_oracle.py) is at most 4x that of torch.optim.Adam in fp32 on the CPU from the same state.  Both figures are printed."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import optim_oracle as oo  # noqa: E402
from multi_hmr_amd import _lib  # noqa: E402
from multi_hmr_amd.optim import HeadsAdam, bias_corrections  # noqa: E402

GUARD, SENT = 16, 77.0
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
KIND = {None: _lib.ADAM_PACK_NONE, "f32": _lib.ADAM_PACK_F32, "f16": _lib.ADAM_PACK_F16, "bf16": _lib.ADAM_PACK_BF16}
SPECS = [dict(n=1, kind="f32"), dict(n=3, kind="f16"), dict(n=255, kind="bf16"), dict(n=256, kind="f32", addend=True),
         dict(n=257, kind="f32", pair="same"), dict(n=4099, kind="f32", step0=5, tiny=True),
         dict(n=40, kind="f32", cols=5, pitch=8, row_off=2, rows_total=12), dict(n=40, kind="f16", cols=5, pitch=8),
         dict(n=4096, kind="bf16", cols=64, pitch=72), dict(n=300, kind="f32", inactive=True), dict(n=4099, kind=None),
         dict(n=256, kind="f16", pair="own", step0=1, step0b=3)]


def dev():
    return torch.device("cuda:0")


def report(tag, rows):
    print(f"\n{tag}")
    for r in rows:
        print("   " + "  ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in r.items()))


class Buf:
    """n elements between sentinels; `mis` moves the data off its 16-byte boundary by that many elements."""

    def __init__(self, n, dtype, mis=0, init=None):
        self.t = torch.full((n + 2 * GUARD + 4,), SENT, dtype=dtype, device=dev())
        self.o, self.n = GUARD + mis, n
        if init is not None:
            self.t[self.o:self.o + n] = init.to(dev())

    @property
    def ptr(self):
        return self.t.data_ptr() + self.o * self.t.element_size()

    def data(self):
        return self.t[self.o:self.o + self.n]

    def guards_ok(self):
        return bool((self.t[:self.o] == SENT).all()) and bool((self.t[self.o + self.n:] == SENT).all())


def _bits(t):
    return oo.bits(t)


def _initial(seed):
    """CPU state and three steps of gradients for every tensor of SPECS (a pair has two)."""
    g = torch.Generator().manual_seed(seed)
    segs = []
    for sp in SPECS:
        n = sp["n"]
        tensors = []
        for which in range(2 if sp.get("pair") else 1):
            p, m, v = torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g), (0.1 * torch.randn(n, generator=g)) ** 2
            grads = [torch.randn(n, generator=g) for _ in range(3)]
            for gr in grads:
                gr[::7] = 0.0                                            # exact zeros
            if sp.get("tiny"):
                v[:8], m[:8] = 1e-42, 1e-21                              # a subnormal second moment
                grads[0][:8], grads[1][:8], grads[2][:8] = 0.0, 1e-22, 0.0
                assert 0 < float(v[0]) < 1.1754944e-38
            tensors.append(dict(p=p, m=m, v=v, step=sp.get("step0b" if which else "step0", 0), grads=grads))
        if sp.get("pair") == "same":
            tensors[1]["grads"] = tensors[0]["grads"]
        segs.append(dict(spec=sp, tensors=tensors, addend=torch.randn(n, generator=g) if sp.get("addend") else None))
    return segs


def _expected_packed(sp, new_p, addend):
    x = new_p[0]
    if len(new_p) == 2:
        x = x + new_p[1]
    if addend is not None:
        x = x + addend
    return _bits(x.to(TDT[sp["kind"]]))


def _torch_step(state, grads, max_norm):
    """One step of torch.optim.Adam (single-tensor form) in fp32 on the CPU from `state`."""
    params = [torch.nn.Parameter(st["p"].clone()) for st in state]
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS, foreach=False)
    for p, st, g in zip(params, state, grads):
        p.grad = None if g is None else g.clone()
        opt.state[p] = dict(step=torch.tensor(float(st["step"])), exp_avg=st["m"].clone(), exp_avg_sq=st["v"].clone())
    norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)) if max_norm else None
    opt.step()
    return [dict(p=p.detach(), m=opt.state[p]["exp_avg"], v=opt.state[p]["exp_avg_sq"]) for p in params], norm


def run_scenario(L, mis, max_norm=None, check=False, seed=5, steps=3):
    """The three steps on the GPU.  -> the bit patterns of every buffer after each step (a flat list)."""
    segs = _initial(seed)
    nseg = len(segs)
    host = (_lib.AdamSegment * nseg)()
    bufs, chunk0 = [], 0
    for sg in segs:
        sp = sg["spec"]
        b = dict(state=[{k: Buf(sp["n"], torch.float32, mis, t[k]) for k in ("p", "m", "v")} for t in sg["tensors"]],
                 grads=[[Buf(sp["n"], torch.float32, mis, gr) for gr in t["grads"]] for t in sg["tensors"]],
                 addend=Buf(sp["n"], torch.float32, mis, sg["addend"]) if sg["addend"] is not None else None, packed=None, chunk0=chunk0)
        if sp["kind"]:
            cols, pitch = sp.get("cols", 1), sp.get("pitch", 1)
            rows = sp["n"] // cols
            total = sp.get("rows_total", rows) * pitch if pitch > 1 else sp["n"]
            b["packed"] = Buf(total, TDT[sp["kind"]], mis)
            i = torch.arange(sp["n"])
            b["idx"] = (sp.get("row_off", 0) * pitch + (i // cols) * pitch + i % cols).to(dev())
        chunk0 += -(-sp["n"] // _lib.ADAM_CHUNK)
        bufs.append(b)
    partials = torch.full((chunk0 + 2,), -1.0, dtype=torch.float64, device=dev())
    norm_out = torch.full((3,), SENT, device=dev())
    table = torch.empty(C.sizeof(host), dtype=torch.uint8, device=dev())
    stream = torch.cuda.current_stream(dev()).cuda_stream
    out, rows = [], []
    for step in range(steps):
        for seg, sg, b in zip(host, segs, bufs):
            sp, t0 = sg["spec"], sg["tensors"][0]
            st = b["state"][0]
            seg.param, seg.exp_avg, seg.exp_avg_sq = st["p"].ptr, st["m"].ptr, st["v"].ptr
            seg.grad = None if sp.get("inactive") else b["grads"][0][step].ptr
            seg.step_size, seg.bc2_sqrt = bias_corrections(t0["step"] + step + 1, LR, *BETAS)
            if sp.get("pair"):
                s2 = b["state"][1]
                seg.param2, seg.exp_avg2, seg.exp_avg_sq2 = s2["p"].ptr, s2["m"].ptr, s2["v"].ptr
                seg.grad2 = b["grads"][0 if sp["pair"] == "same" else 1][step].ptr
                seg.step_size2, seg.bc2_sqrt2 = bias_corrections(sg["tensors"][1]["step"] + step + 1, LR, *BETAS)
            seg.addend = b["addend"].ptr if b["addend"] is not None else None
            seg.n, seg.cols, seg.pitch, seg.packed_kind, seg.chunk0 = sp["n"], sp.get("cols", 1), sp.get("pitch", 1), KIND[sp["kind"]], b["chunk0"]
            if b["packed"] is not None:
                seg.packed = b["packed"].ptr + sp.get("row_off", 0) * sp.get("pitch", 1) * b["packed"].t.element_size()
        table.copy_(torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8))
        before = None
        if check:      # the state this step starts from, as the GPU holds it
            before = [[{k: st[k].data().cpu() for k in ("p", "m", "v")} for st in b["state"]] for b in bufs]
        rc = L.mhmr_adam_step(host, table.data_ptr(), nseg, BETAS[0], BETAS[1], EPS, max_norm or 0.0,
                              partials.data_ptr() if max_norm else None, chunk0 if max_norm else 0, norm_out.data_ptr(), stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        for b in bufs:
            for st in b["state"]:
                out += [_bits(st[k].data()) for k in ("p", "m", "v")]          # (the data, not the guards: `mis` moves it)
            if b["packed"] is not None:
                out.append(_bits(b["packed"].data()))
        out += [_bits(norm_out), partials.cpu().numpy().view(np.int64).copy()]
        if not check:
            continue
        # ---- sentinels, skipped segments, packed copies
        flat_state, flat_grads, owners = [], [], []
        for sg, b, bef in zip(segs, bufs, before):
            sp = sg["spec"]
            for bb in [x for st in b["state"] for x in st.values()] + [x for gs in b["grads"] for x in gs] + ([b["addend"]] if b["addend"] else []):
                assert bb.guards_ok(), sp
            new_p = [st["p"].data().cpu() for st in b["state"]]
            if sp.get("inactive"):
                for st, old in zip(b["state"], bef):
                    assert all(np.array_equal(_bits(st[k].data()), _bits(old[k])) for k in ("p", "m", "v")), sp
                assert bool((b["packed"].t == SENT).all())
                flat_state.append(dict(bef[0], step=0))
                flat_grads.append(None)
                owners.append((b, 0))
                continue
            if b["packed"] is not None:
                pk = b["packed"]
                assert pk.guards_ok(), sp
                claimed = torch.zeros(pk.n, dtype=torch.bool, device=dev())
                claimed[b["idx"]] = True
                assert int(claimed.sum()) == sp["n"]
                assert bool((pk.data()[~claimed] == SENT).all()), ("padding written", sp)
                got = _bits(pk.data()[b["idx"]])
                assert np.array_equal(got, _expected_packed(sp, new_p, sg["addend"])), ("packed copy", sp)
            for w, t in enumerate(sg["tensors"]):
                flat_state.append(dict(bef[w], step=t["step"] + step))
                flat_grads.append(t["grads"][step])
                owners.append((b, w))
        if not max_norm:
            assert bool((norm_out == SENT).all()) and bool((partials == -1.0).all())       # not touched without the clip
        else:
            assert float(norm_out[1]) == SENT and float(partials[chunk0]) == -1.0
        # ---- accuracy: ours and torch's fp32 CPU step against fp64, from the same state
        ref, ref_norm = oo.adam_step([dict(p=s["p"].numpy(), m=s["m"].numpy(), v=s["v"].numpy(), step=s["step"]) for s in flat_state],
                                     [None if g is None else g.numpy() for g in flat_grads], LR, BETAS, EPS, max_norm)
        tor, tor_norm = _torch_step(flat_state, flat_grads, max_norm)
        row = dict(step=step + 1)
        for k in ("p", "m", "v"):
            e_us = max(float(np.max(np.abs(b["state"][w][k].data().cpu().double().numpy() - r[k]))) for (b, w), r in zip(owners, ref))
            e_t = max(float(np.max(np.abs(t[k].double().numpy() - r[k]))) for t, r in zip(tor, ref))
            row.update({f"{k}_ours": e_us, f"{k}_torch": e_t})
            assert e_us <= 4.0 * e_t, (step, k, e_us, e_t)
        if max_norm:
            e_us, e_t = abs(float(norm_out[0].double()) - ref_norm), abs(tor_norm - ref_norm)
            row.update(norm_ours=e_us, norm_torch=e_t, norm=ref_norm)
            assert e_us <= 4.0 * e_t, (e_us, e_t)
        rows.append(row)
    if check:
        report(f"adam step, synthetic segments, pointers {'4 / 2 bytes off' if mis else 'on'} 16 bytes, max_norm {max_norm}: max abs error vs fp64", rows)
    return out


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def _aligned_bits(max_norm):
    return run_scenario(_lib.lib(), 0, max_norm, check=True)


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), i


def test_synthetic_segments_against_fp64(L):
    _aligned_bits(None)


def test_two_runs_give_the_same_bits(L):
    _same(_aligned_bits(None), run_scenario(L, 0))
    _same(_aligned_bits(0.5), run_scenario(L, 0, 0.5))


@pytest.mark.parametrize("max_norm", [None, 0.5])
def test_misaligned_pointers_give_the_same_bits(L, max_norm):
    """Every pointer one element off its 16-byte boundary: the element-by-element form, checked on its own and against the 16-byte form."""
    _same(_aligned_bits(max_norm), run_scenario(L, 1, max_norm, check=True))


def test_clip(L):
    """max_norm 0.5 clips (the gradient norm of the table is ~ 120): norm and update against fp64 inside run_scenario.  With the norm
    below max_norm the update is the unclipped one, bit for bit (the norm buffers differ: they are written)."""
    _aligned_bits(0.5)
    a, b = _aligned_bits(None), run_scenario(L, 0, 1e6)
    per_step = len(a) // 3
    for i, (x, y) in enumerate(zip(a, b)):
        if i % per_step < per_step - 2:
            assert np.array_equal(x, y), i
    c = _aligned_bits(0.5)                                                      # and the clip at 0.5 did change the update
    assert sum(int(not np.array_equal(x, y)) for x, y in zip(c[:per_step - 2], a[:per_step - 2])) > per_step // 2


def test_bad_arguments_leave_every_buffer_alone(L):
    """A wrong first chunk, an overlap, a zero count, a missing norm buffer: the documented code, and no byte changes."""
    n = 600
    bufs = {k: Buf(n, torch.float32, 0, torch.randn(n)) for k in ("p", "m", "v", "g", "packed", "p2", "packed2")}
    before = {k: _bits(b.t) for k, b in bufs.items()}

    def seg(packed, chunk0, **kw):
        s = _lib.AdamSegment()
        s.param, s.exp_avg, s.exp_avg_sq, s.grad, s.packed = bufs["p"].ptr, bufs["m"].ptr, bufs["v"].ptr, bufs["g"].ptr, packed
        s.n, s.cols, s.pitch, s.packed_kind, s.chunk0 = n, 1, 1, _lib.ADAM_PACK_F32, chunk0
        s.step_size, s.bc2_sqrt = bias_corrections(1, LR, *BETAS)
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    stream = torch.cuda.current_stream(dev()).cuda_stream
    norm, partials = torch.zeros(1, device=dev()), torch.zeros(4, dtype=torch.float64, device=dev())
    cases = [([seg(bufs["packed"].ptr, 1)], 0.0, -1), ([seg(bufs["packed"].ptr, 0), seg(bufs["packed"].ptr + 4 * 100, 1, param=bufs["p2"].ptr)], 0.0, -1),
             ([seg(bufs["packed"].ptr, 0, n=0)], 0.0, -2), ([seg(bufs["packed"].ptr, 0, cols=7)], 0.0, -2),
             ([seg(bufs["packed"].ptr, 0)], 1.0, -1)]
    for segs, max_norm, want in cases:
        host = (_lib.AdamSegment * len(segs))(*segs)
        table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev())
        rc = L.mhmr_adam_step(host, table.data_ptr(), len(segs), 0.9, 0.999, 1e-8, max_norm, partials.data_ptr() if max_norm else None, 0,
                              norm.data_ptr(), stream)
        assert rc == want, (rc, want)
    torch.cuda.synchronize()
    assert all(np.array_equal(_bits(b.t), before[k]) for k, b in bufs.items())


# ------------------------------------------------------------------------------------------------------ the model
NAME, S, GRID = "dinov2_vits14", 224, 16


@functools.lru_cache(maxsize=None)
def _assets():
    import synthetic
    data, mean = synthetic.make_smplx_data(seed=0), synthetic.make_mean_params(seed=0)
    sd = synthetic.make_state_dict(NAME, S, seed=42, depth_override=4, mean_params=mean)
    return dict(data=data, mean=mean, sd=sd)


def _new_model(precision="f16", sd=None):
    """The fixture of tests/test_gpu_hph_backward.py: ViT-S, 224^2, backbone depth 4, synthetic weights."""
    from multi_hmr_amd import Model
    a = _assets()
    m = Model(backbone=NAME, img_size=S, smplx_data=a["data"], mean_params=a["mean"], backbone_depth=4, precision=precision)
    m.load_state_dict(a["sd"] if sd is None else sd, strict=True)
    return m.to(dev()).eval()


def _scene(persons, seed):
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


def _backward(m, x, K, idx, seed, detection=True, heads=True):
    """One forward + backward with fixed random cotangents of readout, offset and scores (the loss is not what is tested here)."""
    out = m(x, idx=idx, K=K, is_training=True, return_readout=True, train_heads=heads, train_detection=detection)
    g = torch.Generator().manual_seed(seed)
    total = 0.0
    for k in ("readout", "offset", "scores"):
        if k in out and out[k].requires_grad:            # (no person: no "offset" key, an empty read-out whose backward gives zeros)
            total = total + (out[k] * torch.randn(out[k].shape, generator=g).to(dev())).sum()
    total.backward()
    return out


def _packed_bits(m):
    P = m._packed
    tensors = [P["hph_t"][n] for n in m.HEAD_TENSORS] + [t for layer in P["hph_t"]["layers"] for t in layer.values()]
    tensors += [P[n] for n in ("cls0_w", "cls0_b", "cls2_w", "cls2_b")]
    return [_bits(t) for t in tensors]


def _trainable(m):
    return m.heads_parameters() + m.detection_parameters()


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_step_leaves_exactly_what_repack_heads_would(precision):
    """The contract: after HeadsAdam.step() every packed head tensor and the four detector tensors already hold what repack_heads() makes
    of the updated parameters -- and the next forward is, bit for bit, that of a second model loaded from the first one's state_dict()."""
    m = _new_model(precision).train_heads_(True).train_detection_(True)
    x, K, idx = _scene((2, 1), 1)
    opt = HeadsAdam(m, lr=1e-3, max_grad_norm=1e9)
    before = _packed_bits(m) if m._packed is not None else None
    for step in range(2):
        opt.zero_grad(set_to_none=True)
        _backward(m, x, K, idx, 10 + step)
        gen = m._packed["heads_generation"]
        if step == 0:
            before = _packed_bits(m)
        opt.step()
        assert m._packed["heads_generation"] == gen + 1
        after = _packed_bits(m)
        m.repack_heads()
        repacked = _packed_bits(m)
        assert len(after) == len(repacked) == 13 + 17 * m.xat_depth + 4
        for i, (a, b) in enumerate(zip(after, repacked)):
            assert np.array_equal(a, b), (step, i)
    assert sum(int((a != b).sum()) for a, b in zip(before, after)) > 100000      # the step did move the packed weights
    assert float(opt.last_grad_norm) > 0
    out = m(x, idx=idx, K=K, is_training=True, return_readout=True)
    twin = _new_model(precision, sd=m.state_dict())
    ref = twin(x, idx=idx, K=K, is_training=True, return_readout=True)
    assert list(out) == list(ref)
    for k in out:
        assert torch.equal(out[k], ref[k]), k


def test_three_steps_against_torch_adam_and_repack_heads():
    """Twin models, the same cotangents: HeadsAdam against torch.optim.Adam + repack_heads() for three steps.  Per parameter, the 4x rule:
    each side's one-step error against the fp64 oracle from the state the step started from."""
    ma, mb = (_new_model().train_heads_(True).train_detection_(True) for _ in range(2))
    x, K, idx = _scene((2, 1), 1)
    oa = HeadsAdam(ma, lr=LR, betas=BETAS, eps=EPS)
    ob = torch.optim.Adam(_trainable(mb), lr=LR, betas=BETAS, eps=EPS, foreach=False)
    names = oa._names
    worst = []
    for step in range(3):
        rows = {}
        for tag, m, opt in (("ours", ma, oa), ("torch", mb, ob)):
            opt.zero_grad(set_to_none=True)
            _backward(m, x, K, idx, 20 + step)
            start = []
            for p in _trainable(m):
                st = opt.state.get(p, {})
                z = lambda: torch.zeros_like(p)
                start.append(dict(p=p.detach().cpu().numpy().copy(), m=st.get("exp_avg", z()).cpu().numpy().copy(),
                                  v=st.get("exp_avg_sq", z()).cpu().numpy().copy(), step=int(st.get("step", 0))))
            grads = [p.grad.detach().cpu().numpy().copy() for p in _trainable(m)]
            ref, _ = oo.adam_step(start, grads, LR, BETAS, EPS)
            opt.step()
            if tag == "torch":
                m.repack_heads()
            rows[tag] = [max(float(np.max(np.abs(p.detach().cpu().double().numpy() - r["p"]))),
                             float(np.max(np.abs(opt.state[p]["exp_avg"].cpu().double().numpy() - r["m"]))),
                             float(np.max(np.abs(opt.state[p]["exp_avg_sq"].cpu().double().numpy() - r["v"]))))
                         for p, r in zip(_trainable(m), ref)]
            assert all(int(opt.state[p]["step"]) == step + 1 for p in _trainable(m))
        for n, e_us, e_t in zip(names, rows["ours"], rows["torch"]):
            assert e_us <= 4.0 * e_t, (step, n, e_us, e_t)
        i = int(np.argmax([a / max(b, 1e-300) for a, b in zip(rows["ours"], rows["torch"])]))
        worst.append(dict(step=step + 1, parameter=names[i], ours=rows["ours"][i], torch=rows["torch"][i]))
        # The twins track each other.  No tight bound exists: where a gradient element is rounding noise, g / sqrt(g^2) amplifies a last-bit
        # difference to a whole update.  An update of step t is at most lr sqrt(t) (|m^| <= max |g|, v^ >= max g^2 / t up to beta2^t), so the
        # twins are never further apart than twice the sum of that over the steps so far.
        bound = 2.0 * LR * sum(t ** 0.5 for t in range(1, step + 2))
        for pa, pb in zip(_trainable(ma), _trainable(mb)):
            assert float((pa.detach() - pb.detach()).abs().max()) <= bound
    report("HeadsAdam vs torch.optim.Adam (fp32, same device), worst ratio per step: max abs error of p / m / v vs fp64", worst)


def test_detector_untouched_without_train_detection():
    m = _new_model().train_heads_(True)
    x, K, idx = _scene((2, 1), 2)
    opt = HeadsAdam(m, lr=1e-3)
    _backward(m, x, K, idx, 30, detection=False)
    det = [p.detach().clone() for p in m.detection_parameters()]
    packed = [_bits(m._packed[n]) for n in ("cls0_w", "cls0_b", "cls2_w", "cls2_b")]
    heads = [p.detach().clone() for p in m.heads_parameters()]
    opt.step()
    for p, q in zip(m.detection_parameters(), det):
        assert np.array_equal(_bits(p), _bits(q)) and p not in opt.state                       # no moments, no step count
    assert all(np.array_equal(_bits(m._packed[n]), b) for n, b in zip(("cls0_w", "cls0_b", "cls2_w", "cls2_b"), packed))
    assert sum(int(not torch.equal(p, q)) for p, q in zip(m.heads_parameters(), heads)) >= len(heads) // 2
    assert all(int(opt.state[p]["step"]) == 1 for p in m.heads_parameters())


def test_only_the_detector_moves_without_persons():
    """No person: the heads' gradients are zeros (the empty read-out is part of the graph), so their step leaves parameters and packed
    copies with the same bits; the detector's are not (every cell is a negative)."""
    m = _new_model().train_heads_(True).train_detection_(True)
    x, K, idx = _scene((0, 0), 3)
    opt = HeadsAdam(m, lr=1e-3)
    _backward(m, x, K, idx, 31)
    heads = [p.detach().clone() for p in m.heads_parameters()]
    det = [p.detach().clone() for p in m.detection_parameters()]
    head_bits = _packed_bits(m)[:-4]
    opt.step()
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(m.heads_parameters(), heads))
    assert all(np.array_equal(a, b) for a, b in zip(_packed_bits(m)[:-4], head_bits))
    assert all(not torch.equal(p, q) for p, q in zip(m.detection_parameters(), det))
    after = _packed_bits(m)
    m.repack_heads()
    assert all(np.array_equal(a, b) for a, b in zip(after, _packed_bits(m)))


def test_backward_after_step_raises_the_generation_error():
    m = _new_model().train_heads_(True).train_detection_(True)
    x, K, idx = _scene((2, 1), 4)
    opt = HeadsAdam(m, lr=1e-4)
    _backward(m, x, K, idx, 32)
    out = m(x, idx=idx, K=K, is_training=True, return_readout=True, train_heads=True, train_detection=True)
    opt.step()
    with pytest.raises(_lib.MhmrError, match="backward must run before the next forward of the same batch size and before repack_heads"):
        (out["readout"].sum() + out["scores"].sum()).backward()


def test_parameters_only_before_the_first_forward_and_refusals():
    m = _new_model().train_heads_(True).train_detection_(True)
    assert m._packed is None
    opt = HeadsAdam(m, lr=1e-3)
    g = torch.Generator().manual_seed(1)
    old = [p.detach().clone() for p in _trainable(m)]
    for p in _trainable(m):
        p.grad = torch.randn(p.shape, generator=g).to(dev())
    opt.step()
    assert m._packed is None and all(not torch.equal(p, q) for p, q in zip(_trainable(m), old))
    x, K, idx = _scene((2, 1), 5)
    ref = _new_model(sd=m.state_dict())(x, idx=idx, K=K, is_training=True)
    out = m(x, idx=idx, K=K, is_training=True)                                  # packs the updated parameters
    assert all(torch.equal(out[k], ref[k]) for k in out)
    opt.step()                                                                  # the table is rebuilt for the new pack
    after = _packed_bits(m)
    m.repack_heads()
    assert all(np.array_equal(a, b) for a, b in zip(after, _packed_bits(m)))
    p = m.heads_parameters()[0]
    p.data = p.data.t().contiguous().t()
    with pytest.raises(_lib.MhmrError, match="contiguous fp32"):
        opt.step()


def test_state_dict_round_trip_through_torch_adam():
    """Two steps; the state through torch.optim.Adam's state_dict and back into a fresh HeadsAdam on a twin; the third step has the
    bits of the uninterrupted run."""
    x, K, idx = _scene((2, 1), 6)
    ma = _new_model().train_heads_(True).train_detection_(True)
    oa = HeadsAdam(ma, lr=LR)
    for step in range(2):
        oa.zero_grad(set_to_none=True)
        _backward(ma, x, K, idx, 40 + step)
        oa.step()
    mb = _new_model(sd=ma.state_dict()).train_heads_(True).train_detection_(True)
    via = torch.optim.Adam(_trainable(mb), lr=LR)
    via.load_state_dict(copy.deepcopy(oa.state_dict()))            # (a copy, as a saved file would be: load_state_dict keeps the tensors it is given)
    ob = HeadsAdam(mb, lr=LR)
    ob.load_state_dict(via.state_dict())
    for m, opt in ((ma, oa), (mb, ob)):
        opt.zero_grad(set_to_none=True)
        _backward(m, x, K, idx, 42)
        opt.step()
    for pa, pb in zip(_trainable(ma), _trainable(mb)):
        assert torch.equal(pa, pb) and float(oa.state[pa]["step"]) == float(ob.state[pb]["step"]) == 3.0
        assert torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])
    assert all(np.array_equal(a, b) for a, b in zip(_packed_bits(ma), _packed_bits(mb)))
