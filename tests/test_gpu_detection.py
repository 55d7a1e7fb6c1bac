"""-m gpu: the discrete half of inference -- NMS, threshold, ordered compaction into person rows, the decoder's group and work-item tables
(detect_count_kernel, detect_write_kernel, person_groups_kernel of csrc/hph.hip; Model._detect_and_heads) -- against the plain oracle of
tests/detect_cases.py at the workload's grid sizes.  A fault here is no rounding error: a person is dropped, duplicated, written to the
wrong image or put in the wrong order.  Everything is integer-exact or bit-exact; there is no tolerance in this file.  What each case is
for, and that it is what it claims to be, is asserted without a GPU in tests/test_detection_host.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import detect_cases as dc  # noqa: E402
import make_golden  # noqa: E402
from multi_hmr_amd import Model, _lib  # noqa: E402

SLACK, SENT = 16, -7                  # rows behind the last one a kernel may write, and what they (and every unwritten row) must still hold
BAD_ARG = -1                          # include/mhmr.h MHMR_ERR_BAD_ARG


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev_scores(c):
    return torch.from_numpy(c.scores).cuda().contiguous()


def sentinel_rows(n):
    """det [3, n] int32 full of -7 and det_score [n] float32 full of -7.0."""
    return torch.full((3, n), SENT, dtype=torch.int32, device="cuda"), torch.full((n,), float(SENT), dtype=torch.float32, device="cuda")


def assert_rows(det, dsc, oracle, kept, what):
    """Rows [0, kept) are the oracle's first rows -- coordinates as integers, scores as BITS (a -0.0 or a wrong zero would show) -- and every
    row behind them still holds the sentinel."""
    det_b, det_y, det_x, det_score, _ = oracle
    det, dsc = det.cpu(), dsc.cpu()
    assert det[:, :kept].tolist() == [det_b[:kept].tolist(), det_y[:kept].tolist(), det_x[:kept].tolist()], what
    assert torch.equal(dsc[:kept].view(torch.int32), torch.from_numpy(det_score[:kept].copy()).view(torch.int32)), what
    assert bool((det[:, kept:] == SENT).all()) and bool((dsc[kept:] == float(SENT)).all()), what


def count(L, sc, c):
    counts = torch.full((c.B,), SENT, dtype=torch.int32, device="cuda")
    _lib.check(L.mhmr_detect_count(sc.data_ptr(), c.B, c.G, c.k, c.thr, counts.data_ptr(), stream()), "mhmr_detect_count")
    return counts


# ------------------------------------------------------------------------------------------------------ kernels against the oracle
@pytest.mark.parametrize("name", dc.NAMES)
def test_count_and_ordered_compaction(L, name):
    c = dc.CASES[name]
    sc = dev_scores(c)
    counts = count(L, sc, c)
    ref_counts = c.oracle[4]
    assert counts.tolist() == ref_counts.tolist()
    total = int(ref_counts.sum())
    base = torch.tensor(dc.groups_oracle(ref_counts, total)[0], dtype=torch.int32, device="cuda")       # exclusive prefix of the counts
    det, dsc = sentinel_rows(total + SLACK)
    _lib.check(L.mhmr_detect_write(sc.data_ptr(), c.B, c.G, c.k, c.thr, base.data_ptr(), det[0].data_ptr(), det[1].data_ptr(),
                                   det[2].data_ptr(), dsc.data_ptr(), stream()), "mhmr_detect_write")
    assert_rows(det, dsc, c.oracle, total, name)


@pytest.mark.parametrize("name", dc.CAP_NAMES)
def test_fixed_capacity_keeps_the_first_rows_and_touches_no_other(L, name):
    c = dc.CASES[name]
    sc = dev_scores(c)
    ref_counts = c.oracle[4]
    total = int(ref_counts.sum())
    base_l = dc.groups_oracle(ref_counts, total)[0]
    base = torch.tensor(base_l, dtype=torch.int32, device="cuda")
    caps = dc.cap_set(base_l, total)
    assert len(caps) >= 6 and base_l[1] + 1 < total                      # the cut falls inside image 1 for one of them
    for cap in caps:
        det, dsc = sentinel_rows(max(cap, total) + SLACK)
        _lib.check(L.mhmr_detect_write_cap(sc.data_ptr(), c.B, c.G, c.k, c.thr, base.data_ptr(), det[0].data_ptr(), det[1].data_ptr(),
                                           det[2].data_ptr(), dsc.data_ptr(), cap, stream()), "mhmr_detect_write_cap")
        assert_rows(det, dsc, c.oracle, min(cap, total), (name, cap))


@pytest.mark.parametrize("name", dc.CAP_NAMES)
def test_counts_groups_and_rows_describe_one_person_set(L, name):
    """mhmr_detect_count -> mhmr_person_groups (counts on the device, det_b null) -> mhmr_detect_write_cap, as Model._detect_and_heads
    chains them: the tables equal the host bookkeeping and describe exactly the rows that were written."""
    c = dc.CASES[name]
    sc = dev_scores(c)
    counts = count(L, sc, c)
    ref_counts = c.oracle[4]
    total, B = int(ref_counts.sum()), c.B
    for cap in dc.cap_set(dc.groups_oracle(ref_counts, total)[0], total):
        rbase, rgstart, rchunks, rinfo = dc.groups_oracle(ref_counts, cap)
        ngc, ncc = min(B, cap) + 2, cap // 8 + min(B, cap) + 3          # bounds a little above the sufficient ones
        base, gs, ch, info = (torch.full((n,), SENT, dtype=torch.int32, device="cuda") for n in (B, ngc + 1, 3 * ncc, 4))
        _lib.check(L.mhmr_person_groups(counts.data_ptr(), None, 0, B, cap, base.data_ptr(), gs.data_ptr(), ngc, ch.data_ptr(), ncc,
                                        info.data_ptr(), stream()), "mhmr_person_groups")
        det, dsc = sentinel_rows(max(cap, total) + SLACK)
        _lib.check(L.mhmr_detect_write_cap(sc.data_ptr(), B, c.G, c.k, c.thr, base.data_ptr(), det[0].data_ptr(), det[1].data_ptr(),
                                           det[2].data_ptr(), dsc.data_ptr(), cap, stream()), "mhmr_detect_write_cap")
        kept = min(cap, total)
        assert info.tolist() == rinfo == [kept, rinfo[1], rinfo[2], total], (name, cap)
        assert base.tolist() == rbase
        assert gs.tolist() == rgstart + [kept] * (ngc + 1 - len(rgstart))
        assert ch.tolist() == rchunks + [0] * (3 * ncc - len(rchunks))
        assert_rows(det, dsc, c.oracle, kept, (name, cap))
        det_b, chunks, nxt = det[0].cpu(), ch.tolist(), 0
        for i in range(info[2].item()):
            b, first, n = chunks[3 * i:3 * i + 3]
            assert first == nxt and 1 <= n <= 8, (name, cap, i)          # the work items tile [0, kept) without gap or overlap
            assert det_b[first:first + n].tolist() == [b] * n, (name, cap, i)
            nxt = first + n
        assert nxt == kept


def test_bad_arguments_are_refused_and_nothing_is_written(L):
    c = dc.CASES["random-G17-k3"]
    sc = dev_scores(c)
    total = int(c.oracle[4].sum())
    base = torch.tensor(dc.groups_oracle(c.oracle[4], total)[0], dtype=torch.int32, device="cuda")
    counts = torch.full((c.B,), SENT, dtype=torch.int32, device="cuda")
    det, dsc = sentinel_rows(total + SLACK)
    rows = (det[0].data_ptr(), det[1].data_ptr(), det[2].data_ptr(), dsc.data_ptr())
    for k, B in ((0, c.B), (-1, c.B), (3, 0), (3, -2)):
        assert L.mhmr_detect_count(sc.data_ptr(), B, c.G, k, c.thr, counts.data_ptr(), stream()) == BAD_ARG
        assert L.mhmr_detect_write(sc.data_ptr(), B, c.G, k, c.thr, base.data_ptr(), *rows, stream()) == BAD_ARG
        assert L.mhmr_detect_write_cap(sc.data_ptr(), B, c.G, k, c.thr, base.data_ptr(), *rows, total, stream()) == BAD_ARG
    assert L.mhmr_detect_write_cap(sc.data_ptr(), c.B, c.G, c.k, c.thr, base.data_ptr(), *rows, -1, stream()) == BAD_ARG
    torch.cuda.synchronize()
    assert counts.tolist() == [SENT] * c.B
    assert_rows(det, dsc, c.oracle, 0, "bad arguments")


# ------------------------------------------------------------------------------------------------------ the model against its own score map
def build(cfg, smplx_data, mean_params, sd):
    m = Model(backbone=cfg["backbone"], img_size=cfg["img_size"], smplx_data=smplx_data, mean_params=mean_params,
              backbone_depth=cfg["depth_override"], precision="f16")
    m.load_state_dict(sd, strict=True)
    return m.to("cuda:0").eval()


@pytest.mark.parametrize("size,k", [(672, 3), (896, 3), (1288, 4)])      # G = 48, 64 (the benchmark's grid), 92
def test_inference_person_set_equals_the_oracle_on_the_models_own_score_map(size, k, smplx_data, mean_params):
    """Inference at the workload's grids: whoever the oracle detects on the model's own score map, in the oracle's order, with the
    oracle's scores bit for bit; and each person equal, key by key and bit for bit, to the training-mode forward of a fresh model that is
    handed the oracle's detections as idx (both go through Model._heads).  The thresholds are midpoints between adjacent surviving
    scores; the sequence walks the first call (count first), a capacity with padding rows, an overflow (more persons than the capacity:
    re-run at the exact size), a shrink, nobody, and back."""
    cfg = dict(backbone="dinov2_vits14", img_size=size, depth_override=2, batch=3, persons=None, seed=60 + k)
    sd = make_golden.case_state_dict(cfg)
    x, K, _ = make_golden.case_inputs(cfg)
    xc, Kc, G, B = x.cuda(), K.cuda(), size // 14, 3
    one = tuple(torch.zeros(1, dtype=torch.long, device="cuda") for _ in range(4))
    smap = build(cfg, smplx_data, mean_params, sd)(xc, idx=one, K=Kc, is_training=True)["scores"]
    assert smap.shape == (B, G, G, 1) and smap.dtype == torch.float32
    smap = smap.view(B, G, G).cpu().numpy()
    after = dc.nms_oracle(smap, k)
    thr_a, n_a = dc.threshold_between(after[after > 0], 40)
    thr_b, n_b = dc.threshold_between(after[after > 0], 200)
    thr_none = 1.0
    cap_a = -(-max(n_a + max(n_a // 8, 8), 16) // 16) * 16               # Model._forward's next capacity after n_a persons
    print(f"\n[detection {size}^2 k={k}] {int((after > 0).sum())} cells survive NMS; thr_a {thr_a!r} -> {n_a} persons (capacity {cap_a}), "
          f"thr_b {thr_b!r} -> {n_b}")
    assert 40 <= n_a <= 60 and 200 <= n_b <= 260 and n_b > cap_a and float(smap.max()) < thr_none

    ref = {}
    for thr in (thr_a, thr_b):                                           # the expected persons, once per threshold
        det_b, det_y, det_x, det_score, counts = dc.detect_oracle(smap, k, thr)
        assert len(det_b) == {thr_a: n_a, thr_b: n_b}[thr] and (counts > 0).all()
        idx = tuple(torch.from_numpy(a).cuda() for a in (det_b, det_y, det_x, np.zeros_like(det_b)))
        out = build(cfg, smplx_data, mean_params, sd)(xc, idx=idx, K=Kc, is_training=True)
        ref[thr] = (det_b.tolist(), torch.from_numpy(det_score.copy()).view(torch.int32), {n: out[n].clone() for n in Model.PERSON_KEYS if n != "scores"})

    model = build(cfg, smplx_data, mean_params, sd)
    for i, thr in enumerate((thr_a, thr_a, thr_b, thr_a, thr_none, thr_a)):
        persons, ids = model(xc, K=Kc, det_thresh=thr, nms_kernel_size=k, return_image_index=True)
        if thr == thr_none:
            assert persons == [] and ids.numel() == 0
            continue
        det_b, score_bits, out = ref[thr]
        assert len(persons) == len(det_b) and ids.tolist() == det_b, (i, thr, len(persons))
        assert torch.equal(torch.stack([p["scores"] for p in persons]).cpu().view(torch.int32), score_bits), (i, thr)
        for n, want in out.items():
            assert torch.equal(torch.stack([p[n] for p in persons]), want), (i, thr, n)
