"""No GPU: the loop oracle of tests/detect_cases.py against the reference's own statement of NMS + threshold (oracle.multihmr_ref.nms, the
max-pool form of model.py:620-638, + torch.where, model.py:612-617, 146-149) on every case, and the conditions that make each case mean
something, asserted from the oracle alone.  tests/test_gpu_detection.py runs the kernels on the same cases."""
import numpy as np
import pytest
import torch

import detect_cases as dc
from oracle.multihmr_ref import nms


@pytest.mark.parametrize("name", dc.NAMES)
def test_loop_oracle_equals_the_max_pool_statement(name):
    c = dc.CASES[name]
    heat = nms(torch.from_numpy(c.scores).view(c.B, 1, c.G, c.G), c.k)
    assert np.array_equal(heat.view(c.B, c.G, c.G).numpy().view(np.int32), dc.nms_oracle(c.scores, c.k).view(np.int32))
    idx = torch.where(heat.permute(0, 2, 3, 1) >= c.thr)
    det_b, det_y, det_x, det_score, counts = c.oracle
    assert [det_b.tolist(), det_y.tolist(), det_x.tolist()] == [idx[0].tolist(), idx[1].tolist(), idx[2].tolist()]
    assert np.array_equal(det_score.view(np.int32), heat[idx[0], idx[3], idx[1], idx[2]].numpy().view(np.int32))
    assert counts.tolist() == torch.bincount(idx[0], minlength=c.B).tolist()
    assert det_score.dtype == np.float32 and c.scores.dtype == np.float32 and c.scores.shape == (c.B, c.G, c.G)


def test_the_case_table_is_the_one_the_issue_asks_for():
    by = {}
    for c in dc.CASES.values():
        by.setdefault(c.pattern, set()).add((c.G, c.k))
    full = {(G, k) for G in dc.GRIDS for k in (1, 3, 4)}
    assert by["random"] >= full and by["plateau"] == full
    assert {G for G, k in by["run_edges"]} == {17, 37, 64, 92} and {k for G, k in by["run_edges"]} == {3}
    window = {(G, k) for G in (15, 64) for k in dc.WINDOWS}
    assert by["borders"] == by["ties"] == by["at_threshold"] == window
    assert by["one_sided"] == {(G, k) for G in (15, 64) for k in (2, 4)}
    assert {dc.CASES[n].B for n in dc.NAMES if n.startswith("random-G16-") and "-B" in n} == {1, 33}
    assert {c.thr for c in dc.CASES.values() if c.pattern == "at_threshold"} == {0.3, 0.8}
    assert [dc.per_thread(G) for G in (16, 17, 37, 48, 64, 92)] == [1, 2, 6, 9, 16, 34]


@pytest.mark.parametrize("name", [n for n in dc.NAMES if dc.CASES[n].pattern in ("random", "plateau")])
def test_random_and_plateau_hold_what_they_are_for(name):
    c = dc.CASES[name]
    det_b, det_y, det_x, _, counts = c.oracle
    if c.pattern == "plateau":
        assert counts[0] == c.G * c.G and counts[2] == 0
        return
    if c.B > 2:
        assert counts[2] == 0
    if c.G >= 37:
        t = dc.thread_of(c.G, det_y, det_x)
        assert (t == (c.G * c.G - 1) // dc.per_thread(c.G)).any(), "no detection in the last non-empty thread's run"
        assert np.unique(det_b * dc.THREADS + t, return_counts=True)[1].max() >= 2, "no run with two detections"
    if c.G >= 15:
        assert counts[0] > 0 and counts[1 % c.B] > 0


@pytest.mark.parametrize("name", [n for n in dc.NAMES if dc.CASES[n].pattern == "thr_zero"])
def test_thr_zero_returns_every_cell_and_zeros_for_the_suppressed(name):
    c = dc.CASES[name]
    _, _, _, det_score, counts = c.oracle
    assert counts.tolist() == [c.G * c.G] * c.B
    zeros = det_score.view(np.int32) == 0                               # +0.0, bit for bit
    assert np.array_equal(zeros, det_score == 0)
    if c.k > 1 and c.G > 1:
        assert zeros.any() and not zeros.all()
    else:
        assert not zeros.any()


@pytest.mark.parametrize("name", [n for n in dc.NAMES if dc.CASES[n].pattern == "run_edges"])
def test_run_edges_detect_one_cell_per_image_where_intended(name):
    c = dc.CASES[name]
    det_b, det_y, det_x, _, counts = c.oracle
    assert counts.tolist() == [1, 1, 1]
    assert (det_y * c.G + det_x).tolist() == c.meta["n"]


def test_run_edges_cover_both_sides_of_the_seams():
    for G in (17, 37, 64, 92):
        N, per = G * G, dc.per_thread(G)
        ns = {n for c in dc.CASES.values() if c.pattern == "run_edges" and c.G == G for n in c.meta["n"]}
        last = (N - 1) // per
        assert {0, N - 1, per - 1, per, last * per - 1, last * per} <= ns
        assert sum(1 for t in range(1, last + 1) if t * per - 1 in ns and t * per in ns) >= 4
    assert dc.per_thread(92) * ((92 * 92 - 1) // dc.per_thread(92) + 1) > 92 * 92          # G = 92: a short last run
    assert (17 * 17 - 1) // dc.per_thread(17) == 144                                          # G = 17: threads >= 145 idle


@pytest.mark.parametrize("name", [n for n in dc.NAMES if dc.CASES[n].pattern == "one_sided"])
def test_one_sided_windows_show_their_asymmetry(name):
    c = dc.CASES[name]
    det_b, det_y, det_x, _, _ = c.oracle
    cy, cx = c.meta["cell"]
    offs = c.meta["offsets"]
    assert len(offs) == (4 if c.k == 2 else 8) == c.B
    survives = {o: bool(((det_b == b) & (det_y == cy) & (det_x == cx)).any()) for b, o in enumerate(offs)}
    for b, (oy, ox) in enumerate(offs):                                 # the larger neighbour itself is always a detection
        assert ((det_b == b) & (det_y == cy + oy) & (det_x == cx + ox)).any()
    assert any(not survives[o] and survives[(-o[0], -o[1])] for o in offs), survives
    pad = dc.nms_pad(c.k)                                               # and exactly: up / left reach pad, down / right pad - 1
    assert survives == {o: not (-pad <= o[0] <= c.k - 1 - pad and -pad <= o[1] <= c.k - 1 - pad) for o in offs}


@pytest.mark.parametrize("name", [n for n in dc.NAMES if dc.CASES[n].pattern == "ties"])
def test_ties_all_survive(name):
    c = dc.CASES[name]
    det_b, det_y, det_x, det_score, counts = c.oracle
    assert counts.tolist() == [4, 2, 2] and (det_score == np.float32(0.9)).all()
    y, x = c.meta["block"]
    assert sorted(zip(det_y[det_b == 0].tolist(), det_x[det_b == 0].tolist())) == [(y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)]
    for b, d in zip((1, 2), c.meta["dist"]):
        assert list(zip(det_y[det_b == b].tolist(), det_x[det_b == b].tolist())) == [(y, x), (y + d, x + d)]


@pytest.mark.parametrize("name", [n for n in dc.NAMES if dc.CASES[n].pattern == "at_threshold"])
def test_at_threshold_two_of_three_pass(name):
    c = dc.CASES[name]
    det_b, det_y, det_x, det_score, counts = c.oracle
    t = np.float32(c.thr)
    below, above = np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))
    assert below < t < above and c.meta["values"] == [t, below, above]
    assert counts.tolist() == [2, 2, 2]
    for b in range(3):
        assert sorted(det_score[det_b == b].tolist()) == [float(t), float(above)]
        got = set(zip(det_y[det_b == b].tolist(), det_x[det_b == b].tolist()))
        assert got == {s for i, s in enumerate(c.meta["spots"]) if c.meta["values"][(i + b) % 3] >= t}


@pytest.mark.parametrize("name", [n for n in dc.NAMES if dc.CASES[n].pattern == "borders"])
def test_borders_keep_the_eight_peaks(name):
    """The eight peaks are the eight largest values, so every window keeps them; which of their neighbours (one step below, above the
    threshold) survive is the clipped, anchored window's business: all of them at k = 1, none at odd k >= 3, at k = 2 those the window
    does not reach back from."""
    c = dc.CASES[name]
    det_b, det_y, det_x, det_score, counts = c.oracle
    top = np.sort(c.scores.reshape(c.B, -1), axis=1)[:, -8:]
    for b in range(c.B):
        got = set(zip(det_y[det_b == b].tolist(), det_x[det_b == b].tolist()))
        assert set(c.meta["spots"]) <= got
        assert sorted(c.scores[b, y, x] for y, x in c.meta["spots"]) == top[b].tolist() and len(set(top[b].tolist())) == 8
        extra = len(got) - 8
        if c.k == 2:
            assert 0 < extra < 4 * 3 + 4 * 5
        else:
            assert extra == (4 * 3 + 4 * 5 if c.k == 1 else 0)


def test_groups_oracle_on_a_hand_checked_example():
    base, gstart, chunks, info = dc.groups_oracle([3, 0, 11, 1], 20)
    assert (base, gstart, info) == ([0, 3, 3, 14], [0, 3, 14, 15], [15, 3, 4, 15])
    assert chunks == [0, 0, 3, 2, 3, 8, 2, 11, 3, 3, 14, 1]
    assert dc.groups_oracle([3, 0, 11, 1], 5) == ([0, 3, 3, 14], [0, 3, 5], [0, 0, 3, 2, 3, 2], [5, 2, 2, 15])
    assert dc.groups_oracle([0, 0], 4) == ([0, 0], [0], [], [0, 0, 0, 0])
    assert dc.cap_set([0, 7, 9], 9) == [0, 1, 7, 8, 9, 14]
