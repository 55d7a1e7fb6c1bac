"""TEST INFRASTRUCTURE: the discrete half of detection -- NMS, threshold, ordered compaction, the decoder's group and work-item tables --
stated once in plain numpy / Python, and a named, seeded set of score maps at which the kernels of csrc/hph.hip can go wrong
(detect_count_kernel, detect_write_kernel, person_groups_kernel).  No GPU here: tests/test_detection_host.py holds this statement to the
reference's own (oracle.multihmr_ref.nms + torch.where, model.py:612-638) and asserts what makes each case mean something;
tests/test_gpu_detection.py holds the kernels to it.  Everything is integer-exact or bit-exact: no tolerance anywhere.

detect_write_kernel gives thread t of 256 the cells [t * per, t * per + per) of an image, per = ceil(G * G / 256): ``per_thread`` /
``thread_of`` say which cells share a thread, so that cases can sit on the seams."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

GRIDS = (1, 2, 15, 16, 17, 37, 48, 64, 92)          # 48 / 64 / 92: 672^2, 896^2 (the benchmark) and 1288^2 at patch 14
WINDOWS = (1, 2, 3, 4, 5, 7)
THREADS = 256                                        # detect_write_kernel's workgroup


def nms_pad(k: int) -> int:
    """model.py:620-638: the max-pool's padding; its output is cropped top-left where it is larger than the map (k = 2 and 4)."""
    return 1 if k == 2 else 2 if k == 4 else (k - 1) // 2


def nms_oracle(scores: np.ndarray, k: int) -> np.ndarray:
    """scores [B, G, G] float32 -> the map after NMS: a cell that equals the maximum of the window (y - pad .. y - pad + k - 1) x
    (x - pad .. x - pad + k - 1), clipped to the image, keeps its own value; every other cell becomes 0."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    B, G, _ = scores.shape
    pad = nms_pad(k)
    hmax = np.full_like(scores, -np.inf)
    for dy in range(k):
        for dx in range(k):
            oy, ox = dy - pad, dx - pad                                  # cell (y, x) sees (y + oy, x + ox) where that is inside the image
            y0, y1, x0, x1 = max(0, -oy), min(G, G - oy), max(0, -ox), min(G, G - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            view = hmax[:, y0:y1, x0:x1]
            np.maximum(view, scores[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox], out=view)
    return np.where(hmax == scores, scores, np.float32(0.0)).astype(np.float32)


def detect_oracle(scores: np.ndarray, k: int, thr: float):
    """-> (det_b, det_y, det_x, det_score, counts): the cells whose score after NMS is >= float32(thr), in (b, y, x) ascending order."""
    kept = nms_oracle(scores, k)
    B, G, _ = kept.shape
    sel = np.flatnonzero(kept.reshape(-1) >= np.float32(thr))            # ascending flat index == (b, y, x) ascending
    det_b, n = sel // (G * G), sel % (G * G)
    return det_b, n // G, n % G, kept.reshape(-1)[sel], np.bincount(det_b, minlength=B)


def groups_oracle(counts, cap: int):
    """The reference's host bookkeeping after torch.where (model.py:146-151; rebatch / pad_to_max, utils/tensor_manip.py:7-45) for per-image
    person counts of which only the first ``cap`` persons are kept -> (base, gstart, chunks, info), all plain lists WITHOUT padding:
    base[b] exclusive prefix of the counts; gstart the person offsets of the non-empty images, [0, ..., kept]; chunks the flat
    (image, first person, count <= 8) triples; info = [persons kept, groups, chunks, total]."""
    counts = [int(c) for c in counts]
    kept, left = [], cap
    for c in counts:
        kept.append(min(c, max(left, 0)))
        left -= kept[-1]
    gstart, chunks, start = [0], [], 0
    for b, c in enumerate(kept):
        if c == 0:
            continue
        for q0 in range(0, c, 8):
            chunks += [b, start + q0, min(8, c - q0)]
        start += c
        gstart.append(start)
    base = [sum(counts[:b]) for b in range(len(counts))]
    return base, gstart, chunks, [start, len(gstart) - 1, len(chunks) // 3, sum(counts)]


def per_thread(G: int) -> int:
    return (G * G + THREADS - 1) // THREADS


def thread_of(G: int, y, x):
    return (np.asarray(y) * G + np.asarray(x)) // per_thread(G)


def cap_set(base, total: int):
    """The capacities of the fixed-capacity tests: none, one, the cut at the first image's end and one inside the second image, one short
    of everything, everything, and room to spare."""
    b1 = base[1] if len(base) > 1 else total
    return sorted({c for c in (0, 1, b1, b1 + 1, total - 1, total, total + 5) if c >= 0})


# ------------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    name: str
    pattern: str
    G: int
    k: int
    thr: float
    scores: np.ndarray                      # [B, G, G] float32
    meta: dict = field(default_factory=dict)

    @property
    def B(self) -> int:
        return self.scores.shape[0]

    @functools.cached_property
    def oracle(self):
        return detect_oracle(self.scores, self.k, self.thr)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _low(rng, B, G):
    """A background nobody detects and no placed cell loses to: uniform in [0, 0.2)."""
    return (rng.random((B, G, G), dtype=np.float32) * np.float32(0.2)).astype(np.float32)


#: seeds of the ``random`` cases at G >= 37, chosen so that a detection falls into the last non-empty thread's run and some run holds
#: two (tests/test_detection_host.py asserts both); every other case takes seed 0
RANDOM_SEEDS = {(37, 3): 7, (37, 4): 4, (48, 4): 1}


def _random(G, k, B=3, seed=0):
    s = _rng("random", G, k, B, seed).random((B, G, G), dtype=np.float32)
    if B > 2:
        s[2] *= np.float32(0.1)                                          # an image without detections
    return Case(f"random-G{G}-k{k}" + (f"-B{B}" if B != 3 else ""), "random", G, k, 0.8, s)


def _plateau(G, k):
    s = _rng("plateau", G, k).random((3, G, G), dtype=np.float32)
    s[0] = np.float32(0.9)                                               # every cell equals every window's maximum: G * G persons
    s[2] = np.float32(0.1)
    return Case(f"plateau-G{G}-k{k}", "plateau", G, k, 0.8, s)


def _thr_zero(G, k):
    return Case(f"thr_zero-G{G}-k{k}", "thr_zero", G, k, 0.0, _rng("thr_zero", G, k).random((3, G, G), dtype=np.float32))


def _neighbours(G, y, x):
    return [(y + dy, x + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy or dx) and 0 <= y + dy < G and 0 <= x + dx < G]


def _borders(G, k):
    rng = _rng("borders", G, k)
    s = _low(rng, 3, G)
    m = G // 2
    spots = [(0, 0), (0, G - 1), (G - 1, 0), (G - 1, G - 1), (0, m), (G - 1, m), (m, 0), (m, G - 1)]
    below = np.float32(0.95)                                             # the neighbours: above the threshold, a step from winning
    peaks = below + np.arange(1, 9, dtype=np.float32) * np.spacing(below)                 # the next eight float32 values, all distinct
    for b in range(3):
        for (y, x), v in zip(spots, rng.permutation(peaks)):
            for yy, xx in _neighbours(G, y, x):
                s[b, yy, xx] = below
            s[b, y, x] = v
    return Case(f"borders-G{G}-k{k}", "borders", G, k, 0.8, s, dict(spots=spots))


def one_sided_offsets(k):
    pad = nms_pad(k)
    offs = [(pad, 0), (-pad, 0), (0, pad), (0, -pad), (pad - 1, 0), (-(pad - 1), 0), (0, pad - 1), (0, -(pad - 1))]
    return [o for o in offs if o != (0, 0)]


def _one_sided(G, k):
    """Image i: the cell c = (G // 2, G // 2) at 0.85 and ONE larger neighbour (0.95) at the i-th offset.  The window of an even k
    reaches pad cells up / left and pad - 1 down / right, so an offset and its mirror give different answers."""
    offs = one_sided_offsets(k)
    s = _low(_rng("one_sided", G, k), len(offs), G)
    c = G // 2
    for b, (oy, ox) in enumerate(offs):
        s[b, c, c] = np.float32(0.85)
        s[b, c + oy, c + ox] = np.float32(0.95)
    return Case(f"one_sided-G{G}-k{k}", "one_sided", G, k, 0.8, s, dict(cell=(c, c), offsets=offs))


def _ties(G, k):
    """Image 0: a 2 x 2 block of equal values (each is the maximum of every window it is in).  Images 1 / 2: two equal cells at Chebyshev
    distance pad (inside each other's window, or at least inside one) and pad + 1 (outside)."""
    s = _low(_rng("ties", G, k), 3, G)
    c, pad = G // 2 - 2, max(nms_pad(k), 1)
    s[0, c:c + 2, c:c + 2] = np.float32(0.9)
    for b, d in ((1, pad), (2, pad + 1)):
        s[b, c, c] = s[b, c + d, c + d] = np.float32(0.9)
    return Case(f"ties-G{G}-k{k}", "ties", G, k, 0.8, s, dict(block=(c, c), dist=(pad, pad + 1)))


def _at_threshold(G, k, thr):
    """Three isolated cells (8 apart, the widest window is 7) hold float32(thr) and its two float32 neighbours; each image a rotation."""
    s = (_low(_rng("at_threshold", G, k, thr), 3, G) * np.float32(0.5)).astype(np.float32)
    t = np.float32(thr)
    vals = [t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))]
    spots = [(1, 1), (1, 9), (9, 1)]
    for b in range(3):
        for i, (y, x) in enumerate(spots):
            s[b, y, x] = vals[(i + b) % 3]
    return Case(f"at_threshold-G{G}-k{k}-thr{thr}", "at_threshold", G, k, thr, s, dict(spots=spots, values=vals))


def run_edge_placements(G):
    """Flat cell indices on the seams of detect_write_kernel's runs: the first and the last cell of the image, and for several threads
    t the last cell of thread t - 1 and the first of t (the last non-empty thread among them)."""
    N, per = G * G, per_thread(G)
    last = (N - 1) // per
    ns = [0, N - 1]
    for t in (1, 2, 63, 64, 65, 128, 200, last):
        if t * per < N:
            ns += [t * per - 1, t * per]
    return sorted(set(ns))


def _run_edges(G, k, i, ns):
    """One cell above the threshold per image, at flat index ns[b]."""
    s = _low(_rng("run_edges", G, k, i), 3, G)
    for b, n in enumerate(ns):
        s[b, n // G, n % G] = np.float32(0.9)
    return Case(f"run_edges-G{G}-k{k}-{i}", "run_edges", G, k, 0.8, s, dict(n=list(ns)))


def _build():
    cases = []
    for G in GRIDS:
        for k in (1, 3, 4):
            cases.append(_random(G, k, seed=RANDOM_SEEDS.get((G, k), 0)))
            cases.append(_plateau(G, k))
    for G in (2, 17, 64, 92):
        for k in (1, 3, 4):
            cases.append(_thr_zero(G, k))
    for G in (17, 37, 64, 92):
        ns = run_edge_placements(G)
        ns += ns[:(-len(ns)) % 3]                                         # whole cases of three images
        for i in range(0, len(ns), 3):
            cases.append(_run_edges(G, 3, i // 3, ns[i:i + 3]))
    for G in (15, 64):
        for k in WINDOWS:
            cases += [_borders(G, k), _ties(G, k), _at_threshold(G, k, 0.3), _at_threshold(G, k, 0.8)]
            if k in (2, 4):
                cases.append(_one_sided(G, k))
    for B in (1, 33):
        for k in (3, 4):
            cases.append(_random(16, k, B=B))
    return {c.name: c for c in cases}


CASES = _build()
NAMES = tuple(CASES)
#: the cases of the fixed-capacity tests: many persons, the cut inside an image, grids with more than one cell per thread
CAP_NAMES = tuple(n for n, c in CASES.items() if c.pattern in ("random", "plateau") and c.G in (17, 64, 92))


def threshold_between(survivors: np.ndarray, target: int):
    """A threshold that about ``target`` of the scores ``survivors`` (the non-zero cells after NMS) pass and that no score is near: the
    midpoint of two adjacent distinct scores that are more than two float32 steps apart, searched downwards from the target-th largest
    -> (thr as a Python float that float32 holds exactly, the number of scores >= thr)."""
    d = np.unique(np.asarray(survivors, dtype=np.float32))[::-1]
    passing = len(survivors) - np.searchsorted(np.sort(survivors), d, side="left")        # passing[i] = number of scores >= d[i]
    for i in range(int(np.argmax(passing >= target)), len(d) - 1):
        hi, lo = d[i], d[i + 1]
        mid = np.float32((float(hi) + float(lo)) / 2)
        if np.nextafter(lo, np.float32(np.inf)) < mid < np.nextafter(hi, np.float32(-np.inf)):
            return float(mid), int(passing[i])
    raise ValueError("no two adjacent scores far enough apart")
