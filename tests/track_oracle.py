"""numpy restatement of the tracker's contract (include/mhmr.h mhmr_track_update) at any dtype: a slot table, a sorted-pair
sweep and the One-Euro recursion.  ``OracleTracker(..., dtype=np.float32)`` is the exact yardstick for ids, hits and the table's integers
(every operation is one numpy operation on arrays of that dtype, so each is rounded on its own, as the kernels round it);
``dtype=np.float64`` is the yardstick for the filtered values.  ``table_views`` reads the device table's layout, ``scenes()`` are the
scenes the host and the GPU tests share."""
import math

import numpy as np

GROUPS = ("pose", "shape", "depth", "expr", "loc")
DEFAULT_SMOOTH = dict(pose=(1.0, 0.007), shape=(0.1, 0.0), depth=(1.0, 0.007), expr=(1.0, 0.007), loc=(1.0, 0.007))


def width(nb):
    return 318 + nb + 13


def column_groups(nb):
    """Group index of every state column ``[readout[:318+nb+1] | readout[318+nb+3:] | u | v]``."""
    return np.array([0] * 318 + [1] * nb + [2] + [3] * 10 + [4] * 2)


def state_columns(nb):
    """Read-out column of every state column but the last two."""
    return np.array(list(range(318 + nb + 1)) + list(range(318 + nb + 3, width(nb))))


class OracleTracker:
    def __init__(self, nb, capacity=256, fps=30.0, max_dist=1.0, max_age=30, smooth=DEFAULT_SMOOTH, dcutoff=1.0, dtype=np.float32, predict=True):
        self.nb, self.cap, self.D, self.dt = nb, capacity, width(nb), dtype
        dt = dtype
        self.fps, self.gate, self.max_age, self.predict = np.array(fps, dt), np.array(max_dist, dt) * np.array(max_dist, dt), int(max_age), predict
        self.dcutoff, self.two_pi = np.array(dcutoff, dt), np.array(2.0 * math.pi, dt)
        g = column_groups(nb)
        smooth = smooth or {}
        self.on = np.array([smooth.get(GROUPS[i]) is not None for i in g])
        self.minc = np.array([smooth[GROUPS[i]][0] if smooth.get(GROUPS[i]) is not None else 1.0 for i in g], dt)
        self.beta = np.array([smooth[GROUPS[i]][1] if smooth.get(GROUPS[i]) is not None else 0.0 for i in g], dt)
        self.reset()

    def reset(self):
        c, D, dt = self.cap, self.D, self.dt
        self.next_id = 0
        self.id, self.missed, self.hits = np.zeros(c, np.int64), np.zeros(c, np.int32), np.zeros(c, np.int32)
        self.pos, self.vel, self.x, self.dx = np.zeros((c, 3), dt), np.zeros((c, 3), dt), np.zeros((c, D), dt), np.zeros((c, D), dt)

    def alpha(self, fc, dt_):
        one = np.array(1.0, self.dt)
        return one / (one + (one / (self.two_pi * fc)) / dt_)

    def update(self, F, img_id, idx_y, idx_x, transl, readout, offset):
        dt, D, nb = self.dt, self.D, self.nb
        P = len(img_id)
        img_id = np.asarray(img_id, np.int64)
        transl, readout, offset = (np.asarray(a, np.float32).astype(dt) for a in (transl, readout, offset))
        transl, readout, offset = transl.reshape(P, 3), readout.reshape(P, D), offset.reshape(P, 2)
        out = dict(track_id=np.full(P, -1, np.int64), hits=np.zeros(P, np.int32), readout=readout.copy(), offset=offset.copy(), status=0)
        if P and (img_id.min() < 0 or img_id.max() >= F or np.any(np.diff(img_id) < 0)):
            out["status"] = 1
            return out
        half, cols = np.array(0.5, dt), state_columns(nb)
        for f in range(F):
            rows = np.nonzero(img_id == f)[0]
            n = len(rows)
            live = np.nonzero(self.hits > 0)[0]
            taken_d, slot_row = np.zeros(n, bool), {}
            if n and len(live):
                k = (self.missed[live] + 1).astype(dt)[:, None]
                p = self.pos[live] + self.vel[live] * k if self.predict else self.pos[live]
                e = transl[rows][:, None, :] - p[None]
                c = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                dd, tt = np.nonzero(c <= self.gate)
                order = np.lexsort((live[tt], dd, c[dd, tt]))          # (c, d, t): costs are >= 0, so their bits order like their values
                taken_t = set()
                for i in order:
                    d, t = int(dd[i]), int(live[tt[i]])
                    if not taken_d[d] and t not in taken_t:
                        taken_d[d] = True
                        taken_t.add(t)
                        slot_row[t] = d
            for t in live:                                               # steps 1 and 2
                t = int(t)
                if t in slot_row:
                    r = rows[slot_row[t]]
                    k = int(self.missed[t]) + 1
                    self.vel[t] = (transl[r] - self.pos[t]) / np.array(k, dt)
                    self.pos[t] = transl[r]
                    self.missed[t] = 0
                    self.hits[t] += 1
                    out["track_id"][r], out["hits"][r] = self.id[t], self.hits[t]
                    self._filter(t, k, r, readout, offset, idx_y, idx_x, out, cols, half)
                else:
                    self.missed[t] += 1
                    if self.missed[t] > self.max_age:
                        self.hits[t] = 0
            free = list(np.nonzero(self.hits == 0)[0])                   # steps 3 and 4
            for d in range(n):
                if taken_d[d] or not free:
                    continue
                t, r = int(free.pop(0)), rows[d]
                self.id[t], self.pos[t], self.vel[t], self.missed[t], self.hits[t] = self.next_id, transl[r], 0, 0, 1
                self.next_id += 1
                out["track_id"][r], out["hits"][r] = self.id[t], 1
                self._filter(t, 0, r, readout, offset, idx_y, idx_x, out, cols, half)
        return out

    def _filter(self, t, k, r, readout, offset, idx_y, idx_x, out, cols, half):
        dt, on = self.dt, self.on
        cell = np.array([idx_x[r], idx_y[r]]).astype(dt) + half
        z = np.concatenate([readout[r, cols], cell + offset[r]])
        if k == 0:
            self.x[t, on], self.dx[t, on] = z[on], 0
            return
        dt_ = np.array(k, dt) / self.fps
        x, dx = self.x[t], self.dx[t]
        e = z - x
        d = e / dt_
        dx_new = dx + self.alpha(self.dcutoff, dt_) * (d - dx)
        fc = self.minc + self.beta * np.abs(dx_new)
        x_new = x + self.alpha(fc, dt_) * e
        self.x[t, on], self.dx[t, on] = x_new[on], dx_new[on]
        ro, loc = on[:-2], on[-2:]
        out["readout"][r, cols[ro]] = x_new[:-2][ro]
        out["offset"][r, loc] = (x_new[-2:] - cell)[loc]

    def table(self):
        return dict(next_id=self.next_id, id=self.id, pos=self.pos, vel=self.vel, missed=self.missed, hits=self.hits, x=self.x, dx=self.dx)


def table_views(buf, capacity, D):
    """Views of the device table (a uint8 numpy array of mhmr_track_state_bytes(capacity, D) bytes) by the layout of include/mhmr.h."""
    c, o = capacity, 64
    v = dict(next_id=int(buf[:8].view(np.int64)[0]), reserved=buf[8:64])
    for name, dtype, shape in (("id", np.int64, (c,)), ("pos", np.float32, (c, 3)), ("vel", np.float32, (c, 3)), ("missed", np.int32, (c,)),
                               ("hits", np.int32, (c,)), ("x", np.float32, (c, D)), ("dx", np.float32, (c, D))):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        v[name] = buf[o:o + nbytes].view(dtype).reshape(shape)
        o += nbytes
    assert o == len(buf) == 64 + c * 40 + c * D * 8
    return v


def make_scene(frames, nb=10, seed=0, grid=16, **params):
    """``frames``: per frame the list of (x, y, z) of its persons, in row order -> the call's arrays (seeded N(0, 1) read-outs, offsets in
    +-0.5, cells in the grid) and the tracker's parameters."""
    rng = np.random.default_rng(seed)
    img_id = np.array([f for f, rows in enumerate(frames) for _ in rows], np.int64)
    P = len(img_id)
    transl = np.array([p for rows in frames for p in rows], np.float32).reshape(P, 3)
    return dict(F=len(frames), nb=nb, img_id=img_id, idx_y=rng.integers(0, grid, P).astype(np.int64), idx_x=rng.integers(0, grid, P).astype(np.int64),
                transl=transl, readout=rng.standard_normal((P, width(nb))).astype(np.float32),
                offset=rng.uniform(-0.5, 0.5, (P, 2)).astype(np.float32), params=dict(dict(capacity=8, max_dist=0.8, max_age=2), **params))


def call_args(sc, frames=None):
    """The update arguments of a scene, or of its frames ``[a, b)`` renumbered from 0."""
    a, b = frames if frames is not None else (0, sc["F"])
    m = (sc["img_id"] >= a) & (sc["img_id"] < b)
    return dict(F=b - a, img_id=sc["img_id"][m] - a, **{k: sc[k][m] for k in ("idx_y", "idx_x", "transl", "readout", "offset")})


def ids_by_frame(sc, track_id):
    return [[int(i) for i in track_id[sc["img_id"] == f]] for f in range(sc["F"])]


def scenes():
    """name -> (scene, the ids per frame the issue states, or None)."""
    at = lambda x, y=0.0, z=3.0: (x, y, z)
    S = {}
    cross = [sorted([at(-0.75 + 0.5 * f), at(0.75 - 0.5 * f)]) for f in range(4)]           # rows sorted by x: the row order swaps
    S["crossing"] = (make_scene(cross, nb=10, seed=1), [[0, 1], [0, 1], [1, 0], [1, 0]])
    A, B = at(0.0), at(2.0)
    S["leave_and_return"] = (make_scene([[A, B], [A], [A], [A, B], [A], [A], [A], [A, B]], nb=11, seed=2),
                             [[0, 1], [0], [0], [0, 1], [0], [0], [0], [0, 2]])
    S["empty_frames"] = (make_scene([[], [A], [], [], [A], [], [], [], [A]], nb=10, seed=3), [[], [0], [], [], [0], [], [], [], [1]])
    S["tie_two_detections"] = (make_scene([[A], [at(-0.25), at(0.25)]], nb=10, seed=4), [[0], [0, 1]])
    S["tie_two_tracks"] = (make_scene([[at(-0.25), at(0.25)], [A]], nb=11, seed=5), [[0, 1], [0]])
    three = [at(0.0), at(2.0), at(4.0)]
    S["capacity"] = (make_scene([three, three], nb=10, seed=6, capacity=2), [[0, 1, -1], [0, 1, -1]])
    crowd = [at(float(i % 10), float(i // 10), 5.0) for i in range(70)]
    ids = list(range(64)) + [-1] * 6
    S["crowd"] = (make_scene([crowd, crowd, crowd[::-1]], nb=10, seed=7, capacity=64), [ids, ids, ids[::-1]])
    return S


def filter_scene(nb, seed=11):
    """8 frames, two tracks 2 m apart; the second misses frame 3, so its frame 4 has k = 2."""
    A, B = (0.0, 0.0, 3.0), (2.0, 0.0, 3.0)
    return make_scene([[A, B] if f != 3 else [A] for f in range(8)], nb=nb, seed=seed)


def random_walk_scene(n=40, F=5, nb=10, seed=31, area=3.0, step=0.6):
    """n persons packed into 3 m x 3 m, each walking up to 0.6 m per frame and axis, a seeded fifth of them absent from every frame, the rows of every
    frame shuffled: neighbours compete for the same tracks, so the sweep's outcome depends on its order (and takes several rounds)."""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([rng.uniform(0, area, (n, 2)), np.full((n, 1), 5.0)], 1)
    frames = []
    for f in range(F):
        pos = pos + np.concatenate([rng.uniform(-step, step, (n, 2)), np.zeros((n, 1))], 1)
        there = rng.permutation(n)[:n - n // 5]
        frames.append([tuple(pos[i]) for i in there])
    return make_scene(frames, nb=nb, seed=seed, capacity=48, max_dist=0.8, max_age=1)


def wide_frame_scene(n=300, nb=11, seed=41):
    """Two frames of n persons on a 1 m grid, the second frame shuffled and moved by centimetres: more rows in a frame than the kernel keeps
    in LDS (256), more slots than a wave has lanes."""
    rng = np.random.default_rng(seed)
    pos = np.stack([np.arange(n) % 20, np.arange(n) // 20, np.full(n, 8.0)], 1).astype(np.float64)
    moved = (pos + np.concatenate([rng.uniform(-0.1, 0.1, (n, 2)), np.zeros((n, 1))], 1))[rng.permutation(n)]
    return make_scene([[tuple(p) for p in pos], [tuple(p) for p in moved]], nb=nb, seed=seed, capacity=320, max_dist=0.8, max_age=1)
