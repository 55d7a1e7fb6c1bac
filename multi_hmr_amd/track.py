"""Track persons across video frames and smooth them (``mhmr_track_update``, csrc/track.hip).

``Tracker(model).update(batched, img_id, frames)`` takes what ``model(x, K=K, return_batched=True, return_readout=True)`` returns for a batch of
``frames`` consecutive video frames and gives every person row a stable ``track_id`` and temporally filtered ``readout`` / ``offset`` rows;
``model.decode_readout(result.readout, result.offset, batched["idx"], K)`` turns those into the smoothed meshes.  The slot table lives on the
device and the call enqueues two launches: no host round trip, no synchronisation.  The contract -- the table, the greedy association and its
tie rule, the One-Euro filter -- is written down once, in include/mhmr.h.

There is no CPU path: CPU tensors raise."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import torch

from . import _lib
from .heads import readout_width

#: the One-Euro paper's starting points (mincutoff in Hz, beta) for every group; ``shape`` does not change within a clip: a pure slow low-pass
DEFAULT_SMOOTH = dict(pose=(1.0, 0.007), shape=(0.1, 0.0), depth=(1.0, 0.007), expr=(1.0, 0.007), loc=(1.0, 0.007))


class TrackResult(NamedTuple):
    track_id: torch.Tensor      # [P] int64; -1: the table was full (or status 1)
    hits: torch.Tensor          # [P] int32 frames the track has been seen in, this one included; 1 = a new track
    readout: torch.Tensor       # [P, 318 + num_betas + 13] the filtered rows (new tensor)
    offset: torch.Tensor        # [P, 2]
    status: torch.Tensor        # [1] int32 on the device: 0 ok, 1 = img_id decreasing or out of range (nothing was tracked)


class Tracker:
    """``Tracker(model, fps=30.0, max_dist=1.0, max_age=30, capacity=256, smooth=DEFAULT_SMOOTH, dcutoff=1.0)``.

    ``max_dist`` (metres) gates a detection against a track's predicted position, ``max_age`` is the number of frames a track survives unseen,
    ``capacity`` the number of slots (1 ... 1024; a person who finds none gets ``track_id`` -1 and unfiltered rows).  ``smooth`` maps the groups
    ``pose``, ``shape``, ``depth``, ``expr`` (``expression``, the fitter's spelling, is read too) and ``loc`` to ``(mincutoff, beta)`` of their One-Euro filter;
    a group set to ``None`` keeps its bits, a missing group gets the default, ``smooth=None`` tracks only."""

    def __init__(self, model, fps: float = 30.0, max_dist: float = 1.0, max_age: int = 30, capacity: int = 256, smooth: dict | None = DEFAULT_SMOOTH,
                 dcutoff: float = 1.0):
        positive = lambda v: isinstance(v, (int, float)) and math.isfinite(v) and v > 0
        if not positive(fps) or not positive(dcutoff):
            raise ValueError("fps and dcutoff must be finite and positive")
        if not (isinstance(max_dist, (int, float)) and math.isfinite(max_dist) and max_dist >= 0):
            raise ValueError("max_dist must be finite and non-negative")
        if int(max_age) != max_age or max_age < 0:
            raise ValueError("max_age must be a non-negative integer")
        if int(capacity) != capacity or not 1 <= capacity <= _lib.TRACK_MAX_CAPACITY:
            raise ValueError(f"capacity must be 1 ... {_lib.TRACK_MAX_CAPACITY}")
        groups = {}
        if smooth is not None:
            given = {("expr" if k == "expression" else k): v for k, v in smooth.items()}
            bad = [k for k in given if k not in _lib.TRACK_GROUPS]
            if bad or len(given) != len(smooth):
                raise ValueError(f"unknown or repeated groups {bad}: the groups are {_lib.TRACK_GROUPS}")
            for g, v in {**DEFAULT_SMOOTH, **given}.items():
                if v is None:
                    continue
                if len(v) != 2 or not positive(v[0]) or not (math.isfinite(v[1]) and v[1] >= 0):
                    raise ValueError(f"smooth[{g!r}] must be (mincutoff > 0, beta >= 0) or None")
                groups[g] = (float(v[0]), float(v[1]))
        self.model, self.fps, self.max_dist, self.max_age, self.capacity = model, float(fps), float(max_dist), int(max_age), int(capacity)
        self.groups, self.dcutoff = groups, float(dcutoff)
        self.nb = int(model.num_betas)
        self.width = readout_width(self.nb)
        self.table = None             # the slot table: int64 words on the device, allocated (zeros = empty) by the first update
        self._ws: dict = {}           # (frames, device) -> workspace

    def _state(self, dev):
        if self.table is None:
            nbytes = _lib.workspace_bytes("mhmr_track_state_bytes", self.capacity, self.width)
            self.table = torch.zeros(nbytes // 8, dtype=torch.int64, device=dev)
        elif self.table.device != dev:
            raise ValueError(f"the tracker's table is on {self.table.device}, the batch on {dev}")
        return self.table

    def _workspace(self, frames, dev):
        key = (frames, dev.type, dev.index)
        if key not in self._ws:
            nbytes = _lib.workspace_bytes("mhmr_track_workspace_bytes", frames, self.capacity)
            self._ws[key] = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        return self._ws[key]

    def reset(self):
        """Forget every track; the next id is 0 again."""
        if self.table is not None:
            self.table.zero_()

    def state_dict(self) -> dict:
        """The table (a copy; ``None`` before the first update) and the two sizes that fix its layout."""
        return dict(table=None if self.table is None else self.table.clone(), capacity=self.capacity, width=self.width)

    def load_state_dict(self, state: dict):
        if state["capacity"] != self.capacity or state["width"] != self.width:
            raise ValueError("the state belongs to a tracker of another capacity or read-out width")
        table = state["table"]
        if table is None:
            self.table = None
            return
        nbytes = _lib.workspace_bytes("mhmr_track_state_bytes", self.capacity, self.width)
        if table.dtype != torch.int64 or table.dim() != 1 or table.numel() != nbytes // 8 or not table.is_cuda:
            raise ValueError("the state's table has another size, dtype or is not on the device")
        self.table = table.clone()

    @torch.no_grad()
    def update(self, batched: dict, img_id, frames: int) -> TrackResult:
        """``batched``: the dict of ``model(x, K=K, return_batched=True, return_readout=True)`` for ``frames`` consecutive frames (the empty
        dict: nobody in the batch, time passes all the same), ``img_id [P]`` the frame of every row as that call returns it.  The inputs are
        not modified; nothing is copied to the host."""
        frames = int(frames)
        if frames < 1:
            raise ValueError("frames must be at least 1")
        W = self.width
        if batched:
            missing = [k for k in ("transl", "readout", "offset", "idx") if k not in batched]
            if missing:
                raise ValueError(f"batched lacks {missing}: call the model with return_batched=True, return_readout=True")
            readout = batched["readout"]
            if not readout.is_cuda:
                raise _lib.MhmrError("Tracker.update runs on the HIP device only (no CPU fallback)")
            dev = readout.device
        else:
            dev = img_id.device if torch.is_tensor(img_id) and img_id.is_cuda else next(self.model.parameters()).device
            if dev.type != "cuda":
                raise _lib.MhmrError("Tracker.update runs on the HIP device only (no CPU fallback)")
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        i64 = lambda t: t.detach().to(device=dev, dtype=torch.int64).contiguous()
        with torch.cuda.device(dev):
            if batched:
                r, o, tr = f32(readout), f32(batched["offset"]), f32(batched["transl"])
                Pn = int(r.shape[0])
                if r.dim() != 2 or r.shape[1] != W or tuple(o.shape) != (Pn, 2) or tuple(tr.shape) != (Pn, 3):
                    raise ValueError(f"readout must be [P, {W}], offset [P, 2] and transl [P, 3]")
                ids, iy, ix = i64(img_id), i64(batched["idx"][1]), i64(batched["idx"][2])
                if any(tuple(t.shape) != (Pn,) for t in (ids, iy, ix)):
                    raise ValueError("img_id and idx must hold one entry per read-out row")
            else:
                Pn = 0
                r, o, tr = (torch.empty(0, n, dtype=torch.float32, device=dev) for n in (W, 2, 3))
                ids = iy = ix = torch.empty(0, dtype=torch.int64, device=dev)
            res = TrackResult(torch.empty(Pn, dtype=torch.int64, device=dev), torch.empty(Pn, dtype=torch.int32, device=dev), torch.empty_like(r),
                              torch.empty_like(o), torch.empty(1, dtype=torch.int32, device=dev))
            table, ws = self._state(dev), self._workspace(frames, dev)
            d = _lib.TrackDesc()
            d.F, d.P, d.nb, d.capacity = frames, Pn, self.nb, self.capacity
            for n, t in (("img_id", ids), ("idx_y", iy), ("idx_x", ix), ("transl", tr), ("readout", r), ("offset", o), ("state", table),
                         ("workspace", ws), ("track_id", res.track_id), ("hits", res.hits), ("readout_s", res.readout), ("offset_s", res.offset),
                         ("status", res.status)):
                setattr(d, n, _lib.ptr(t) or None)
            d.fps, d.max_dist, d.max_age, d.dcutoff = self.fps, self.max_dist, self.max_age, self.dcutoff
            d.groups = 0
            for bit, g in enumerate(_lib.TRACK_GROUPS):
                if g in self.groups:
                    d.groups |= 1 << bit
                    setattr(d, "mincutoff_" + g, self.groups[g][0])
                    setattr(d, "beta_" + g, self.groups[g][1])
            d.state_bytes, d.workspace_bytes = table.numel() * 8, ws.numel() * 8
            _lib.check(_lib.lib().mhmr_track_update(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "mhmr_track_update")
        return res


__all__ = ["DEFAULT_SMOOTH", "TrackResult", "Tracker"]
