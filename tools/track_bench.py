"""Time the tracker (Tracker.update: one call of mhmr_track_update per batch of frames, nothing copied to the host) against the host form a
user would otherwise write: one ``.cpu()`` copy of the batch's rows, then the tracker in numpy (tests/track_oracle.py, fp32).
  Sizes: 32 frames x 1 person, 32 frames x 5 persons (160 rows), 2 frames x 160 persons; capacity 256, the default filter.
  The persons stand 1.5 m apart and jitter by centimetres, so every call matches every row to its track (the first call, which creates
  the tracks, is part of the warm-up).  Each repetition times both forms, alternating: ``update`` by device events around the call, the
  host form by the wall clock around copy + numpy (the device is idle before it starts).  "faster" is true only if update's WORST
  repetition beats the host form's BEST.
  Also, not gated: predict_video against predict_images in images/s on the same frames (a depth-3 ViT-S at 224^2 with synthetic weights: the
  difference is the tracker and the second decode_readout).
  --trace-only runs update alone (for a kernel trace in a run of its own).
Prints one JSON line per measurement and writes them to --out.
  python tools/track_bench.py [--reps 9] [--warmup 3] [--trace-only] [--out profiles/track_bench.txt]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from multi_hmr_amd import Model, Preprocessor, Tracker, predict_images, predict_video  # noqa: E402
from multi_hmr_amd.preprocess import get_camera_parameters  # noqa: E402
import synthetic  # noqa: E402
import track_oracle as to  # noqa: E402

DEV = "cuda:0"
S, NB, NAME, CAPACITY = 224, 10, "dinov2_vits14", 256


def make_batch(F, n, seed):
    """F frames of n persons on a 1.5 m grid, each jittering by centimetres about its place -> the batched dict, img_id."""
    rng = np.random.default_rng(seed)
    place = np.stack([1.5 * (np.arange(n) % 16), 1.5 * (np.arange(n) // 16), np.full(n, 6.0)], 1)
    transl = (place[None] + 0.02 * rng.standard_normal((F, n, 3))).reshape(F * n, 3).astype(np.float32)
    P = F * n
    dev = lambda a: torch.from_numpy(a).to(DEV)
    batch = dict(transl=dev(transl), readout=dev(rng.standard_normal((P, to.width(NB))).astype(np.float32)),
                 offset=dev(rng.uniform(-0.5, 0.5, (P, 2)).astype(np.float32)),
                 idx=(dev(np.repeat(np.arange(F), n)), dev(rng.integers(0, 16, P)), dev(rng.integers(0, 16, P))))
    return batch, batch["idx"][0]


def host_form(oracle, batch, F):
    """One copy to the host, then numpy."""
    P = batch["readout"].shape[0]
    flat = torch.cat([batch["readout"], batch["offset"], batch["transl"], torch.stack(batch["idx"], 1).float()], 1).cpu().numpy()
    W = to.width(NB)
    idx = flat[:, W + 5:].astype(np.int64)
    return oracle.update(F, idx[:, 0], idx[:, 1], idx[:, 2], flat[:, W + 2:W + 5], flat[:, :W], flat[:, W:W + 2]), P


def part(model, F, n, a, lines):
    batch, img = make_batch(F, n, seed=F * 1000 + n)
    tracker = Tracker(model, capacity=CAPACITY)
    oracle = to.OracleTracker(NB, capacity=CAPACITY, dtype=np.float32)
    ms = dict(update=[], host=[])
    for rep in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = tracker.update(batch, img, F)
        e1.record()
        torch.cuda.synchronize()
        t_update = e0.elapsed_time(e1)
        t_host = None
        if not a.trace_only:
            t0 = time.perf_counter()
            ref, _ = host_form(oracle, batch, F)
            t_host = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(res.track_id.cpu().numpy(), ref["track_id"]) and np.array_equal(res.hits.cpu().numpy(), ref["hits"])
        if rep >= a.warmup:
            ms["update"].append(t_update)
            if t_host is not None:
                ms["host"].append(t_host)
    out = dict(part=f"track_{F}x{n}", frames=F, persons_per_frame=n, rows=F * n, capacity=CAPACITY, launches_per_update=2,
               ids_equal_the_host_forms=not a.trace_only)
    for k, v in ms.items():
        if v:
            out[k] = dict(median_ms=round(float(np.median(v)), 4), best_ms=round(min(v), 4), worst_ms=round(max(v), 4), reps=len(v))
    if ms["host"]:
        out["faster"] = bool(max(ms["update"]) < min(ms["host"]))
        out["median_ratio_host_over_update"] = round(float(np.median(ms["host"]) / np.median(ms["update"])), 1)
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)


def pipeline_part(model, a, lines):
    g = torch.Generator().manual_seed(0)
    base = torch.randint(0, 256, (S, S, 3), generator=g, dtype=torch.uint8)
    frames = [torch.roll(base, f % 14, dims=1).numpy() for f in range(128)]
    x = Preprocessor(S, torch.device(DEV)).batch([torch.from_numpy(f) for f in frames[:14]])
    K = get_camera_parameters(S, fov=60, device=torch.device(DEV), batch=14)
    z = torch.zeros(1, dtype=torch.long, device=DEV)
    top = model(x, idx=(z, z + 3, z + 5), K=K, is_training=True)["scores"].flatten().sort(descending=True).values
    thr = float(top[41] + top[42]) / 2                                           # about three persons per frame
    rate, persons = dict(predict_images=[], predict_video=[]), 0
    for rep in range(1 + 3):
        for name in rate:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "predict_images":
                res = list(predict_images(model, frames, batch_size=32, det_thresh=thr))
            else:
                res = list(predict_video(model, frames, batch_size=32, tracker=Tracker(model, max_dist=1e3), det_thresh=thr))
            torch.cuda.synchronize()
            if rep:
                rate[name].append(len(frames) / (time.perf_counter() - t0))
            persons = sum(len(r.humans) for r in res)
    out = dict(part="pipeline_vits14_224_depth3", frames=len(frames), batch_size=32, persons=persons,
               images_per_s={k: [round(x, 1) for x in v] for k, v in rate.items()})
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_bench measures on the GPU; there is none here")
    data, mean = synthetic.make_smplx_data(0), synthetic.make_mean_params(0)
    model = Model(backbone=NAME, img_size=S, smplx_data=data, mean_params=mean, backbone_depth=3, precision="f16")
    model.load_state_dict(synthetic.make_state_dict(NAME, S, seed=42, depth_override=3, mean_params=mean), strict=True)
    model = model.to(DEV).eval()
    lines = []
    for F, n in ((32, 1), (32, 5), (2, 160)):
        part(model, F, n, a, lines)
    if not a.trace_only:
        pipeline_part(model, a, lines)
        head = ("tools/track_bench.py -- Tracker.update (mhmr_track_update, two launches, no host copy) against the host form (one .cpu() copy,\n"
                "then tests/track_oracle.py in numpy fp32), forms alternating inside each repetition, one MI355X\n"
                f"  python tools/track_bench.py --reps {a.reps} --warmup {a.warmup}\n\n")
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(head + "\n".join(lines) + "\n")
