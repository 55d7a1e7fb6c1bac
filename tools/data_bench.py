"""Time the training-data path.  One process; forms alternate; device events and host wall time; medians.
  orient   32 decoded images of 1280 x 720 -> 896^2, half of them mirrored, eight of them closeups to rotate (720 x 1280 once oriented):
           Preprocessor.batch_oriented   against   the route without it: torch.rot90 / flip + .contiguous() per image, then
           Preprocessor.batch -- with the images on the device and in pinned host memory
  loader   TrainLoader over PNG files of that size at 16 workers: images / s with nothing behind it, then workload/ratio_data of a
           Trainer.train_n_iters pass at the headline shape (ViT-L 896^2, 32 images, f16) from the loader and from cached features
  python tools/data_bench.py [--reps 10] [--warmup 2] [--images 32] [--files 64] [--batches 8] [--workers 16]"""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import synthetic  # noqa: E402
from multi_hmr_amd import BEDLAM, BodyModel, GroundTruth, HeadsAdam, Loss, Model, Preprocessor, Trainer, TrainLoader  # noqa: E402
from eval_bench import DEV, report  # noqa: E402

W0, H0 = 1280, 720


def picture(g):
    """A stored 1280 x 720 frame: smooth content plus mild noise (a PNG of it decodes like a rendered frame, not like white noise)."""
    yy, xx = np.mgrid[0:H0, 0:W0]
    base = np.stack([xx * 255.0 / W0, yy * 255.0 / H0, 127 + 120 * np.sin(xx / 37.0) * np.cos(yy / 23.0)], -1)
    return np.clip(base + g.integers(-6, 7, (H0, W0, 3)), 0, 255).astype(np.uint8)


def timed(forms, a):
    dev, wall = {k: [] for k in forms}, {k: [] for k in forms}
    for r in range(a.warmup + a.reps):
        for name, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if r >= a.warmup:
                dev[name].append(e0.elapsed_time(e1))
                wall[name].append((t1 - t0) * 1e3)
    return dev, wall


def part_orient(a):
    g = np.random.default_rng(0)
    B, S = a.images, 896
    orient = [(2 if j % 4 == 3 else 0) | (j // 2 % 2) for j in range(B)]          # a quarter rotated, half mirrored (both kinds)
    host = [torch.from_numpy(picture(g)).pin_memory() for _ in range(B)]
    device = [t.to(DEV) for t in host]
    pre = Preprocessor(S, DEV)
    out = torch.empty(B, 3, S, S, device=DEV)

    def parent_route(imgs):
        oriented = []
        for t, o in zip(imgs, orient):
            if o & 2:
                t = torch.rot90(t, -1, (0, 1))
            if o & 1:
                t = t.flip(1)
            oriented.append(t.contiguous())
        return pre.batch(oriented, out=out)
    lines = []
    for where, imgs in (("device", device), ("pinned_host", host)):
        same = torch.equal(pre.batch_oriented(imgs, orient).clone(), parent_route(imgs))
        dev, wall = timed({"batch_oriented": lambda: pre.batch_oriented(imgs, orient, out=out), "rot90_flip_then_batch": lambda: parent_route(imgs)}, a)
        med = lambda v: float(np.median(v))
        lines.append(report(f"orient_{where}", dev, dict(
            images=B, size=S, stored=f"{W0}x{H0}", rotated=sum(1 for o in orient if o & 2), mirrored=sum(1 for o in orient if o & 1),
            same_bits=bool(same), wall_ms={k: round(med(v), 4) for k, v in wall.items()},
            median_ratio_parent_over_oriented=round(med(dev["rot90_flip_then_batch"]) / med(dev["batch_oriented"]), 3),
            wall_ratio_parent_over_oriented=round(med(wall["rot90_flip_then_batch"]) / med(wall["batch_oriented"]), 3),
            oriented_faster=bool(max(dev["batch_oriented"]) < min(dev["rot90_flip_then_batch"])),
            note="device events around the whole call (the copy of the staging buffer included); wall = issue + synchronize")))
    return lines


def part_loader(a):
    from PIL import Image
    g = np.random.default_rng(1)
    root = tempfile.mkdtemp(prefix="mhmr_data_bench_")
    os.makedirs(os.path.join(root, "training", "seq_closeup"))
    annots = {}
    person = lambda: dict({k: (0.2 * g.standard_normal(sh)).astype(np.float32) for k, sh in (
        ("smplx_root_pose", (1, 3)), ("smplx_body_pose", (21, 3)), ("smplx_jaw_pose", (1, 3)), ("smplx_leye_pose", (1, 3)),
        ("smplx_reye_pose", (1, 3)), ("smplx_left_hand_pose", (15, 3)), ("smplx_right_hand_pose", (15, 3)), ("smplx_shape", (11,)))},
        smplx_gender="neutral", smplx_transl=np.asarray([g.uniform(-0.8, 0.8), g.uniform(-0.3, 0.3), g.uniform(3, 6)], np.float32))
    for i in range(a.files):
        name = f"seq_closeup/f_{i:03d}.png" if i % 4 == 3 else f"f_{i:03d}.png"
        Image.fromarray(picture(g)).save(os.path.join(root, "training", name), compress_level=1)
        annots[name] = {"focal": np.asarray([1.2 * W0, 1.2 * W0], np.float32), "princpt": np.asarray([W0 / 2, H0 / 2], np.float32),
                        "size": np.asarray([W0, H0], np.int32), "humans": [person() for _ in range(8)]}
    B, S = a.images, 896
    ds = BEDLAM(split="training", training=True, img_size=S, root_dir=root, annots=annots, n_iter=B * a.batches, seed=0)
    lines = []
    loader = TrainLoader(ds, B, DEV, workers=a.workers)
    for _ in loader:                                     # warm-up: tables, staging buffers, page cache
        break
    t0 = time.perf_counter()
    n = sum(int(x.shape[0]) for x, _ in loader)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lines.append(dict(part="loader_alone", images=n, seconds=round(dt, 3), images_per_s=round(n / dt, 1), workers=a.workers, batch=B,
                      files=f"{a.files} PNG of {W0}x{H0}", ms_per_batch=round(dt / a.batches * 1e3, 1)))
    print(json.dumps(lines[-1]), flush=True)

    smplx_data, mean_params = synthetic.make_smplx_data(0), synthetic.make_mean_params(0)
    m = Model(backbone=a.backbone, img_size=S, smplx_data=smplx_data, mean_params=mean_params, precision="f16")
    m.load_state_dict(synthetic.make_state_dict(a.backbone, S, seed=0, mean_params=mean_params), strict=True)
    m = m.to(DEV).eval().train_heads_(True).train_detection_(True)
    import loss_oracle as lo
    ns = lo.default_args(save_dir=tempfile.mkdtemp(prefix="mhmr_data_bench_log_"), name="run", log_freq=1, max_epochs=1)
    scalars = {}
    writer = SimpleNamespace(add_scalar=lambda tag, v, step: scalars.__setitem__(tag, float(v)), flush=lambda: None)
    tr = Trainer(m, Loss(ns), HeadsAdam(m, lr=1e-6), ns, GroundTruth(S, patch_size=14, smplx_neutral=BodyModel(smplx_data, "smplx", num_betas=11)),
                 writer=writer)
    tr.current_epoch = lo.DEFAULTS["start_2d_epoch"]
    for source in ("images_warm_up", "images", "cached_features"):
        ds.seed(0)
        data = TrainLoader(ds, B, DEV, workers=a.workers)
        if source == "cached_features":
            data = tr.cache_features(data)
        scalars.clear()
        t0 = time.perf_counter()
        tr.train_n_iters(data)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        line = dict(part=f"train_n_iters_from_{source}", backbone=a.backbone, size=S, batch=B, batches=a.batches, seconds=round(dt, 3),
                    ms_per_batch=round(dt / a.batches * 1e3, 1), ratio_data=round(scalars.get("workload/ratio_data", float("nan")), 4),
                    data_ms=round(scalars.get("workload/data", float("nan")) * 1e3, 2), batch_ms=round(scalars.get("workload/batch", float("nan")) * 1e3, 2))
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def main(a):
    lines = part_orient(a) + ([] if a.no_loader else part_loader(a))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("# tools/data_bench.py: Preprocessor.batch_oriented against rot90 / flip + Preprocessor.batch; the TrainLoader alone and in front of a "
                 "Trainer.train_n_iters pass\n")
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--backbone", default="dinov2_vitl14")
    ap.add_argument("--no-loader", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_data.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("data_bench measures on the GPU; there is none here")
    main(a)
