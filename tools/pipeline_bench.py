#!/usr/bin/env python
"""Images/s from JPEG files to persons: (a) pipeline.predict_images at batch 32, (b) the one-image way it replaces (open_image +
forward_model per file, no rendering), (c) the forward alone at B = 32 on prepared tensors (the ceiling of (a)), and (c') the
forward alone over the very batches (a) infers, prepared on the device beforehand.

ViT-L 896^2, f16, the synthetic weights of bench.py; 256 JPEG files of 800x533 written from a seed into a temporary folder.  The
detection threshold is placed as bench.py's inference leg places it (about 8 persons per image on the first batch), the same for all
three.  Host clocks around work that ends in a synchronise; the per-stage seconds of (a) are predict_images' own counters."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import synthetic  # noqa: E402
from multi_hmr_amd import Model, forward_model, get_camera_parameters, open_image, predict_images  # noqa: E402
from multi_hmr_amd.preprocess import Preprocessor  # noqa: E402


def write_jpegs(folder, n, W=800, H=533, seed=0):
    """n photograph-like JPEGs (smooth gradients + blobs + mild noise: a file size and a decode cost like a photograph's)."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    paths = []
    for j in range(n):
        img = np.stack([128 + 100 * np.sin(xx / rng.uniform(20, 200) + rng.uniform(0, 6)) * np.cos(yy / rng.uniform(20, 200))
                        for _ in range(3)], -1)
        for _ in range(6):
            cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(20, 120)
            img[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] = rng.uniform(0, 255, size=3)
        img += rng.normal(0, 6, size=img.shape)
        p = os.path.join(folder, f"{j:04d}.jpg")
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(p, quality=90)
        paths.append(p)
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--backbone", default="dinov2_vitl14")
    ap.add_argument("--img-size", type=int, default=896)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--persons", type=int, default=8, help="detections per image the threshold aims at")
    ap.add_argument("--cold", action="store_true", help="skip (c'), so that (a) is the first to meet its batches' person counts")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pipeline_bench needs the GPU"
    dev, S, B = torch.device("cuda:0"), args.img_size, args.batch
    smplx_data, mean_params = synthetic.make_smplx_data(0), synthetic.make_mean_params(0)
    model = Model(backbone=args.backbone, img_size=S, smplx_data=smplx_data, mean_params=mean_params, precision="f16")
    model.load_state_dict(synthetic.make_state_dict(args.backbone, S, seed=0, mean_params=mean_params), strict=True)
    model = model.to(dev).eval()

    with tempfile.TemporaryDirectory() as folder:
        t0 = time.perf_counter()
        paths = write_jpegs(folder, args.images)
        print(f"wrote {len(paths)} JPEG files, {sum(os.path.getsize(p) for p in paths) / len(paths) / 1e3:.0f} kB each, "
              f"in {time.perf_counter() - t0:.1f} s", flush=True)
        from multi_hmr_amd.pipeline import decode_image
        x = Preprocessor(S, dev).batch([decode_image(p)[0] for p in paths[:B]])
        K = get_camera_parameters(S, device=dev, batch=B)
        # the threshold: in the gap below the (B * persons)-th largest score that survives the 3x3 NMS, as bench.py's inference leg
        empty = tuple(torch.zeros(0, dtype=torch.long, device=dev) for _ in range(4))
        s = model(x, idx=empty, K=K, is_training=True)["scores"][..., 0]
        m = torch.nn.functional.max_pool2d(s[:, None], 3, stride=1, padding=1)[:, 0]
        surv = torch.sort(s[m == s], descending=True).values
        n = min(B * args.persons, surv.numel() - 1)
        thr = float(0.5 * (surv[n - 1] + surv[n]))
        kw = dict(det_thresh=thr, nms_kernel_size=3)

        # (c) the forward alone, B images resident on the device
        run = lambda: model(x, K=K, **kw)
        for _ in range(2):
            persons_c = run()
        torch.cuda.synchronize()
        steps = 8
        t0 = time.perf_counter()
        for _ in range(steps):
            run()
        torch.cuda.synchronize()
        c = B * steps / (time.perf_counter() - t0)
        print(f"(c) forward alone, B = {B}: {c:.1f} images/s ({1e3 * B / c:.1f} ms per step, {len(persons_c)} persons)", flush=True)

        # (c') the forward alone over the SAME batches as (a), prepared on the device beforehand: what the varying content costs
        # (the person count changes from batch to batch, so the heads' row capacity is sometimes exceeded and they run twice)
        c2 = None
        if not args.cold:
            pre = Preprocessor(S, dev)
            xs = [pre.batch([decode_image(p)[0] for p in paths[i:i + B]]) for i in range(0, len(paths), B)]
            for xi in xs[:2]:
                model(xi, K=K[:xi.shape[0]], **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for xi in xs:
                model(xi, K=K[:xi.shape[0]], **kw)
            torch.cuda.synchronize()
            c2 = len(paths) / (time.perf_counter() - t0)
            del xs
            print(f"(c') forward alone over the {len(paths) // B} batches of (a), resident on the device: {c2:.1f} images/s "
                  f"({1e3 * B / c2:.1f} ms per step)", flush=True)

        # (a) the pipeline (a warm-up pass over two batches: workspaces, tables, pinned buffers)
        n_warm = sum(len(r.humans) for r in predict_images(model, paths[:2 * B], batch_size=B, workers=args.workers, **kw))
        torch.cuda.synchronize()
        stats = {}
        t0 = time.perf_counter()
        n_persons = sum(len(r.humans) for r in predict_images(model, paths, batch_size=B, workers=args.workers, stats=stats, **kw))
        torch.cuda.synchronize()
        ta = time.perf_counter() - t0
        a = len(paths) / ta
        nb = stats["batches"]
        print(f"(a) predict_images, batch_size = {B}, {args.workers} decode threads: {a:.1f} images/s ({ta:.2f} s, {n_persons} persons; "
              f"warm-up {n_warm}); per batch: forward {1e3 * stats['forward'] / nb:.1f} ms, consumer waiting for a staged batch "
              f"{1e3 * stats['wait'] / nb:.1f} ms, producer staging {1e3 * stats['stage'] / nb:.1f} ms, decode "
              f"{1e3 * stats['decode'] / len(paths):.2f} ms per image per thread "
              f"(= {1e3 * stats['decode'] / nb / min(args.workers, 16):.1f} ms per batch over the threads)", flush=True)

        # (b) one image at a time: open_image + forward_model per file
        K1 = get_camera_parameters(S, device=dev)
        for p in paths[:4]:
            forward_model(model, open_image(p, S, dev)[0], K1, **kw)
        torch.cuda.synchronize()
        n_b = min(len(paths), 128)
        t0 = time.perf_counter()
        persons_b = 0
        for p in paths[:n_b]:
            xb, _ = open_image(p, S, dev)
            persons_b += len(forward_model(model, xb, get_camera_parameters(S, device=dev), **kw))
        torch.cuda.synchronize()
        b = n_b / (time.perf_counter() - t0)
        print(f"(b) open_image + forward_model per file ({n_b} files): {b:.1f} images/s ({persons_b} persons)", flush=True)

    result = {"metric": "pipeline_images_per_s", "a_predict_images": round(a, 2), "b_one_image_at_a_time": round(b, 2),
              "c_forward_alone": round(c, 2), "c2_forward_alone_same_batches": c2 and round(c2, 2), "a_over_c2": c2 and round(a / c2, 3), "a_over_b": round(a / b, 3), "a_over_c": round(a / c, 3), "batch": B, "images": len(paths),
              "workers": args.workers, "det_thresh": thr, "persons_a": n_persons,
              "per_batch_ms": {k: round(1e3 * stats[k] / nb, 2) for k in ("forward", "wait", "stage")},
              "decode_ms_per_image": round(1e3 * stats["decode"] / len(paths), 3)}
    print(json.dumps(result))
    assert a > b, "the batched pipeline must beat one image at a time"


if __name__ == "__main__":
    main()
