"""Time the 3D export (multi_hmr_amd/scene.py, csrc/scene.hip) on meshes the size of SMPL-X with random (not zero) vertices:
  (a) scene.pack_meshes at P = 256 and P = 8: hipEvents, median of --iters after warm-up, in microseconds and as a share of the HBM
      peak over its algorithmic bytes (read 12 B and write 24 B per vertex, plus the faces and the CSR once);
  (b) the device -> host copy of that block (and of the bounds), wall time around a synchronising copy;
  (c) scene.export_batch for B = 32 images / 256 persons into a RAM-backed directory, and its stages timed apart: pack, copy, files;
  (d) the same normals by tests/render_oracle.py::vertex_normals on this machine's CPU, per person, and the ratio (d) / (a per person).
--topology icosphere (default: subdivision 5, 10242 vertices / 20480 faces, a mesh's locality) or stand_in (the synthetic SMPL-X
stand-in, 10475 / 20908 with RANDOM faces: no locality at all, the worst case for the caches).  One JSON line per measurement.
  python tools/scene_bench.py [--iters 30] [--topology icosphere|stand_in]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multi_hmr_amd import scene  # noqa: E402
import render_oracle  # noqa: E402

STEP_MS = 129.0            # the headline forward step (bench.py, B = 32 at 896^2)
HBM_PEAK = 8.0e12          # bytes / s, MI355X


def meshes(topology, P, seed=0):
    rng = np.random.default_rng(seed)
    if topology == "icosphere":
        v, f = render_oracle.icosphere(5)
        v = 0.5 * v
    else:
        import synthetic
        data = synthetic.make_smplx_data(seed=0)
        v, f = np.asarray(data["v_template"], np.float32), np.asarray(data["f"], np.int32)
    verts = v[None] + 0.002 * rng.standard_normal((P,) + v.shape) + rng.uniform(-2, 2, size=(P, 1, 3)) + np.array([0, 0, 5.0])
    return verts.astype(np.float32), f


def median_us(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(1000.0 * e0.elapsed_time(e1))
    return float(np.median(us)), float(np.min(us))


def median_wall_us(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        us.append(1e6 * (time.perf_counter() - t0))
    return float(np.median(us)), float(np.min(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--topology", default="icosphere", choices=["icosphere", "stand_in"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    per_person_us = None
    for P in (256, 8):
        v, f = meshes(args.topology, P)
        V, F = v.shape[1], f.shape[0]
        verts = torch.from_numpy(v).to(dev)
        scene.pack_meshes(verts, f)                                       # builds and caches the CSR
        med, lo = median_us(lambda: scene.pack_meshes(verts, f), args.iters)
        nbytes = P * V * 36 + F * 12 + (V + 1) * 4 + 3 * F * 4
        print(json.dumps({"what": "a_pack_meshes", "topology": args.topology, "P": P, "V": V, "F": F, "median_us": round(med, 1),
                          "min_us": round(lo, 1), "us_per_person": round(med / P, 2), "algorithmic_bytes": nbytes,
                          "share_of_hbm_peak": round(nbytes / (med * 1e-6) / HBM_PEAK, 4),
                          "share_of_forward_step": round(med / 1000.0 / STEP_MS, 5)}), flush=True)
        if P == 256:
            per_person_us = med / P
        packed, bounds = scene.pack_meshes(verts, f)
        nb = 4 * (packed.numel() + bounds.numel())
        for reuse in (False, True):                                       # a pageable copy (create_scene), a page-locked one (export_batch)
            med, lo = median_wall_us(lambda: scene._to_host(packed, bounds, reuse=reuse), args.iters)
            print(json.dumps({"what": "b_device_to_host", "P": P, "page_locked": reuse, "bytes": nb, "median_us": round(med, 1),
                              "min_us": round(lo, 1), "GB_per_s": round(nb / (med * 1e-6) / 1e9, 2)}), flush=True)

    # (c) a batch: 32 images, 8 persons each, to a RAM-backed directory
    B, P = 32, 256
    v, f = meshes(args.topology, P, seed=1)
    verts = torch.from_numpy(v).to(dev)
    index = torch.arange(P, dtype=torch.int32, device=dev) // (P // B)
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    folder = tempfile.mkdtemp(prefix="scene_bench_", dir=shm)
    try:
        paths = [os.path.join(folder, f"{b}.glb") for b in range(B)]
        med, lo = median_wall_us(lambda: scene.export_batch(verts, index, f, paths), max(args.iters // 3, 5), warmup=2)
        size = sum(os.path.getsize(p) for p in paths)
        packed, bounds = scene.pack_meshes(verts, f)
        pack_us, _ = median_us(lambda: scene.pack_meshes(verts, f), args.iters)
        copy_us, _ = median_wall_us(lambda: scene._to_host(packed, bounds, reuse=True), args.iters)
        block, bnd = scene._to_host(packed, bounds, reuse=True)
        cols = np.full((P, 3), 0.5)
        per = P // B

        def files():
            for b in range(B):
                scene.GlbScene(scene.glb_parts(block[b * per:(b + 1) * per], bnd[b * per:(b + 1) * per], f,
                                               cols[b * per:(b + 1) * per])).export(paths[b])
        files_us, _ = median_wall_us(files, max(args.iters // 3, 5), warmup=2)
        print(json.dumps({"what": "c_export_batch", "B": B, "P": P, "ram_backed": shm is not None, "bytes_written": size,
                          "total_ms": round(med / 1000, 2), "min_ms": round(lo / 1000, 2), "pack_ms": round(pack_us / 1000, 3),
                          "copy_ms": round(copy_us / 1000, 2), "files_ms": round(files_us / 1000, 2),
                          "share_of_forward_step": round(med / 1000.0 / STEP_MS, 3)}), flush=True)
    finally:
        shutil.rmtree(folder, ignore_errors=True)

    # (d) the host's normals
    v, f = meshes(args.topology, 3, seed=2)
    ms = []
    for p in range(3):
        t0 = time.perf_counter()
        render_oracle.vertex_normals(v[p], f)
        ms.append(1000 * (time.perf_counter() - t0))
    cpu_ms = float(np.median(ms))
    print(json.dumps({"what": "d_host_vertex_normals", "ms_per_person": round(cpu_ms, 2), "device_us_per_person": round(per_person_us, 2),
                      "ratio_host_over_device": round(cpu_ms * 1000 / per_person_us, 1),
                      "host_ms_for_256_persons": round(256 * cpu_ms, 1)}), flush=True)


if __name__ == "__main__":
    main()
