#!/usr/bin/env python
"""Headline benchmark: images/s of the whole Multi-HMR forward (ViT-L 896x896, batch 32 per GPU, 8 pinned
queries per image -> HPH -> SMPL-X LBS), BASELINE.json config #4 (`multiHMR_896_L`, image-sharded over N GPUs).

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A "step" = one full `Model.forward` over one batch of synthetic images already resident in HBM (seeded N(0,1) pixels, seeded
random weights of the named architecture, synthetic SMPL-X arrays), detections pinned to 8 per image through the reference's own
`idx=` / `is_training=True` hook (model.py:141-151), plus -- for N > 1 -- the RCCL all-gather that collates every rank's persons.
Rank 0 prints ONE JSON line.

`dtype` is f16: the MFMA operand format whose outputs meet the north star's 1e-3 parity (tests/test_gpu_parity_fullsize.py; with
`--full` the line's `parity` object is measured in this very process against the CPU oracle on image 0 of the benchmark batch with
the benchmark weights).  bf16 operands run the same kernels ~4 % faster and are reported beside with `--full` (`other_precision`),
but miss 1e-3.

Nothing but the K forwards (and the collation) is inside the timed region.  A plain run stops there: set-up, W warm-up steps, the K
timed steps, the outputs of the last step if `--dump-outputs DIR` is given, the line.  Everything else is measured only with `--full`,
in separate passes after the timed region: the per-kernel hipEvent brackets that feed `roofline`, the inference mode, the SMPL-X layer
alone (`lbs`, BASELINE.json's second metric ms/person), the other precision, the other BASELINE configurations (`configs`), the
batch-1 latency, and the CPU baseline with the `parity` check.
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from multi_hmr_amd import Model, _lib, collate  # noqa: E402
import synthetic  # noqa: E402

PEAK_MFMA_TFLOPS = 2500.0     # bf16/f16 dense, /opt/skills/guides/MI355X_MICROARCH.md "Chip-level parameters"
PEAK_HBM_GBS = 8000.0         # HBM3E spec, same table (6.29 TB/s measured float4 copy)
DUMP_BUDGET = 64 * 2 ** 20    # --dump-outputs: bytes of array data in all
PARITY_KEYS = ["scores", "offset", "loc", "dist", "shape", "expression", "rotmat", "transl", "v3d", "j3d", "j2d"]
#: the other single-GPU BASELINE.json configurations: name, backbone, S, images, persons / image
OTHER_CONFIGS = [("cfg2 multiHMR_672_S", "dinov2_vits14", 672, 16, 8), ("cfg3 multiHMR_672_L", "dinov2_vitl14", 672, 32, 8),
                 ("cfg5 multiHMR_1288_L", "dinov2_vitl14", 1288, 8, 20)]


def flops_per_image(S, C, L, heads_depth=2, inner=256):
    """algorithmic FLOPs of one image (T = N + 1 real tokens, no padding)."""
    G = S // 14
    N, T = G * G, G * G + 1
    gemm = 2 * N * 588 * C + L * 24 * T * C * C + 2 * N * C * C + heads_depth * 2 * N * (C + 99) * 2 * inner
    attn = L * 4 * T * T * C
    return gemm, attn


def lbs_bytes(P, nb=10):
    """Algorithmic HBM bytes of one LBS launch: constants once + per-person in/out."""
    const = 10475 * 3 * 4 * (1 + nb + 10 + 486) + 55 * 3 * (nb + 11) * 4 + 10475 * 4 * 8
    return const + P * (764 + 10475 * 3 * 4 + 10475 * 2 * 4 + 127 * 5 * 4)


def lbs_bytes_shipped(P, Vp=10752, V=10475):
    """HBM bytes the SHIPPED layer has to move per launch: the f16 basis as packed (162 KiB per 48-vertex tile: high halves for the pose
    correctives, an f16 pair for the last 64 k) + the dense f16-pair skin weights (12 KiB per tile) + the fp32 template once, and per
    person the same inputs / outputs as lbs_bytes (the operand fragments the pose role leaves are L2-resident, not counted)."""
    tiles = Vp // 48
    const = tiles * (165888 + 12288) + 3 * Vp * 4
    return const + P * (764 + V * 3 * 4 + V * 2 * 4 + 127 * 5 * 4)


def lib_sha16():
    with open(_lib.LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def lib_source_hash():
    """Hash of the sources + flags the LOADED library was built from (compiled into it; the same on every machine)."""
    return _lib.lib().mhmr_source_hash().decode()


def pmc_summary():
    """The newest committed rocprofv3 PMC summary (tools/pmc_traffic.py -> profiles/r*_pmc.json).  Counters cannot be read from
    inside the timed process, so `traffic` comes from that file -- and only when it was measured on a library built from THE SAME
    SOURCES as the one running now (the summary records `mhmr_source_hash()`, which does not depend on the machine or the checkout
    path; older summaries carry the .so's own sha256 prefix); otherwise traffic is null."""
    best = None
    pdir = os.path.join(ROOT, "profiles")
    for name in sorted(os.listdir(pdir)) if os.path.isdir(pdir) else []:
        if name.endswith("_pmc.json"):
            try:
                with open(os.path.join(pdir, name)) as f:
                    d = json.load(f)
            except (OSError, ValueError):
                continue
            if d.get("_source_hash") == lib_source_hash() or ("_source_hash" not in d and d.get("_lib_sha16") == lib_sha16()):
                best = dict(d, _file=name)
    return best


def prof_window(kind):
    _lib.check(_lib.lib().mhmr_prof_enable(kind), "prof_enable")


def prof_collect():
    n, ms, work = C.c_int(0), C.c_double(0), C.c_double(0)
    _lib.check(_lib.lib().mhmr_prof_collect(C.byref(n), C.byref(ms), C.byref(work)), "prof_collect")
    _lib.lib().mhmr_prof_enable(-1)
    return n.value, ms.value, work.value


def dump_outputs(out, d):
    """--dump-outputs: the arrays the timed path returned in its last step, as DIR/<name>.npy in float32.  Above DUMP_BUDGET in all,
    every array keeps the same fixed, seeded sample of its leading rows (images for `scores`, persons for the rest), sized to fit."""
    arrs = {k: v.detach().float().cpu().numpy() for k, v in out.items() if torch.is_tensor(v) and not k.startswith("_")}
    total = sum(a.nbytes for a in arrs.values())
    os.makedirs(d, exist_ok=True)
    for k, a in sorted(arrs.items()):
        if total > DUMP_BUDGET and a.ndim and a.shape[0] > 1:
            n = max(1, a.shape[0] * DUMP_BUDGET // total)
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], n, replace=False))]
        np.save(os.path.join(d, k + ".npy"), np.ascontiguousarray(a))


def build_model(backbone, S, dtype, smplx_data, mean_params, dev):
    model = Model(backbone=backbone, img_size=S, smplx_data=smplx_data, mean_params=mean_params, precision=dtype)
    model.load_state_dict(synthetic.make_state_dict(backbone, S, seed=0, mean_params=mean_params), strict=True)
    return model.to(dev).eval()


def make_inputs(B, S, q, rank, dev):
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    x = torch.randn(B, 3, S, S, generator=g, device=dev)          # random, not zero-filled (DVFS, MICROARCH "DVFS give-back")
    K = synthetic.get_camera_K(S, B).to(dev)
    idx = tuple(t.to(dev) for t in synthetic.make_pinned_idx(B, S // 14, q, seed=rank))
    return x, K, idx


def time_steps(fn, steps, warmup, dev):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


class _StubModel:
    """MHMR_BENCH_STUB=1 (tests/test_bench_gloo.py): a CPU stand-in with the output contract of ``Model.forward(is_training=True)`` so that
    the N > 1 CONTROL FLOW of this file -- per-step asynchronous collation, the barrier + max-over-ranks clock, rank 0's extra passes
    against the other ranks' barrier, destroy_process_group -- runs under gloo without a GPU.  It measures nothing."""

    def __init__(self, G, V=32):
        self.G, self.V, self.calls = G, V, 0

    def _nsplit(self, B):
        return 1

    def __call__(self, x, idx=None, K=None, is_training=True):
        self.calls += 1
        B, P = x.shape[0], idx[0].shape[0]
        f = lambda *s: torch.full(s, float(self.calls), dtype=torch.float32)
        return {"scores": torch.rand(B, self.G, self.G, 1), "loc": f(P, 2), "transl": f(P, 3), "transl_pelvis": f(P, 1, 3), "rotvec": f(P, 53, 3),
                "expression": f(P, 10), "shape": f(P, 10), "j3d": f(P, 127, 3), "j2d": f(P, 127, 2), "v3d": f(P, self.V, 3)}


class _HostEvent:
    """torch.cuda.Event's interface on the host clock (stub mode)."""

    def __init__(self, enable_timing=True):
        self.t = 0.0

    def record(self):
        self.t = time.perf_counter()

    def elapsed_time(self, other):
        return 1e3 * (other.t - self.t)


def self_launch(n):
    """`python bench.py --gpus N` from a bare shell: start N ranks (one per GPU) of this same command under torch.distributed.run on a
    free local port and hand its exit code back.  More ranks than GPUs -> ONE JSON error line, exit code 2."""
    import socket
    import subprocess
    have = torch.cuda.device_count()
    if n > have and os.environ.get("MHMR_BENCH_STUB") != "1":
        print(json.dumps({"error": f"--gpus {n} requested, {have} GPU(s) visible on this node", "n_gpus": n, "gpus_visible": have,
                          "metric": "images/sec (whole node)", "value": None}))
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="f16", choices=["bf16", "f16"])
    ap.add_argument("--backbone", default="dinov2_vitl14")
    ap.add_argument("--img-size", type=int, default=896)
    ap.add_argument("--batch", type=int, default=32, help="images per GPU")
    ap.add_argument("--persons", type=int, default=8, help="pinned detections per image")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs as DIR/<name>.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the side measurements: roofline passes, inference mode, LBS, other precision, "
                         "other configs, batch-1 latency, CPU baseline + parity (a plain run times the steps and prints the line)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU oracle legs (cpu_baseline AND parity)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the roofline side measurements, the other configs and the other precision")
    ap.add_argument("--only-latency", action="store_true", help="print the latency_b1 object alone (A/B sessions)")
    ap.add_argument("--only-headline-kernels", action="store_true",
                    help="with --full, profiling runs (rocprofv3 --pmc): the headline forward and its roofline passes only, so that per-kernel "
                         "averages are not mixed with the other configurations' shapes")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.only_latency:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        print(json.dumps(latency_b1(args.dtype, synthetic.make_smplx_data(0), synthetic.make_mean_params(0), dev)))
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    stub = os.environ.get("MHMR_BENCH_STUB") == "1"         # CPU + gloo + _StubModel: the control flow only (tests/test_bench_gloo.py)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if stub:
            torch.distributed.init_process_group("gloo")
        else:
            torch.cuda.set_device(local)
            torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local))
    ranks_seen = 1
    if world > 1:
        # the group really spans `world` processes: an all-reduce of ones (a silent group-of-one fallback would report N x one GPU's rate)
        one = torch.ones(1, device=torch.device("cpu") if stub else torch.device("cuda", local))
        torch.distributed.all_reduce(one)
        ranks_seen = int(one.item())
        if ranks_seen != world:
            if rank == 0:
                print(json.dumps({"error": f"all_reduce of ones over the process group gave {ranks_seen}, expected {world}", "n_gpus": args.gpus}))
            sys.exit(2)
    if world != args.gpus:
        if rank == 0:
            print(json.dumps({"error": f"--gpus {args.gpus} but WORLD_SIZE={world}", "n_gpus": args.gpus}))
        sys.exit(2)
    dev = torch.device("cpu") if stub else torch.device("cuda", local)
    if not stub:
        torch.cuda.set_device(dev)
    Event = _HostEvent if stub else torch.cuda.Event
    sync = (lambda: None) if stub else (lambda: torch.cuda.synchronize(dev))

    S, B, q = args.img_size, args.batch, args.persons
    cfg = synthetic.VIT_CFG[args.backbone]
    if stub:
        smplx_data = mean_params = None
        model = _StubModel(S // 14)
        x, K = torch.zeros(B, 3, 1, 1), torch.zeros(B, 3, 3)
        idx = synthetic.make_pinned_idx(B, S // 14, q, seed=rank)
    else:
        smplx_data, mean_params = synthetic.make_smplx_data(0), synthetic.make_mean_params(0)
        model = build_model(args.backbone, S, args.dtype, smplx_data, mean_params, dev)
        x, K, idx = make_inputs(B, S, q, rank, dev)

    pending = []          # N > 1: the collation of step i travels over xGMI while step i + 1 computes (waited one step later)
    compute_ev = []       # N > 1: hipEvent pairs around the forward alone (separates compute from exposed collation)
    # a real caller hands in a NEW idx tuple at every step: one set of tensor objects per step, made before the clock starts
    # (the forward derives everything it needs from idx on the device, every step -- nothing is remembered between steps)
    idx_steps = [tuple(t.clone() for t in idx) for _ in range(args.warmup + args.steps)]
    step_no = [0]

    def step():
        if world > 1:
            e0, e1 = Event(enable_timing=True), Event(enable_timing=True)
            e0.record()
        idx = idx_steps[step_no[0] % len(idx_steps)]
        step_no[0] += 1
        out = model(x, idx=idx, K=K, is_training=True)
        if world > 1:
            e1.record()
            compute_ev.append((e0, e1))
            out["scores"] = out["scores"][idx[0], idx[1], idx[2], 0]      # per-person score slot of the record
            pending.append(collate.allgather_persons_async(out, capacity=B * q, image_offset=rank * B, image_index=idx[0]))
            if len(pending) > 1:
                pending.pop(0).wait()
        return out

    def drain():
        while pending:
            pending.pop(0).wait()

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        sync()

    for _ in range(args.warmup):
        step()
    drain()
    barrier()
    compute_ev.clear()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out_last = step()
    drain()               # every step's persons are collated on every rank inside the timed region
    barrier()
    dt = time.perf_counter() - t0
    if rank == 0 and args.dump_outputs:
        dump_outputs(out_last, args.dump_outputs)
    compute_ms = sum(a.elapsed_time(b) for a, b in compute_ev) if compute_ev else None
    if world > 1:
        t = torch.tensor([dt, compute_ms], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt, compute_ms = float(t[0].item()), float(t[1].item())

    gemm_fl, attn_fl = flops_per_image(S, cfg["embed_dim"], cfg["depth"])
    ms_step = 1e3 * dt / args.steps
    value = world * B * args.steps / dt
    size = args.backbone[-3].upper()
    result = {
        "metric": f"images/sec (whole node) ViT-{size} {S}x{S} bs{B}", "value": round(value, 3), "unit": "images/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic (seeded N(0,1) images, random-init weights, synthetic SMPL-X)",
        "config": {"workload": f"multiHMR_{S}_{size} full forward: {args.backbone} {S}x{S}, {B} images/GPU, "
                               f"{q} pinned persons/image -> HPH (depth 2) -> SMPL-X LBS; image-sharded x{world}",
                   "global_batch": world * B, "parallelism": f"dp{world} (images)"},
        "mfma_utilisation_whole_forward": round((gemm_fl + attn_fl) * B * args.steps / dt / 1e12 / PEAK_MFMA_TFLOPS, 4),
        "lib_sha16": None if stub else lib_sha16(), "source_hash": None if stub else lib_source_hash(),
        "backbone_image_blocks": model._nsplit(B),
        # what Model(precision=...) resolved to at pack time ("auto" -> "f16" | "f16x3" from the weights; the bench asks for args.dtype)
        "precision_resolved": None if stub else model.packed_precision,
    }
    if world > 1:
        result["multi_gpu"] = {"max_rank_compute_ms_per_step": round(compute_ms / args.steps, 3),
                               "exposed_collation_ms_per_step": round(ms_step - compute_ms / args.steps, 3),
                               "collation": "async RCCL all_gather of counts + padded person records, overlapped with the next step",
                               "ranks_verified_by_all_reduce": ranks_seen}

    if stub:
        result["stub"] = True
    if rank == 0 and stub and args.full:
        # stub mode: rank 0's extra passes are a few more calls of the stand-in (the other ranks wait at the barrier below)
        for _ in range(4):
            model(x, idx=idx, K=K, is_training=True)
    if rank == 0 and not stub and args.full:
        # ---- profiled passes, OUTSIDE the timed region: hipEvent brackets around every GEMM / attention launch ----
        # `launches`, `algorithmic_flops_per_launch`, `share_of_step` are PER FORWARD (the brackets run over `profiled_forwards` forwards)
        reps = 2
        prof_window(0)
        for _ in range(reps):
            model(x, idx=idx, K=K, is_training=True)
        n_gemm, ms_gemm, work_gemm = prof_collect()
        gemm_tf = gemm_fl * B * reps / (ms_gemm * 1e-3) / 1e12 if ms_gemm > 0 else 0.0
        pmc = pmc_summary()
        pmc_src = ("profiles/" + pmc["_file"]) if pmc else None
        result["roofline"] = {
            "kernel": "gemm256_kernel (persistent 256x256x64 8-phase, v_mfma_f32_16x16x32; all ViT linears + heads)", "bound": "mfma",
            "achieved": round(gemm_tf, 1), "peak": PEAK_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(gemm_tf / PEAK_MFMA_TFLOPS, 4),
            "traffic": pmc.get("_gemm_avg_bytes_per_launch") if pmc else None,
            "traffic_source": pmc_src, "traffic_note": "rocprofv3 --pmc FETCH_SIZE + WRITE_SIZE per launch, committed summary of a run of these "
                                                       "same sources (matched by source_hash); null when no summary matches",
            "launches": n_gemm // reps, "profiled_forwards": reps,
            "avg_launch_ms": round(ms_gemm / max(n_gemm, 1), 4), "algorithmic_flops_per_launch": round(gemm_fl * B * reps / max(n_gemm, 1)),
            "share_of_step": round(ms_gemm / reps / ms_step, 3),
            # what the matrix pipe executed in those launches: 2 M N K as launched, i.e. with the low-half weight passes (k doubled
            # for V and proj of blocks 0-11) and the padded rows of the 128-row kernels; `achieved` stays the ALGORITHMIC rate
            "executed": round(work_gemm / (ms_gemm * 1e-3) / 1e12, 1) if ms_gemm > 0 else 0.0}
        prof_window(1)
        for _ in range(reps):
            model(x, idx=idx, K=K, is_training=True)
        n_a, ms_a, _ = prof_collect()
        att_tf = attn_fl * B * reps / (ms_a * 1e-3) / 1e12 if ms_a > 0 else 0.0
        result["roofline_attention"] = {
            "kernel": "attn16_kernel (flash, d=64, v_mfma_f32_16x16x32; reference level in the accumulator init)", "bound": "mfma", "achieved": round(att_tf, 1),
            "peak": PEAK_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(att_tf / PEAK_MFMA_TFLOPS, 4),
            "traffic": pmc.get("_attention_bytes_per_call") if pmc else None, "traffic_source": pmc_src,
            "launches": n_a // reps, "profiled_forwards": reps,
            "avg_launch_ms": round(ms_a / max(n_a, 1), 4), "share_of_step": round(ms_a / reps / ms_step, 3)}
    extras = args.full and rank == 0 and not stub and not args.no_extras and not args.only_headline_kernels
    if extras and world == 1:
        result["inference_mode"] = inference_bench(model, x, K, out_last, B, q, dev, steps=min(args.steps, 20))
    if extras:
        result["lbs"] = lbs_bench(model, dev, P=160)
        small = {p: lbs_bench(model, dev, P=p) for p in (20, 1)}
        # BASELINE.json's second metric at the three person counts of SURVEY 8(d), top level
        result["ms_per_person_lbs"] = {"P=160": result["lbs"]["ms_per_person"], "P=20": small[20]["ms_per_person"], "P=1": small[1]["ms_per_person"]}
        result["lbs_small_batches"] = {f"P={p}": {"ms_per_person": v["ms_per_person"], "layer_ms": v["layer_ms"]} for p, v in small.items()}
    if world > 1:
        torch.distributed.barrier()

    if args.full and rank == 0 and world == 1 and not stub and not args.no_cpu_baseline:
        result["cpu_baseline"], result["parity"] = cpu_baseline_and_parity(args, smplx_data, mean_params, model, x, K, idx, out_last)
    if extras and world == 1:
        # release the headline model's workspace before the other configurations
        del model, out_last
        torch.cuda.empty_cache()
        other = "bf16" if args.dtype == "f16" else "f16"
        m2 = build_model(args.backbone, S, other, smplx_data, mean_params, dev)
        dt2 = time_steps(lambda: m2(x, idx=idx, K=K, is_training=True), 10, 3, dev)
        result["other_precision"] = {"dtype": other, "value": round(B * 10 / dt2, 2), "unit": "images/s", "ms_per_step": round(1e3 * dt2 / 10, 3),
                                     "mfma_utilisation_whole_forward": round((gemm_fl + attn_fl) * B * 10 / dt2 / 1e12 / PEAK_MFMA_TFLOPS, 4),
                                     "note": "same kernels; bf16 operands miss the 1e-3 parity contract (tests/test_gpu_parity_fullsize.py)"
                                     if other == "bf16" else "the precision that meets 1e-3 parity"}
        del m2
        torch.cuda.empty_cache()
        result["configs"] = [other_config(name, bb, s, b, p, args.dtype, smplx_data, mean_params, dev) for name, bb, s, b, p in OTHER_CONFIGS]
        # the ONE runtime the reference publishes (README.md:87-93, measured at demo.py:333-338): batch-1 forward_model latency
        result["latency_b1"] = latency_b1(args.dtype, smplx_data, mean_params, dev)
    if rank == 0:
        print(json.dumps(result))
    if world > 1:
        torch.distributed.destroy_process_group()


#: reference README.md:87-91: per-image forward_model runtime, batch 1, fp16 autocast, on a V100 (ms)
REFERENCE_V100_MS = {"multiHMR_896_L": 126.0, "multiHMR_672_L": 74.0, "multiHMR_672_B": 43.0, "multiHMR_672_S": 29.0}
LATENCY_MODELS = [("multiHMR_896_L", "dinov2_vitl14", 896), ("multiHMR_672_L", "dinov2_vitl14", 672), ("multiHMR_672_B", "dinov2_vitb14", 672),
                  ("multiHMR_672_S", "dinov2_vits14", 672)]


def latency_b1(dtype, smplx_data, mean_params, dev, reps=30, persons=4):
    """Batch-1 latency of ``demo.forward_model``'s path (reference demo.py:108-126, timed at demo.py:333-338 and published in README.md:
    87-93 for a V100): ONE image resident in HBM, inference mode (detection + NMS on the model's own scores, HPH + SMPL-X for the
    detected persons, the person-dict list), no batching.  `ms` = host wall clock around the call (it ends with the person-count
    read-back, so the host clock is exact), `gpu_ms` = hipEvents around the same call on its stream; medians of `reps` calls."""
    import torch.nn.functional as F
    from multi_hmr_amd import demo
    out = {}
    for name, backbone, S in LATENCY_MODELS:
        model = build_model(backbone, S, dtype, smplx_data, mean_params, dev)
        x, K, idx = make_inputs(1, S, persons, 0, dev)
        s = model(x, idx=idx, K=K, is_training=True)["scores"][..., 0]
        m = F.max_pool2d(s[:, None], 3, stride=1, padding=1)[:, 0]
        surv = torch.sort(s[m == s], descending=True).values
        n = min(persons, surv.numel() - 1)
        thr = float(0.5 * (surv[n - 1] + surv[n]))
        def clock(run):
            for _ in range(5):
                humans = run()
            torch.cuda.synchronize(dev)
            wall, gpu = [], []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                run()
                e1.record()
                wall.append(time.perf_counter() - t0)
                e1.synchronize()
                gpu.append(e0.elapsed_time(e1))
            return humans, wall, gpu

        humans, wall, gpu = clock(lambda: demo.forward_model(model, x, K, det_thresh=thr, nms_kernel_size=3))
        # the same call replayed from a hipGraph (multi_hmr_amd/graphed.py: recorded on first use; same kernels, same results).  An
        # auxiliary leg: if the recording fails on some box the line says so instead of losing the eager numbers.
        graph = {}
        try:
            hg, wg, gg = clock(lambda: demo.forward_model(model, x, K, det_thresh=thr, nms_kernel_size=3, use_graph=True))
            same = len(hg) == len(humans) and all(torch.equal(p[k], q[k]) for p, q in zip(hg, humans) for k in p)
            graph = {"graph_ms": round(1e3 * sorted(wg)[len(wg) // 2], 3), "graph_gpu_ms": round(sorted(gg)[len(gg) // 2], 3),
                     "graph_min_ms": round(1e3 * min(wg), 3), "graph_equals_eager": bool(same)}
            # the replay alone (no copy into the graph's input, no clones of its outputs) at the eager call's own person capacity
            from multi_hmr_amd.graphed import GraphedForward
            gf = GraphedForward(model, 1, thr, 3, capacity=model._person_cap.get(1, 16))
            gf.x.copy_(x)
            gf.K.copy_(K)
            _, wr, _ = clock(gf.replay)
            graph["graph_replay_ms"] = round(1e3 * sorted(wr)[len(wr) // 2], 3)
            del gf
        except Exception as e:                                          # noqa: BLE001
            graph = {"graph_ms": None, "graph_error": f"{type(e).__name__}: {e}"[:200]}
        cfg = synthetic.VIT_CFG[backbone]
        gemm_fl, attn_fl = flops_per_image(S, cfg["embed_dim"], cfg["depth"])
        med = sorted(wall)[len(wall) // 2]
        out[name] = {"ms": round(1e3 * med, 3), "gpu_ms": round(sorted(gpu)[len(gpu) // 2], 3), "min_ms": round(1e3 * min(wall), 3),
                     "persons": len(humans), "reps": reps,
                     "mfma_utilisation_whole_forward": round((gemm_fl + attn_fl) / med / 1e12 / PEAK_MFMA_TFLOPS, 4),
                     "reference_v100_fp16_ms": REFERENCE_V100_MS[name], "speedup_vs_reference_v100": round(REFERENCE_V100_MS[name] / (1e3 * med), 1)}
        out[name].update(graph)
        del model
        torch.cuda.empty_cache()
    out["note"] = ("batch 1, is_training=False through demo.forward_model, image already in HBM, seeded random weights; ms = the eager forward, "
                   "graph_ms = forward_model(use_graph=True), the same launches replayed from a hipGraph; the reference's figures are "
                   "README.md:87-91 (V100, fp16 autocast) -- other hardware, quoted for orientation, not a baseline this line is scored against")
    return out


def other_config(name, backbone, S, B, q, dtype, smplx_data, mean_params, dev, steps=10, warmup=3):
    """One of the other single-GPU BASELINE.json configurations: whole forward, same definition of a step."""
    model = build_model(backbone, S, dtype, smplx_data, mean_params, dev)
    x, K, idx = make_inputs(B, S, q, 0, dev)
    dt = time_steps(lambda: model(x, idx=idx, K=K, is_training=True), steps, warmup, dev)
    cfg = synthetic.VIT_CFG[backbone]
    gemm_fl, attn_fl = flops_per_image(S, cfg["embed_dim"], cfg["depth"])
    out = {"config": name, "workload": f"{backbone} {S}x{S}, {B} images, {q} persons/image", "dtype": dtype, "value": round(B * steps / dt, 2),
           "unit": "images/s", "ms_per_step": round(1e3 * dt / steps, 3), "steps": steps,
           "mfma_utilisation_whole_forward": round((gemm_fl + attn_fl) * B * steps / dt / 1e12 / PEAK_MFMA_TFLOPS, 4)}
    del model
    torch.cuda.empty_cache()
    return out


def inference_bench(model, x, K, out_train, B, q, dev, steps=20, warmup=3):
    """The path `demo.forward_model` drives (reference demo.py:108-126 -> model.py:141-149, 329-347): is_training=False -- NMS + threshold
    on the scores, the one host synchronisation for the person count, ordered compaction, HPH + SMPL-X for the detected persons, the
    per-person dict list.  The threshold is placed in the gap below the (B * q)-th largest NMS-surviving score of the benchmark batch
    (about q persons per image, as in the headline), and the same detections are then pinned through the training hook to price the
    host-side share of the inference mode (count sync + Python dict loop)."""
    import torch.nn.functional as F
    s = out_train["scores"][..., 0]                                        # [B, G, G]
    m = F.max_pool2d(s[:, None], 3, stride=1, padding=1)[:, 0]
    surv = torch.sort(s[m == s], descending=True).values
    n = min(B * q, surv.numel() - 1)
    thr = float(0.5 * (surv[n - 1] + surv[n]))
    run = lambda: model(x, K=K, det_thresh=thr, nms_kernel_size=3)
    persons = run()
    dt = time_steps(run, steps, warmup, dev)
    # per-step clocks as well (every inference step ends with the person-count read-back, so a host clock per step is exact): the
    # median is insensitive to the occasional Python garbage-collection pass that the ~3 000 tensor views of a person list provoke
    per = []
    for _ in range(steps):
        t0 = time.perf_counter()
        run()
        per.append(time.perf_counter() - t0)
    med = sorted(per)[len(per) // 2]
    keep = (m == s) & (s >= thr)
    idx = tuple(torch.where(keep)) + (torch.zeros(int(keep.sum()), dtype=torch.long, device=dev),)
    dt_hook = time_steps(lambda: model(x, idx=idx, K=K, is_training=True), steps, warmup, dev)
    gemm_fl, attn_fl = flops_per_image(model.img_size, model.embed_dim, len(model.backbone.encoder.blocks))
    return {"value": round(B * steps / dt, 2), "unit": "images/s", "ms_per_step": round(1e3 * dt / steps, 3), "steps": steps,
            "mfma_utilisation_whole_forward": round((gemm_fl + attn_fl) * B * steps / dt / 1e12 / PEAK_MFMA_TFLOPS, 4),
            "persons_per_step": len(persons), "det_thresh": thr, "nms_kernel_size": 3,
            "training_hook_same_detections_ms_per_step": round(1e3 * dt_hook / steps, 3),
            "host_side_share_ms_per_step": round(1e3 * (dt - dt_hook) / steps, 3),
            "median_step_ms": round(1e3 * med, 3), "host_side_share_ms_median_step": round(1e3 * (med - dt_hook / steps), 3),
            "note": "is_training=False: detection, heads enqueued for a person-row capacity, ONE D2H person-count read after the last launch, "
                    "per-person dict list; host_side_share = inference-mode step minus the training-hook step pinned to the same detections"}


def lbs_bench(model, dev, P=160, iters=20):
    """ms/person of the SMPL-X layer alone (BASELINE.json second metric; config #5 = 8 images x 20 persons)."""
    L = _lib.lib()
    Pk = model._packed
    lb, cs = Pk["lbs"], Pk["lbs_struct"]
    g = torch.Generator(device=dev).manual_seed(5)
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    pose = 0.3 * torch.randn(P, 53, 3, generator=g, device=dev)
    shape, expr = torch.randn(P, 10, generator=g, device=dev), torch.randn(P, 10, generator=g, device=dev)
    loc, dist = 1288 * torch.rand(P, 2, generator=g, device=dev), 2 + 6 * torch.rand(P, 1, generator=g, device=dev)
    K = synthetic.get_camera_K(1288, 8).to(dev)
    det_b = torch.arange(P, device=dev, dtype=torch.int32) // max(1, (P + 7) // 8)
    V = lb["V"]
    bufs = [f((P + 15) // 16 * 16, lb["Kb"]), f((P + 15) // 16 * 16, 768), f(P, 24), f(P, V, 3), f(P, V, 2), f(P, 127, 3), f(P, 127, 2), f(P, 3)]
    stream = torch.cuda.current_stream(dev).cuda_stream

    sync = Pk["lbs_sync"]
    fused = os.environ.get("MHMR_LBS_FUSED") == "1"

    def run():      # the entry Model.forward calls: pose kernel + vertex kernel (MHMR_LBS_FUSED=1: the one-launch form, slower on this chip)
        a = [C.byref(cs), pose.data_ptr(), shape.data_ptr(), expr.data_ptr(), loc.data_ptr(), dist.data_ptr(), K.data_ptr(), det_b.data_ptr(), P] + \
            [b.data_ptr() for b in bufs]
        _lib.check(L.mhmr_lbs_forward_fused(*a, sync.data_ptr(), stream) if fused else L.mhmr_lbs_forward(*a, stream), "lbs")
    for _ in range(3):
        run()
    torch.cuda.synchronize(dev)
    prof_window(2)
    t0 = time.perf_counter()
    for _ in range(iters):
        run()
    torch.cuda.synchronize(dev)
    wall = (time.perf_counter() - t0) / iters
    n, ms, _ = prof_collect()
    avg = ms / max(n, 1) * 1e-3
    gbs = lbs_bytes(P) / avg / 1e9 if avg > 0 else 0.0
    gbs_s = lbs_bytes_shipped(P) / avg / 1e9 if avg > 0 else 0.0
    pmc = pmc_summary()
    kern = (pmc or {}).get("lbs_fused_kernel") or (pmc or {}).get("lbs_vertex_kernel") or {}
    return {"persons": P, "ms_per_person": round(1e3 * wall / P, 6), "layer_ms": round(1e3 * wall, 4),
            "roofline": {"kernel": "lbs_fused_kernel (one launch: pose role + vertex role)" if os.environ.get("MHMR_LBS_FUSED") == "1" else "lbs_vertex_kernel",
                         "bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                         "frac": round(gbs / PEAK_HBM_GBS, 4),
                         "traffic": kern.get("total_bytes_per_launch") if P == 160 else None,
                         "traffic_source": ("profiles/" + pmc["_file"]) if (pmc and P == 160 and kern) else None,
                         "algorithmic_bytes": lbs_bytes(P), "avg_launch_ms": round(avg * 1e3, 4),
                         # SURVEY 8(d)'s figure prices the reference's fp32 constants (66.4 MB); the shipped layer keeps them as f16
                         # (40 MB): against the bytes it actually has to move the same launch reads as
                         "shipped_bytes": lbs_bytes_shipped(P), "achieved_shipped": round(gbs_s, 1), "frac_shipped": round(gbs_s / PEAK_HBM_GBS, 4),
                         "note": "avg_launch_ms brackets the vertex kernel (the pose kernel runs in front of it; layer_ms is both + the gap)"}}


def cpu_model_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def cpu_baseline_and_parity(args, smplx_data, mean_params, model, x, K, idx, out_gpu):
    """The oracle (reference algorithm restated, CPU fp32, all host cores) on a bounded sample of the same workload: image 0 of
    the benchmark batch, same weights, same pinned persons.  The first (warm-up) run doubles as the parity check of the GPU
    result for that image; three more runs are timed (median)."""
    from oracle.multihmr_ref import OracleModel
    S, q = args.img_size, args.persons
    sd = synthetic.make_state_dict(args.backbone, S, seed=0, mean_params=mean_params)
    ref = OracleModel(sd, smplx_data, backbone=args.backbone, img_size=S)
    sel = (idx[0] == 0)
    idx0 = tuple(t[sel].cpu() for t in idx)
    x0, K0 = x[:1].cpu(), K[:1].cpu()
    t0 = time.perf_counter()
    o = ref.forward(x0, idx=idx0, K=K0, is_training=True)          # warm-up + parity reference
    warm = time.perf_counter() - t0
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref.forward(x0, idx=idx0, K=K0, is_training=True)
        times.append(time.perf_counter() - t0)
    med = sorted(times)[1]
    rel = lambda a, b: float(np.linalg.norm(a.double().numpy() - b.double().numpy()) / max(np.linalg.norm(b.double().numpy()), 1e-30))
    per = {}
    for k in PARITY_KEYS:
        g = out_gpu[k][0:1] if k == "scores" else out_gpu[k][sel]
        r = o[k][0:1] if k == "scores" else o[k]
        per[k] = rel(g.cpu(), r)
    vmm = 1e3 * float((out_gpu["v3d"][sel].cpu() - o["v3d"]).abs().max())
    parity = {"dtype": args.dtype, "reference": "CPU fp32 oracle (reference model.py semantics), image 0 of the benchmark batch, benchmark weights",
              "tolerance": 1e-3, "worst_rel_l2": max(per.values()), "max_vertex_mm": round(vmm, 4), "rel_l2": {k: float(f"{v:.3e}") for k, v in per.items()},
              "persons": int(sel.sum())}
    base = {"value": round(1.0 / med, 4), "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port", "cpu": cpu_model_name(),
            "torch": torch.__version__,
            "sample": f"1 image {S}x{S} {args.backbone}, {q} persons, full forward incl. HPH + LBS, fp32 torch CPU; 1 warm-up ({warm:.1f} s) + 3 "
                      f"timed runs, median {med:.1f} s (min {min(times):.1f}, max {max(times):.1f})"}
    return base, parity


if __name__ == "__main__":
    main()
