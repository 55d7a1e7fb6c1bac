"""Time the optimiser step for the whole model: ViT-L 896^2, f16, gradients already in place.  One process, one
model, two optimisers over the same parameters and the same gradients, alternating in every repetition after warm-up; device events and
medians, plus the host's wall time to issue each form (before any synchronisation).
  parent      torch.optim.Adam.step() + Model.repack_heads() + Model.repack_backbone()
  model_adam  ModelAdam.step()  (one mhmr_adam_step + one mhmr_vit_repack)
at two configurations: train_backbone_(24).train_embeddings_() and train_backbone_(4); heads and detector trained in both.  The bytes the
new step moves come from its two tables (multi_hmr_amd.optim.table_bytes with the jobs); the fraction of the HBM rate is bytes / median
time / 8 TB/s.  After the timing, one more ModelAdam.step() is compared with repack_backbone() on the same parameters: how many packed
elements differ (only fixed-order fp64 sums may, in the last bit).
  python tools/model_adam_bench.py [--reps 7] [--warmup 2] [--backbone dinov2_vitl14] [--size 896]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import synthetic  # noqa: E402
from multi_hmr_amd import Model, ModelAdam  # noqa: E402
from multi_hmr_amd.optim import table_bytes  # noqa: E402
from eval_bench import DEV, report  # noqa: E402
from train_step_bench import HBM_BYTES_PER_S, timed  # noqa: E402


def main(a):
    S = a.size
    smplx_data, mean_params = synthetic.make_smplx_data(0), synthetic.make_mean_params(0)
    m = Model(backbone=a.backbone, img_size=S, smplx_data=smplx_data, mean_params=mean_params, precision="f16")
    m.load_state_dict(synthetic.make_state_dict(a.backbone, S, seed=0, mean_params=mean_params), strict=True)
    m = m.to(DEV).eval().train_heads_(True).train_detection_(True)
    L = len(m.backbone.encoder.blocks)
    m._packed_for(torch.device(DEV))                      # the pack both forms rewrite
    med = lambda v: float(np.median(v))
    lines = []
    for n, embed in ((L, True), (min(4, L), False)):
        m.train_backbone_(L, flag=False).train_embeddings_(False)
        m.train_backbone_(n).train_embeddings_(embed)
        params = m.heads_parameters() + m.detection_parameters() + m.backbone_parameters(n) + (m.embedding_parameters() if embed else [])
        g = torch.Generator(device=DEV).manual_seed(11)
        for p in params:
            p.grad = 1e-3 * torch.randn(p.shape, generator=g, device=DEV)
        opt_t, opt_m = torch.optim.Adam(params, lr=1e-7), ModelAdam(m, lr=1e-7)

        def parent():
            opt_t.step()
            m.repack_heads()
            m.repack_backbone()
        ms, host = timed({"parent": parent, "model_adam": opt_m.step}, a)
        # the packed encoder after one more ModelAdam.step() against repack_backbone() on the same parameters: the fixed-order fp64 sums may
        # differ in the last bit, nothing else may differ at all
        opt_m.step()
        v = m._packed["vit"]
        packed = {("embed", k): t for k, t in v["embed_t"].items()}
        for l in range(L - n, L):
            packed.update({(l, k): t for k, t in v["block_t"][l].items() if t is not None})
        mine = {k: t.clone() for k, t in packed.items()}
        m.repack_backbone()
        fixed = [k for k in packed if k[1] in ("qkv_b", "fc1_b", "qkv_colsum", "fc1_colsum", "pos", "cls_pos0")]
        differ = {k: int((mine[k] != packed[k]).sum()) for k in packed}
        last_bit = dict(fixed_order_elements=int(sum(packed[k].numel() for k in fixed)), fixed_order_differing=int(sum(differ[k] for k in fixed)),
                        other_elements=int(sum(t.numel() for k, t in packed.items() if k not in fixed)),
                        other_differing=int(sum(d for k, d in differ.items() if k not in fixed)))
        del mine
        tab = opt_m._table
        nbytes = table_bytes(tab["host"], tab["jobs_host"][:tab["njobs"]])
        t = med(ms["model_adam"])
        lines.append(report(f"optimiser_step_train_backbone_{n}" + ("_with_embeddings" if embed else ""), ms, dict(
            backbone=a.backbone, size=S, dtype=m.packed_precision, blocks=n, embeddings=embed, parameters=len(params),
            elements=int(sum(p.numel() for p in params)), host_issue_ms={k: round(med(v), 4) for k, v in host.items()},
            median_ratio_parent_over_model_adam=round(med(ms["parent"]) / t, 3),
            model_adam_faster_in_every_repetition=bool(max(ms["model_adam"]) < min(ms["parent"])),
            model_adam_bytes=nbytes, adam_segments=len(tab["rows"]), pack_jobs=tab["njobs"],
            against_repack_backbone=last_bit, model_adam_fraction_of_hbm=round(nbytes / (t * 1e-3) / HBM_BYTES_PER_S, 4),
            note="gradients in place before the first event; parent = torch.optim.Adam.step() + repack_heads() + repack_backbone()")))
        for p in params:
            p.grad = None
        del opt_t, opt_m
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("# tools/model_adam_bench.py: torch.optim.Adam.step() + repack_heads() + repack_backbone() against ModelAdam.step(), "
                 "interleaved, gradients in place\n")
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--backbone", default="dinov2_vitl14")
    ap.add_argument("--size", type=int, default=896)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_adam_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("model_adam_bench measures on the GPU; there is none here")
    main(a)
