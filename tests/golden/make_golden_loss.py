"""Regenerate tests/golden/loss_ref.npz: the REFERENCE's own loss (its loss.py, imported from a checkout given on the command line)
on one seeded case of tests/loss_oracle.make_inputs, CPU fp32 with autograd.  Generation time only -- no test imports this file or the
reference; the tests regenerate the inputs from the stored seed and compare this record with the fp64 statement and the GPU path.

    python tests/golden/make_golden_loss.py /path/to/multi-hmr

Stored: the case, the eleven values, per gradient its fp64 sum and sum of magnitudes plus its first SLICE values, and the defaults of
Loss.add_specific_args as a list of (name, value) in the parser's order.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import loss_oracle as lo  # noqa: E402

CASE = dict(seed=20260117, P=7, V=10475, J=127, B=2, G=5, nb_hat=10, nb_gt=11, img_size=224.0, epoch=10)
SLICE = 64
GRAD_KEYS = ("scores", "offset", "rotmat", "shape", "dist_postprocessed", "transl", "transl_pelvis", "j3d", "v3d", "j2d", "v2d")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="checkout of the reference project (the directory that holds loss.py)")
    ap.add_argument("--out", default=os.path.join(HERE, "loss_ref.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_loss", os.path.join(a.reference, "loss.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    parser = ref.Loss.add_specific_args(argparse.ArgumentParser(add_help=False))
    args = parser.parse_args([])
    defaults = [(act.dest, float(act.default)) for act in parser._actions if act.dest != "help"]
    c = CASE
    h, y = lo.make_inputs(c["seed"], c["P"], c["V"], c["J"], c["B"], c["G"], c["nb_hat"], c["nb_gt"], c["img_size"])
    th = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in h.items()}      # transl_pelvis: a leaf of its own
    ty = {k: torch.from_numpy(v) for k, v in y.items()}
    total, d = ref.Loss(args)(th, ty, epoch=c["epoch"], img_size=c["img_size"])
    total.backward()
    rec = dict(case_keys=np.array(list(c)), case_values=np.array([float(v) for v in c.values()]),
               values=np.array([float(d[k].detach()) for k in lo.KEYS], dtype=np.float32), value_keys=np.array(lo.KEYS),
               default_names=np.array([n for n, _ in defaults]), default_values=np.array([v for _, v in defaults]))
    for k in GRAD_KEYS:
        g = th[k].grad.numpy().astype(np.float64).reshape(-1)
        rec["gsum_" + k] = np.array([g.sum(), np.abs(g).sum()])
        rec["gslice_" + k] = th[k].grad.numpy().reshape(-1)[:SLICE].copy()
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes;", {k: float(d[k].detach()) for k in lo.KEYS})


if __name__ == "__main__":
    main()
