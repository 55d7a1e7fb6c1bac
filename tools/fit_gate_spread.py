"""CPU only: how far two legitimate fp32 evaluations of the keypoint fit's loop lie from the fp64 one, and what a real defect costs --
the figures behind the gate of tests/test_gpu_fit.py::test_loop.  Writes profiles/fit_tests.txt.

The recovery scene of tests/fit_oracle.py (L2, zero priors, every joint given), P = 3, steps = 5 and 30, seeds 0 .. 7:
  y32     the oracle in float32
  y32p    the same with the body's vertices in a permuted order: the same function, other fp32 sums (J_regressor . v, the skinning)
  defect  the fp64 oracle with the recentring's term dropped from the GRADIENT (fit_oracle.energy(recentre="detach"))
each as the trace distance max_t |E[t] - E64[t]| / E64[0] to the fp64 oracle.
  python tools/fit_gate_spread.py [--seeds 8]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import fit_oracle as fo  # noqa: E402
import gt_oracle as go  # noqa: E402
import synthetic  # noqa: E402

S, NB, P, LR, SIGMA = 224, 10, 3, 0.01, 1.0


def permuted(data, seed=1):
    """The same body with its vertices renumbered by a seeded permutation -> (data, picked-vertex ids)."""
    V = np.asarray(data["v_template"]).shape[0]
    perm = np.random.RandomState(seed).permutation(V)          # new vertex i = old vertex perm[i]
    inv = np.argsort(perm)
    out = dict(data)
    out["v_template"], out["shapedirs"], out["weights"] = np.asarray(data["v_template"])[perm], np.asarray(data["shapedirs"])[perm], np.asarray(data["weights"])[perm]
    pd = np.asarray(data["posedirs"])
    out["posedirs"] = pd.reshape(V, 3, -1)[perm].reshape(pd.shape)
    out["J_regressor"] = np.asarray(data["J_regressor"])[:, perm]
    out["f"] = inv[np.asarray(data["f"], dtype=np.int64)]
    return out, [int(inv[v]) for v in go.SMPLX_EXTRA]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=8)
    a = ap.parse_args()
    data, mean = synthetic.make_smplx_data(seed=0), synthetic.make_mean_params(seed=0)
    init = torch.cat([torch.eye(3)[:, :2].reshape(1, 3, 2).repeat(53, 1, 1).flatten(), torch.zeros(NB + 13)])
    init[:144] = torch.as_tensor(np.asarray(mean["pose"], dtype=np.float32)).flatten()
    pdata, pextra = permuted(data)
    b64, b32 = go.OracleBody(data, "smplx", NB, dtype=torch.float64), go.OracleBody(data, "smplx", NB, dtype=torch.float32)
    b32p = go.OracleBody(pdata, "smplx", NB, dtype=torch.float32, extra=pextra)
    mask = fo.column_mask(NB, ("pose", "shape", "depth", "loc"))
    kw = dict(nb=NB, img_size=S, sigma=SIGMA, robust="l2", lam={}, lr=LR)
    lines = ["keypoint fit, loop gate (tools/fit_gate_spread.py; CPU): trace distance max_t |E[t] - E64[t]| / E64[0] to the fp64 oracle",
             f"recovery scene, P = {P}, B = 2, L2, sigma = {SIGMA}, zero priors, all 127 joints given, lr = {LR}, optimize pose + shape + depth + loc",
             "steps seed  E64[0]       E64[last]    y32        y32p       y32p/y32  defect(no recentring in the gradient)"]
    worst = {}
    for steps in (5, 30):
        for seed in range(a.seeds):
            sc = fo.scene(init, P, 2, S // 14, S, 500 + seed, b64, nb=NB)
            args = (sc["readout"], sc["offset"], sc["idx"], sc["K"])
            tail = (sc["keypoints"], sc["confidence"], mask, steps)
            t64 = fo.loop(*args, b64, *tail, torch.float64, **kw)[2]
            d32 = fo.trace_distance(fo.loop(*args, b32, *tail, torch.float32, **kw)[2], t64)
            d32p = fo.trace_distance(fo.loop(*args, b32p, *tail, torch.float32, **kw)[2], t64)
            dd = fo.trace_distance(fo.loop(*args, b64, *tail, torch.float64, recentre="detach", **kw)[2], t64)
            lines.append(f"{steps:5d} {seed:4d}  {float(t64[0].max()):.6e} {float(t64[-1].max()):.6e} {d32:.3e}  {d32p:.3e}  {d32p / d32:8.2f}  {dd:.3e}")
            print(lines[-1], flush=True)
            w = worst.setdefault(steps, dict(y=0.0, ratio_lo=1e9, ratio_hi=0.0, defect=1e9))
            w["y"], w["defect"] = max(w["y"], d32, d32p), min(w["defect"], dd)
            w["ratio_lo"], w["ratio_hi"] = min(w["ratio_lo"], d32p / d32), max(w["ratio_hi"], d32p / d32)
    for steps, w in worst.items():
        lines.append(f"steps {steps}: largest fp32 distance {w['y']:.3e}; y32p / y32 between {w['ratio_lo']:.2f} and {w['ratio_hi']:.2f}; smallest defect "
                     f"{w['defect']:.3e}; a quarter of it {w['defect'] / 4:.3e} = {w['defect'] / 4 / w['y']:.1f} x the largest fp32 distance")
        print(lines[-1])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", "fit_tests.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
