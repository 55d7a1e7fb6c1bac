"""The training loss restated (reference loss.py:8-40, 47-115) -- an independent numpy statement of the
formula the tests hold ``mhmr_loss_forward`` / ``mhmr_loss_backward`` against, plus the seeded input maker they share.

Values are fp64 from the fp32 inputs.  For every L1 term the oracle also returns the magnitude sum ``M``: the same reduction and
normaliser with ``|u - u_hat|`` replaced by ``|u| + |u_hat|`` (u, u_hat = the operands after centring, or the raw operands where
nothing is centred).  The kernel forms each element in fp32 -- at most three roundings (two centrings, one difference), each bounded
by 2^-24 (|u| + |u_hat|) -- accumulates in fp64 (negligible) and rounds the result once, so

    |kernel - fp64| <= BOUND_ULPS * 2^-24 * M,    BOUND_ULPS = 4,

for the focal term (fp64 throughout, one rounding) ``BOUND_ULPS * 2^-24 * |bce|``, and for ``total`` the alpha-weighted sum of the
bounds of the terms it contains.  Gradients: the SIGN of every element comes from the fp32 elementwise evaluation (numpy float32
arithmetic rounds operation by operation, like the kernel built without FMA contraction), the pelvis sums are integers, all scaling is
fp64; the kernel rounds each gradient once, so it is within ``BOUND_ULPS * 2^-24`` relative of the oracle per element and exactly
0 where the oracle is 0.
"""
from types import SimpleNamespace

import numpy as np

KEYS = ("total", "bce", "offset", "rotmat", "shape", "dist", "transl", "j3d", "v3d", "j2d", "v2d")
#: reference loss.py:121-137 (Loss.add_specific_args)
DEFAULTS = dict(alpha_bce=10.0, alpha_offset=1.0, alpha_rotmat=0.1, alpha_shape=1.0, alpha_dist=1.0, alpha_transl=1.0, alpha_j3d=100.0,
                alpha_v3d=100.0, alpha_j2d=1.0, alpha_v2d=1.0, start_2d_epoch=10)
BOUND_ULPS = 4.0
U = 2.0 ** -24


def default_args(**over):
    d = dict(DEFAULTS)
    d.update(over)
    return SimpleNamespace(**d)


def make_inputs(seed, P, V, J, B=2, G=5, nb_hat=10, nb_gt=11, img_size=224.0, num_pos=None):
    """-> (y_hat, y): dicts of fp32 numpy arrays shaped as Model(is_training=True) and GroundTruth.prepare return them.  Persons
    6 - 8 m away, predictions = ground truth + noise; about 20 % of the 2D targets are out of frame, some of them exactly 0 and some
    exactly img_size; a few predictions equal their target exactly (sign 0).  ``num_pos``: positive cells of the score target
    (default: min(P, B G G), at least 1)."""
    r = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    S = float(img_size)
    y, h = {}, {}
    n_pos = max(1, min(P, B * G * G)) if num_pos is None else num_pos
    sc = np.zeros(B * G * G, np.float32)
    sc[r.permutation(B * G * G)[:n_pos]] = 1.0
    y["scores"] = sc.reshape(B, G, G)
    h["scores"] = f(np.clip(r.uniform(0.0, 1.0, (B, G, G, 1)), 1e-4, 1 - 1e-4))
    if P == 0:
        return h, y
    centre = np.concatenate([r.uniform(-1, 1, (P, 1, 2)), r.uniform(6, 8, (P, 1, 1))], -1)
    y["j3d"] = f(centre + 0.3 * r.standard_normal((P, J, 3)))
    y["v3d"] = f(centre + 0.3 * r.standard_normal((P, V, 3)))
    y["transl_pelvis"] = y["j3d"][:, 0].copy()
    y["transl"] = y["j3d"][:, min(15, J - 1)].copy()
    y["offset"] = f(r.uniform(-0.5, 0.5, (P, 2)))
    y["rotmat"] = f(r.uniform(-1, 1, (P, 53, 3, 3)))
    y["shape"] = f(r.standard_normal((P, nb_gt)))
    y["dist_postprocessed"] = f(r.uniform(1.5, 2.5, (P,)))
    for k, n in (("j2d", J), ("v2d", V)):
        t = r.uniform(1.0, S - 1.0, (P, n, 2))
        out = r.uniform(0, 1, (P, n)) < 0.2
        kind = r.integers(0, 5, (P, n))               # 0: x = 0 exactly, 1: y = img_size exactly, 2: negative, 3: beyond, 4: both
        axis = r.integers(0, 2, (P, n))
        val = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [0.0, S, -r.uniform(0, 50, (P, n)), S + r.uniform(0, 50, (P, n)), -3.0])
        pi, ni = np.nonzero(out)
        t[pi, ni, axis[pi, ni]] = val[pi, ni]
        y[k] = f(t)
    noise = dict(j3d=0.02, v3d=0.02, transl=0.02, offset=0.05, rotmat=0.05, shape=0.1, j2d=3.0, v2d=3.0)
    for k, s in noise.items():
        shp = (P, nb_hat) if k == "shape" else y[k].shape
        base = y[k] if k != "shape" else (y[k][:, :nb_hat] if nb_hat <= nb_gt else np.concatenate([y[k], np.zeros((P, nb_hat - nb_gt))], 1))
        h[k] = f(base + s * r.standard_normal(shp))
    h["dist_postprocessed"] = f(y["dist_postprocessed"][:, None] + 0.05 * r.standard_normal((P, 1)))
    # exact ties: sign(0) = 0
    h["rotmat"][:, 0] = y["rotmat"][:, 0]
    h["offset"][0, 0] = y["offset"][0, 0]
    h["j3d"][0, 0] = y["j3d"][0, 0]                  # person 0: equal pelvis ...
    h["v3d"][0, : min(5, V)] = y["v3d"][0, : min(5, V)]   # ... and equal vertices: the centred difference is exactly 0
    h["j2d"][0, 0] = y["j2d"][0, 0]
    h["transl_pelvis"] = h["j3d"][:, :1].copy()      # [P, 1, 3], as the model returns it
    return h, y


def _focal(p, pos):
    eps = 1e-7
    lp = np.where(pos, np.log(p + eps) * (1 - p) ** 2, 0.0)
    ln = np.where(pos, 0.0, np.log(1 - p + eps) * p ** 2)
    dp = np.where(pos, (1 - p) ** 2 / (p + eps) - 2 * (1 - p) * np.log(p + eps), 2 * p * np.log(1 - p + eps) - p ** 2 / (1 - p + eps))
    return lp.sum(), ln.sum(), dp


def loss_ref(y_hat, y, epoch, img_size, args, grad_total=1.0):
    """-> dict(values={key: fp64}, M={key: fp64}, bound={key: fp64}, grads={y_hat key: fp64 array}, counts=dict)."""
    d64 = lambda a: np.asarray(a, dtype=np.float64)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    use_2d = epoch >= args.start_2d_epoch
    gt = float(grad_total)
    val, M, grads = {}, {}, {}
    p = d64(y_hat["scores"]).reshape(-1)
    pos = f32(y["scores"]).reshape(-1) >= 1
    lp, ln, dp = _focal(p, pos)
    npos = int(pos.sum())
    val["bce"] = -ln if npos == 0 else -(lp + ln) / npos
    grads["scores"] = (-gt * args.alpha_bce / max(npos, 1) * dp).reshape(np.shape(y_hat["scores"]))
    counts = dict(num_pos=npos, j2d=0, v2d=0)
    person = "v3d" in y_hat and np.shape(y_hat["v3d"])[0] > 0
    if not person:
        for k in KEYS[2:]:
            val[k], M[k] = 0.0, 0.0
    else:
        P, V, J = np.shape(y_hat["v3d"])[0], np.shape(y_hat["v3d"])[1], np.shape(y_hat["j3d"])[1]
        sd = min(np.shape(y_hat["shape"])[1], np.shape(y["shape"])[1])

        def plain(key, hat, tgt, norm, alpha, shape=None):
            a, b = d64(hat), d64(tgt)
            val[key] = np.abs(a - b).sum() / norm
            M[key] = (np.abs(a) + np.abs(b)).sum() / norm
            g = np.sign(d64(f32(hat) - f32(tgt))) * (gt * alpha / norm)
            return g if shape is None else g.reshape(shape)

        grads["offset"] = plain("offset", y_hat["offset"], y["offset"], P, args.alpha_offset)
        grads["rotmat"] = plain("rotmat", y_hat["rotmat"], y["rotmat"], P, args.alpha_rotmat)
        gs = np.zeros(np.shape(y_hat["shape"]))
        gs[:, :sd] = plain("shape", y_hat["shape"][:, :sd], y["shape"][:, :sd], P, args.alpha_shape)
        grads["shape"] = gs
        grads["dist_postprocessed"] = plain("dist", np.reshape(y_hat["dist_postprocessed"], (P,)), y["dist_postprocessed"], P, args.alpha_dist,
                                            np.shape(y_hat["dist_postprocessed"]))
        grads["transl"] = plain("transl", y_hat["transl"], y["transl"], P, args.alpha_transl)

        pg32, ph32 = f32(y["transl_pelvis"]).reshape(P, 1, 3), f32(y_hat["transl_pelvis"]).reshape(P, 1, 3)
        gp = {}
        for key, n, alpha in (("j3d", J, args.alpha_j3d), ("v3d", V, args.alpha_v3d)):
            u, uh = d64(y[key]) - d64(pg32), d64(y_hat[key]) - d64(ph32)
            val[key] = np.abs(u - uh).sum() / (P * n)
            M[key] = (np.abs(u) + np.abs(uh)).sum() / (P * n)
            sg = np.sign((f32(y[key]) - pg32) - (f32(y_hat[key]) - ph32)).astype(np.int64)     # fp32, operation by operation
            c = gt * alpha / (P * n)
            grads[key] = -sg * c
            gp[key] = c * sg.sum(1)                                                           # integer sums, scaled once

        S = np.float32(img_size)
        for key, alpha in (("j2d", args.alpha_j2d), ("v2d", args.alpha_v2d)):
            t32 = f32(y[key])
            m = ((t32 > 0) & (t32 < S)).sum(-1) == 2
            cnt = int(m.sum())
            counts[key] = cnt
            a, b = d64(y_hat[key]), d64(y[key])
            with np.errstate(invalid="ignore", divide="ignore"):
                val[key] = np.float64(np.abs(a - b)[m].sum()) / cnt
                M[key] = np.float64((np.abs(a) + np.abs(b))[m].sum()) / cnt
            g = np.zeros(a.shape)
            if cnt and use_2d:
                g[m] = np.sign(d64(f32(y_hat[key]) - t32))[m] * (gt * alpha / cnt)
            grads[key] = g
    finite = {}
    for k in KEYS[1:]:
        finite[k] = bool(np.isfinite(val[k]))
        if not finite[k]:
            val[k], M[k] = 0.0, 0.0
    # a term that was not finite contributes nothing, forwards or backwards (the deliberate deviation of DESIGN.md section 17)
    gkeys = dict(bce=("scores",), dist=("dist_postprocessed",))
    for k in KEYS[1:]:
        if not finite[k]:
            for gk in gkeys.get(k, (k,)):
                if gk in grads:
                    grads[gk] = np.zeros_like(grads[gk])
    if person:
        grads["transl_pelvis"] = sum(gp[k] for k in ("j3d", "v3d") if finite[k]).reshape(np.shape(y_hat["transl_pelvis"])) \
            if (finite["j3d"] or finite["v3d"]) else np.zeros(np.shape(y_hat["transl_pelvis"]))
    alphas = {k: getattr(args, "alpha_" + k) for k in KEYS[1:]}
    bound = {k: BOUND_ULPS * U * M[k] for k in KEYS[2:]}
    bound["bce"] = BOUND_ULPS * U * abs(val["bce"])
    in_total = [k for k in KEYS[1:] if use_2d or k not in ("j2d", "v2d")]
    val["total"] = sum(alphas[k] * val[k] for k in in_total)
    bound["total"] = sum(alphas[k] * bound[k] for k in in_total)
    return dict(values=val, M=M, bound=bound, grads=grads, counts=counts, finite=finite)


def reference_fp32_bound(y_hat, y, res, args, use_2d=True, typical=False):
    """A bound on |reference fp32 result - fp64 value| per key, for ANY summation order of the reference's torch reductions: each
    element carries the three fp32 roundings above (3 u M), a sum of n fp32 summands in any order is within (n - 1) u of the sum of
    magnitudes, so a chain of reductions over axes of n_1, n_2, ... summands (plus one rounding per division) adds
    (n_1 + n_2 + ... + 3) u M.  The focal term in fp32: the log's argument is rounded twice (<= 2 u relative, i.e. 2 u absolute in the
    log), the log, the square and the two products once each (<= 5 u relative on the element), the weight is <= 1; then two sums of
    n = B G G summands, a sum and a division.  ``total``: the weighted bounds plus twelve more fp32 operations on its magnitude.
    ``typical=True``: the statistical form of the same count (the worst case assumes every rounding of a 10^5-term sum errs the same
    way and says little there)."""
    P = np.shape(y_hat["v3d"])[0]
    V, J = np.shape(y_hat["v3d"])[1], np.shape(y_hat["j3d"])[1]
    nred = dict(offset=2 + P, rotmat=int(np.prod(np.shape(y_hat["rotmat"])[1:])) + P, shape=min(np.shape(y_hat["shape"])[1], np.shape(y["shape"])[1]) + P,
                dist=P, transl=3 + P, j3d=3 + J + P, v3d=3 + V + P, j2d=2 + res["counts"]["j2d"], v2d=2 + res["counts"]["v2d"])
    b = {k: (3 + n + 3) * U * res["M"][k] for k, n in nred.items()}
    if typical:     # the same roundings as independent errors: the sum of m of them has standard deviation sqrt(m) u; eight of those
        b = {k: 8 * np.sqrt(3 + n + 3) * U * res["M"][k] for k, n in nred.items()}
    p = np.asarray(y_hat["scores"], dtype=np.float64).reshape(-1)
    pos = np.asarray(y["scores"]).reshape(-1) >= 1
    x = np.where(pos, p + 1e-7, 1 - p + 1e-7)
    w = np.where(pos, (1 - p) ** 2, p ** 2)
    term = np.abs(np.log(x)) * w
    npos = max(int(pos.sum()), 1)
    b["bce"] = (U * (2 * w + 5 * term).sum() + (p.size + 4) * U * term.sum()) / npos
    keys = [k for k in KEYS[1:] if use_2d or k not in ("j2d", "v2d")]
    b["total"] = sum(getattr(args, "alpha_" + k) * b[k] for k in keys) + 12 * U * sum(getattr(args, "alpha_" + k) * abs(res["values"][k]) for k in keys)
    return b
