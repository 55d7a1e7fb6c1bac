"""TEST INFRASTRUCTURE for the keypoint fit (multi_hmr_amd/fit.py, csrc/fit.hip).

The objective of include/mhmr.h (mhmr_fit_keypoints) restated in torch on the CPU at any dtype, on ``heads_oracle.decode`` (the read-out ->
j2d function, itself on ``gt_oracle.OracleBody``): the data term over the given joints, the five quadratic priors to the anchors, the
gradient by ``torch.autograd`` times the column mask, and the loop with single-tensor ``torch.optim.Adam``.  float64 is the reference value
(``o64``); the same code in float32 (``y32``) is the yardstick of the 4x rule.

A joint that is not given (c = 0) is taken out at the INPUT: its target is replaced by zeros before anything is computed, so a NaN there
can reach neither the value nor -- through ``0 * NaN`` in a backward -- the gradient."""
import torch

import gt_oracle as go
import heads_oracle as ho

GROUPS = ("pose", "shape", "depth", "expression", "loc")
COCO17 = ("nose", "left_eye", "right_eye", "left_ear", "right_ear", "left_shoulder", "right_shoulder", "left_elbow", "right_elbow",
          "left_wrist", "right_wrist", "left_hip", "right_hip", "left_knee", "right_knee", "left_ankle", "right_ankle")
#: the SMPL-X chain (the oracle's own copy): parent of each of the 55 joints
PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 15, 15, 15,
           20, 25, 26, 20, 28, 29, 20, 31, 32, 20, 34, 35, 20, 37, 38, 21, 40, 41, 21, 43, 44, 21, 46, 47, 21, 49, 50, 21, 52, 53]


def spans(nb):
    """Columns of [pose6d 318 | betas nb | cam 3 | expr 10 | offset 2] that each group owns (cam[1:3] belong to nobody)."""
    return dict(pose=(0, 318), shape=(318, 318 + nb), depth=(318 + nb, 318 + nb + 1), expression=(318 + nb + 3, 318 + nb + 13),
                loc=(318 + nb + 13, 318 + nb + 15))


def column_mask(nb, optimize):
    m = torch.zeros(318 + nb + 15)
    for g in optimize:
        a, b = spans(nb)[g]
        m[a:b] = 1.0
    return m


def energy(r, o, r0, o0, idx, K, body, kp, conf, *, nb, img_size, sigma, robust, lam, nearness=True, center=15, dtype=torch.float64,
           recentre=True):
    """E [P] at (r, o) in ``dtype`` (and the j2d it was taken at).  ``recentre="detach"`` keeps the value and drops the recentring's
    term of the GRADIENT (the centre joint is a constant of the backward: what a placement backward that forgot ``- S_p`` on the centre
    row would compute) -- the defect whose trace change sizes the loop's gate."""
    detach = recentre == "detach" and center is not None
    out, _ = ho.decode(r, o, idx, K, body, nb=nb, img_size=img_size, nearness=nearness, center=None if detach else center, dtype=dtype)
    if detach:                                                         # out: x = u + transl; take the centre off as a constant
        uc = (out["j3d"][:, [center]] - out["transl"][:, None]).detach()
        out = dict(out, j2d=go.perspective_projection(out["j3d"] - uc, K.to(dtype)[idx[0].long()]))
    given = conf > 0
    c = torch.where(given, conf, torch.zeros_like(conf)).to(dtype)
    target = torch.where(given[..., None], kp, torch.zeros_like(kp)).to(dtype)
    s = ((out["j2d"] - target) ** 2).sum(-1) / (sigma * sigma)
    rho = s if robust == "l2" else s / (1 + s)
    E = (c * rho).sum(1)
    x, x0 = torch.cat([r.to(dtype), o.to(dtype)], 1), torch.cat([r0.to(dtype), o0.to(dtype)], 1)
    for g, (a, b) in spans(nb).items():
        if lam.get(g, 0.0):
            E = E + lam[g] * ((x[:, a:b] - x0[:, a:b]) ** 2).sum(1)
    return E, out["j2d"]


def value_and_grad(r, o, r0, o0, idx, K, body, kp, conf, mask, dtype, **kw):
    """-> (E [P], masked gradient [P, D + 2]) in ``dtype``."""
    rr, oo = r.detach().to(dtype).requires_grad_(), o.detach().to(dtype).requires_grad_()
    E, _ = energy(rr, oo, r0, o0, idx, K, body, kp, conf, dtype=dtype, **kw)
    g = torch.autograd.grad(E.sum(), [rr, oo])
    return E.detach(), torch.cat(g, 1) * mask.to(dtype)


def loop(r, o, idx, K, body, kp, conf, mask, steps, dtype, *, lr, betas=(0.9, 0.999), eps=1e-8, **kw):
    """``steps`` steps of single-tensor torch.optim.Adam from (r, o), anchored there -> (r, o, trace [steps + 1, P]) in ``dtype``."""
    r0, o0 = r.detach().to(dtype), o.detach().to(dtype)
    rr, oo = r0.clone().requires_grad_(), o0.clone().requires_grad_()
    opt = torch.optim.Adam([rr, oo], lr=lr, betas=betas, eps=eps, foreach=False)
    m, W = mask.to(dtype), r0.shape[1]
    trace = []
    for _ in range(steps):
        opt.zero_grad()
        E, _ = energy(rr, oo, r0, o0, idx, K, body, kp, conf, dtype=dtype, **kw)
        E.sum().backward()
        rr.grad *= m[:W]
        oo.grad *= m[W:]
        trace.append(E.detach())
        opt.step()
    with torch.no_grad():
        trace.append(energy(rr, oo, r0, o0, idx, K, body, kp, conf, dtype=dtype, **kw)[0])
    return rr.detach(), oo.detach(), torch.stack(trace)


def trace_distance(trace, trace64):
    """max_t |E[t] - E64[t]| / E64[0], the worst person."""
    t64 = trace64.double()
    return float(((trace.double() - t64).abs().max(0).values / t64[0]).max())


def descendants_given(conf_row):
    """[55] bool: joint j of the chain has a given output joint in its subtree -- picked vertices and landmarks hang on the chain through
    their skinning weights, so this is the test's SUFFICIENT condition for an exact-zero pose gradient only when none of them is given
    (the COCO case gives chain joints and face / ear vertices: the caller says which chain joints those hang on)."""
    has = [bool(conf_row[j] > 0) for j in range(55)]
    for j in range(54, 0, -1):
        if has[j]:
            has[PARENTS[j]] = True
    return torch.tensor(has)


def scene(init, P, B, G, img_size, seed, body64, *, nb, perturb=0.05, nearness=True, general_K=False):
    """The recovery scene: seeded persons (``heads_oracle.make_inputs``), targets = the fp64 j2d of a copy whose read-out and offset are
    perturbed by N(0, perturb), every joint given with confidence 1."""
    r, o, idx, K = ho.make_inputs(init, P, B, G, img_size, seed, nearness=nearness, general_K=general_K)
    g = torch.Generator().manual_seed(seed + 7)
    rt, ot = r + perturb * torch.randn(r.shape, generator=g), o + perturb * torch.randn(o.shape, generator=g)
    with torch.no_grad():
        out, _ = ho.decode(rt, ot, idx, K, body64, nb=nb, img_size=img_size, nearness=nearness, center=15, dtype=torch.float64)
    kp = out["j2d"].float()
    return dict(readout=r, offset=o, idx=idx, K=K, keypoints=kp, confidence=torch.ones(P, kp.shape[1]))


max_err = go.max_err
