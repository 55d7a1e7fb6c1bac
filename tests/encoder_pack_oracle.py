"""Oracle of the device re-pack of the derived encoder operands (csrc/encoder_pack.hip, include/mhmr.h mhmr_vit_repack; DESIGN.md
section 34), numpy on the CPU: the kernels' arithmetic restated operation by operation, fp64 sums in THEIR fixed order.

``row_job``: one linear -> folded weight, 16-bit operand, low half, folded bias, column sum.  ``pos_job``: the resampled position table
and the class row.  ``apply_jobs``: ``multi_hmr_amd.optim.encoder_jobs`` applied to parameter values -- where each result lands in the
packed tensors of a pack."""
import numpy as np
import torch

from multi_hmr_amd import packing

LANES, GROUP = 64, 4


def wave_sum(terms):
    """fp64 [N, K] or [N, K, S] (S terms per element, added in that order) -> [N]: lane l adds the elements k with (k / 4) % 64 == l in
    ascending k, then lane l adds lane l ^ o for o = 32, 16, ..., 1.  The order depends on K alone."""
    t = np.asarray(terms, dtype=np.float64)
    if t.ndim == 2:
        t = t[:, :, None]
    N, K, S = t.shape
    Kp = -(-K // (LANES * GROUP)) * LANES * GROUP
    pad = np.zeros((N, Kp, S), dtype=np.float64)
    pad[:, :K] = t
    pad = pad.reshape(N, Kp // (LANES * GROUP), LANES, GROUP, S)
    acc = np.zeros((N, LANES), dtype=np.float64)
    for it in range(pad.shape[1]):
        for e in range(GROUP):
            for s in range(S):
                acc = acc + pad[:, it, :, e, s]
    lane = np.arange(LANES)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    return acc[:, 0]


def round16(x, tdt):
    """fp32 array -> (the 16-bit round-to-nearest-even cast as a torch tensor, the same values back in fp32 as numpy)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(tdt)
    return t, t.float().numpy()


def bits16(t):
    return t.contiguous().view(torch.int16).numpy().copy()


def row_job(W, tdt, ln_w=None, ln_b=None, bias=None, lo_form=None, lo_rows=None, want_sums=False):
    """``W`` fp32 [N, K].  -> dict: ``w16`` (int16 bit patterns [N, K]), ``lo`` ([lo_rows count, 2K or 3K] bit patterns, or None),
    ``bias`` (fp32 [N], with ``bias`` and the fold) and ``colsum`` (fp32 [N]) when ``want_sums``."""
    W = np.ascontiguousarray(W, dtype=np.float32)
    N, K = W.shape
    Wf = W * np.asarray(ln_w, dtype=np.float32)[None, :] if ln_w is not None else W            # one fp32 multiply
    hi_t, hi = round16(Wf, tdt)
    out = dict(w16=bits16(hi_t), lo=None)
    terms = hi.astype(np.float64)[:, :, None]
    if lo_form is not None:
        r0, n = lo_rows
        lo_t, lo = round16(Wf[r0:r0 + n] - hi[r0:r0 + n], tdt)                                  # one fp32 subtraction
        h = out["w16"][r0:r0 + n]
        out["lo"] = np.concatenate([h, bits16(lo_t)] + ([h] if lo_form == "triple" else []), axis=1)
        if lo_form == "pair":
            terms = np.concatenate([terms, np.zeros_like(terms)], axis=2)
            terms[r0:r0 + n, :, 1] = lo.astype(np.float64)
    if want_sums:
        out["colsum"] = wave_sum(terms).astype(np.float32)
        if bias is not None and ln_b is not None:
            s = wave_sum(W.astype(np.float64) * np.asarray(ln_b, dtype=np.float32).astype(np.float64)[None, :])
            out["bias"] = (np.asarray(bias, dtype=np.float32).astype(np.float64) + s).astype(np.float32)
    return out


def pos_job(pos_embed, cls_token, G):
    """fp32 [1, 1 + M*M, C], [.., C] -> (pos fp32 [1 + G*G, C], cls_pos0 fp32 [C]): y first, then x, fp64, taps added in tap order."""
    pe = np.asarray(pos_embed, dtype=np.float32)[0]
    M = int(round((pe.shape[0] - 1) ** 0.5))
    cls = np.asarray(cls_token, dtype=np.float32).reshape(-1)
    if G == M:
        pos = pe.copy()
    else:
        grid = pe[1:].reshape(M, M, -1).astype(np.float64)
        w, idx = packing._cubic_taps(M, G)
        acc = np.zeros((G, G, pe.shape[1]), dtype=np.float64)
        for b in range(4):
            t = np.zeros_like(acc)
            for a in range(4):
                t = t + w[:, a][:, None, None] * grid[idx[:, a]][:, idx[:, b]]
            acc = acc + w[:, b][None, :, None] * t
        pos = np.concatenate([pe[:1], acc.reshape(G * G, -1).astype(np.float32)], axis=0)
    return pos, cls + pos[0]


def apply_jobs(jobs, values, packed, tdt):
    """``jobs``: ``encoder_jobs(model, P)``; ``values``: {parameter name: fp32 array}; ``packed``: {target: flat array of BIT PATTERNS of
    the packed tensor (int32 for fp32, int16 for 16-bit)}, overwritten where a job writes.  -> {target: flat int array of write counts}."""
    claims = {k: np.zeros(v.shape[0], dtype=np.int32) for k, v in packed.items()}

    def put(target, idx, val):
        packed[target][np.asarray(idx).reshape(-1)] = np.asarray(val).reshape(-1)
        np.add.at(claims[target], np.asarray(idx).reshape(-1), 1)

    for j in jobs:
        if j["kind"] == "pos":
            pos, cls0 = pos_job(values[j["pos_embed"]], values[j["cls_token"]], j["G"])
            put(j["pos"], np.arange(pos.size), pos.view(np.int32))
            put(j["cls_pos0"], np.arange(cls0.size), cls0.view(np.int32))
            continue
        (r0, N), K = j["rows"], j["K"]
        W = np.asarray(values[j["w"]], dtype=np.float32).reshape(-1, K)[r0:r0 + N]
        ln = j["ln"]
        r = row_job(W, tdt, ln_w=values[ln[0]] if ln else None, ln_b=values[ln[1]] if ln else None, bias=values[j["bias"]] if j["bias"] else None,
                    lo_form=j["lo_form"], lo_rows=j["lo_rows"], want_sums=j["colsum"] is not None)
        if j["w16"] is not None:
            put(j["w16"], np.arange(N * K), r["w16"])
        if j["lo"] is not None:
            sections, sec = (2 if j["lo_form"] == "pair" else 3), j["section"]
            n = j["lo_rows"][1]
            idx = (np.arange(n)[:, None, None] * sections * sec + np.arange(sections)[None, :, None] * sec + np.arange(K)[None, None, :])
            put(j["lo"], idx.reshape(n, sections * K), r["lo"])
        if j["colsum"] is not None:
            put(j["colsum"], np.arange(N), r["colsum"].view(np.int32))
            put(j["bias_out"], np.arange(N), r["bias"].view(np.int32))
    return claims


def ulp_distance(a, b):
    """Elementwise distance in units of the last place between two fp32 arrays of finite values (0 = the same bits, +0 / -0 apart by 0)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
