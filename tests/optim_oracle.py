"""Oracles of the fused Adam step (csrc/optim.hip, multi_hmr_amd/optim.py), numpy on the CPU.

``adam_step``: Adam in float64 from the state it is given (fp32 state is widened first), per-tensor step counts, skipped tensors (gradient
None) and the global gradient-norm clip of ``torch.nn.utils.clip_grad_norm_``.  ``apply_segments``: the pack rules of
``multi_hmr_amd.optim.head_segments`` applied to parameter values -- where each element of each parameter lands in the packed tensors, with
which cast, plus which constant or second parameter."""
import numpy as np
import torch


def grad_norm(grads):
    """sqrt of the sum of squares over every present gradient, in float64."""
    return float(np.sqrt(sum(float((np.asarray(g, dtype=np.float64) ** 2).sum()) for g in grads if g is not None)))


def adam_step(state, grads, lr, betas=(0.9, 0.999), eps=1e-8, max_norm=None):
    """``state``: list of dicts ``p``, ``m``, ``v`` (arrays) and ``step`` (int); ``grads``: list of arrays or None (skipped: the entry is
    returned unchanged, step included).  -> (new state in float64, gradient norm or None).  Nothing is modified in place."""
    b1, b2 = betas
    norm = grad_norm(grads) if max_norm is not None else None
    coef = 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
    out = []
    for st, g in zip(state, grads):
        if g is None:
            out.append(dict(st))
            continue
        p, m, v = (np.asarray(st[k], dtype=np.float64) for k in ("p", "m", "v"))
        g = np.asarray(g, dtype=np.float64) * coef
        t = int(st["step"]) + 1
        m = m + (g - m) * (1.0 - b1)
        v = v * b2 + (1.0 - b2) * g * g
        denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps
        p = p - (lr / (1.0 - b1 ** t)) * m / denom
        out.append(dict(p=p, m=m, v=v, step=t))
    return out, norm


def cast16(x, tdt):
    """The pack's 16-bit cast of fp32 values (round to nearest even), returned as the raw 16-bit patterns."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(tdt)
    return t.view(torch.int16).numpy().copy()


def bits(t):
    """A torch tensor -> a flat numpy array of its bit patterns (int32 for fp32, int16 for the 16-bit types)."""
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy().copy()


def apply_segments(segs, values, addends, packed, tdt):
    """``segs``: ``head_segments(model)``; ``values``: {parameter name: fp32 array}; ``addends``: {buffer name: fp32 array of its row 0};
    ``packed``: {target: flat array of BIT PATTERNS (see ``bits``)}, overwritten where a segment claims an element.
    -> {target: flat int array, how many segments wrote each element}."""
    claims = {k: np.zeros(v.shape[0], dtype=np.int32) for k, v in packed.items()}
    for s in segs:
        x = np.asarray(values[s["param"]], dtype=np.float32).reshape(-1)
        if s["param2"]:
            x = x + np.asarray(values[s["param2"]], dtype=np.float32).reshape(-1)
        if s["addend"]:
            x = x + np.asarray(addends[s["addend"]], dtype=np.float32).reshape(-1)
        i = np.arange(x.shape[0], dtype=np.int64)
        idx = s["offset"] + (i // s["cols"]) * s["pitch"] + i % s["cols"]
        packed[s["target"]][idx] = x.view(np.int32) if s["kind"] == "f32" else cast16(x, tdt)
        np.add.at(claims[s["target"]], idx, 1)
    return claims
