"""``HeadsAdam``: Adam over ``Model.heads_parameters()`` (+ ``detection_parameters()``) as ONE ``mhmr_adam_step`` call that also rewrites
the packed copies the forward reads.  After ``step()`` the model's packed head buffers hold exactly what
``Model.repack_heads()`` would have produced from the updated parameters -- ``repack_heads()`` afterwards changes no bit -- so the training
step is ``zero_grad(); backward(); step()``.

``head_segments(model)`` is the table in words: for every parameter, where its packed copy lives (``Model._head_tensors`` /
``Model._detect_tensors`` read off into (tensor, offset, cols, pitch, cast, addend, second parameter)).  It needs no GPU; the host tests
apply it in numpy and compare with the pack itself."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .detect_train import DETECTION_PARAMETERS
from .heads_train import DEC_PARTS, HEAD, LAYER_KEYS, head_parameter_names
from .packing import roundup

TOK_B, POS = HEAD + "transformer.to_token_embedding.bias", HEAD + "transformer.pos_embedding"
_INIT = {"decpose": "init_body_pose", "decshape": "init_betas", "deccam": "init_cam", "decexpression": "init_expression"}


def head_segments(model, detection=True) -> list:
    """One dict per segment, in ``heads_parameters()`` (+ ``detection_parameters()``) order: ``param`` (name), ``param2`` (the second
    parameter of a sum, or None), ``target`` (``("head", name)`` -> ``P["hph_t"][name]``, ``("layer", l, field)`` ->
    ``P["hph_t"]["layers"][l][field]``, ``("det", name)`` -> ``P[name]``), ``offset`` (elements into the target), ``cols`` / ``pitch``
    (element i of the parameter -> offset + (i // cols) * pitch + i % cols; 1 / 1 = a plain copy), ``kind`` ("f32" | "op16": the pack's
    16-bit cast) and ``addend`` (name of the buffer whose row 0 the pack adds, or None).  ``pos_embedding`` has no segment of its own: it
    is the second parameter of the token bias."""
    C_, nb, dim = model.embed_dim, model.num_betas, 1024
    Cc = C_ + model.camera_embed_dim
    Kc, Ktok = roundup(Cc, 64), roundup(Cc + 318 + nb + 3, 16)
    segs = []

    def seg(param, target, kind="f32", cols=1, pitch=1, offset=0, addend=None, param2=None):
        segs.append(dict(param=param, param2=param2, target=target, offset=offset, cols=cols, pitch=pitch, kind=kind, addend=addend))

    for name, field in (("mlp_offset.0.weight", "off1_w"), ("mlp_offset.0.bias", "off1_b"), ("mlp_offset.2.weight", "off2_w"),
                        ("mlp_offset.2.bias", "off2_b"), (HEAD + "cross_queries_x", "cq_x"), (HEAD + "cross_queries_y", "cq_y"),
                        (HEAD + "cross_values_x", "cv_x"), (HEAD + "cross_values_y", "cv_y")):
        seg(name, ("head", field))
    seg(HEAD + "transformer.to_token_embedding.weight", ("head", "tok_w"), cols=Cc + 318 + nb + 3, pitch=Ktok)
    seg(TOK_B, ("head", "tok_b"), param2=POS)
    for l in range(model.xat_depth):
        for key, field in zip(LAYER_KEYS, _lib.HphLayerGrads.FIELDS):
            name = f"{HEAD}transformer.transformer.layers.{l}.{key}"
            if field == "to_kv":
                seg(name, ("layer", l, "to_kv16"), kind="op16", cols=Cc, pitch=Kc)
            else:
                seg(name, ("layer", l, field))
    a = 0
    for m, n in zip(DEC_PARTS, (318, nb, 3, 10)):
        seg(f"{HEAD}{m}.weight", ("head", "dec_w"), offset=a * dim)
        seg(f"{HEAD}{m}.bias", ("head", "dec_b"), offset=a, addend=HEAD + _INIT[m])
        a += n
    if detection:
        seg(DETECTION_PARAMETERS[0], ("det", "cls0_w"), kind="op16")
        for name, field in zip(DETECTION_PARAMETERS[1:], ("cls0_b", "cls2_w", "cls2_b")):
            seg(name, ("det", field))
    return segs


def packed_target(P, target):
    """The packed tensor a segment's ``target`` names, in a pack ``P`` (or in any dict laid out like it)."""
    if target[0] == "head":
        return P["hph_t"][target[1]]
    if target[0] == "layer":
        return P["hph_t"]["layers"][target[1]][target[2]]
    return P[target[1]]


def bias_corrections(step, lr, beta1, beta2):
    """(lr / (1 - beta1^t), sqrt(1 - beta2^t)) in double, as torch's single-tensor Adam takes them."""
    return lr / (1.0 - beta1 ** step), (1.0 - beta2 ** step) ** 0.5


def table_bytes(table) -> int:
    """Bytes one ``mhmr_adam_step`` moves for a host table of ``_lib.AdamSegment``: per element of a segment with a gradient, parameter and
    two moments read and written and the gradient read (28 bytes; twice that with a second parameter), the addend read, the packed copy
    written.  Skipped segments move nothing.  The clip's first launch reads the gradients once more (not counted)."""
    total = 0
    for s in table:
        if not s.grad:
            continue
        per = 28 * (2 if s.param2 else 1) + (4 if s.addend else 0) + {_lib.ADAM_PACK_NONE: 0, _lib.ADAM_PACK_F32: 4}.get(s.packed_kind, 2)
        total += per * s.n
    return total


class HeadsAdam(torch.optim.Optimizer):
    """Adam (``lr``, ``betas``, ``eps``; no weight decay, no amsgrad, no maximize) over ``model.heads_parameters()`` and, with
    ``detection=True``, ``model.detection_parameters()``.  State per parameter is ``step`` / ``exp_avg`` / ``exp_avg_sq`` as
    ``torch.optim.Adam`` keeps it: a ``state_dict()`` loads into ``torch.optim.Adam`` over the same list, and the reverse.

    ``step()`` is one ``mhmr_adam_step`` call under the model's lock: every parameter whose ``grad`` is set is updated and its packed copy
    rewritten in the same pass; a parameter without a gradient keeps its bits, moments, step count and packed copy.  It moves the model's
    ``heads_generation`` as ``repack_heads()`` does, so a ``backward()`` that comes after it raises.  Before the first forward (nothing
    packed) it updates the parameters only.  ``max_grad_norm``: global gradient-norm clipping as ``torch.nn.utils.clip_grad_norm_`` over the
    same list, inside the update; ``last_grad_norm`` is then the norm of the last step, a device tensor (no synchronisation).

    Parameters must be contiguous fp32 on the GPU at ``step()``; a CPU model raises (there is no CPU path)."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, detection=True, max_grad_norm=None, weight_decay=0, amsgrad=False,
                 maximize=False):
        if weight_decay != 0 or amsgrad or maximize:
            raise ValueError("HeadsAdam supports lr, betas and eps only: no weight_decay, amsgrad or maximize")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"invalid lr / eps / betas: {lr}, {eps}, {betas}")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError("max_grad_norm must be positive (None: no clipping)")
        self.model, self.detection, self.max_grad_norm = model, bool(detection), max_grad_norm
        self._names = head_parameter_names(model.xat_depth) + (list(DETECTION_PARAMETERS) if detection else [])
        named = dict(model.named_parameters())
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None)
        super().__init__([named[n] for n in self._names], defaults)
        self._table = None
        self.last_grad_norm = None

    # ------------------------------------------------------------------------------------------------ the table
    def _state(self, p, row, which):
        """The state of ``p`` (created with its first gradient, as torch.optim.Adam does).  The two moments are validated when they are first
        seen -- fresh, or loaded by ``load_state_dict`` -- and recognised by identity afterwards."""
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        seen = row[which]
        if seen is None or seen[0] is not st["exp_avg"] or seen[1] is not st["exp_avg_sq"]:
            for k in ("exp_avg", "exp_avg_sq"):
                t = st[k]
                if t.device != p.device or t.dtype != torch.float32 or not t.is_contiguous() or t.shape != p.shape:
                    raise _lib.MhmrError(f"HeadsAdam: state '{k}' must be a contiguous fp32 tensor on the parameter's device, of its shape")
            row[which] = (st["exp_avg"], st["exp_avg_sq"])
        return st

    def _build(self, P, dev):
        """The table for the pack ``P`` (None: parameters only).  What does not change from step to step is written here: element count,
        cols / pitch, first chunk, and where the packed copy and the constant addend live (the rows keep those tensors)."""
        model, named = self.model, dict(self.model.named_parameters())
        buffers = dict(model.named_buffers())
        kind16 = None if P is None else (_lib.ADAM_PACK_F16 if P["tdt"] == torch.float16 else _lib.ADAM_PACK_BF16)
        specs = head_segments(model, self.detection)
        host = (_lib.AdamSegment * len(specs))()
        rows, chunk0 = [], 0
        for seg, s in zip(host, specs):
            p = named[s["param"]]
            row = dict(name=s["param"], name2=s["param2"], p=p, p2=named[s["param2"]] if s["param2"] else None, packed=None, addend=None,
                       st=None, st2=None)
            seg.n, seg.cols, seg.pitch, seg.packed_kind, seg.chunk0 = p.numel(), s["cols"], s["pitch"], _lib.ADAM_PACK_NONE, chunk0
            if s["addend"]:
                row["addend"] = buffers[s["addend"]][0].detach().to(device=dev, dtype=torch.float32).contiguous()
                seg.addend = row["addend"].data_ptr()
            if P is not None:
                t = packed_target(P, s["target"])
                want = torch.float32 if s["kind"] == "f32" else P["tdt"]
                if t.dtype != want or not t.is_contiguous() or s["offset"] + (p.numel() // s["cols"] - 1) * s["pitch"] + s["cols"] > t.numel():
                    raise _lib.MhmrError(f"HeadsAdam: the packed tensor of {s['param']} is not laid out as Model._head_tensors makes it")
                row["packed"], seg.packed_kind = t, (_lib.ADAM_PACK_F32 if s["kind"] == "f32" else kind16)
                seg.packed = t.data_ptr() + s["offset"] * t.element_size()
            chunk0 += -(-p.numel() // _lib.ADAM_CHUNK)
            rows.append(row)
        nbytes = C.sizeof(host)
        return dict(P=P, dev=dev, rows=rows, host=host, nbytes=nbytes, chunks=chunk0, device=torch.empty(nbytes, dtype=torch.uint8, device=dev),
                    partials=torch.empty(chunk0, dtype=torch.float64, device=dev) if self.max_grad_norm is not None else None,
                    norm=torch.zeros(1, dtype=torch.float32, device=dev))

    @staticmethod
    def _check(p, what):
        if not p.is_cuda:
            raise _lib.MhmrError(f"HeadsAdam: {what} is on the CPU; the step runs only on an MI355X (HIP) tensor, there is no CPU fallback")
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise _lib.MhmrError(f"HeadsAdam: {what} must be a contiguous fp32 tensor")

    @staticmethod
    def _grad(p, name, keep):
        g = p.grad
        if g is None:
            return None
        if g.is_sparse or g.device != p.device or g.shape != p.shape:
            raise _lib.MhmrError(f"HeadsAdam: the gradient of {name} must be a dense tensor of the parameter's shape on its device")
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.detach().to(torch.float32).contiguous()
            keep.append(g)                           # (alive until the call has been enqueued: the allocator is stream-ordered)
        return g

    def _fill(self, tab, group):
        """Everything that changes from step to step: parameter / moment / gradient pointers, the step counts and their scalars."""
        lr, (beta1, beta2) = float(group["lr"]), group["betas"]
        keep, stepped, cache = [], [], {}

        def scalars(st):
            t = float(st["step"]) + 1.0
            if t not in cache:
                cache[t] = bias_corrections(t, lr, beta1, beta2)
            return cache[t]

        for seg, row in zip(tab["host"], tab["rows"]):
            p, p2 = row["p"], row["p2"]
            self._check(p, row["name"])
            g = self._grad(p, row["name"], keep)
            if p2 is not None:
                # the sum of two parameters: both with a gradient -> one segment updates both; one without -> it is a constant addend of
                # the other (read from the parameter itself); neither -> skipped
                self._check(p2, row["name2"])
                g2, st_key, st2_key = self._grad(p2, row["name2"], keep), "st", "st2"
                if g is None and g2 is not None:
                    p, p2, g, g2, st_key, st2_key = p2, p, g2, None, "st2", "st"
                seg.param2 = seg.exp_avg2 = seg.exp_avg_sq2 = seg.grad2 = seg.addend = None
                if g is not None and g2 is None:
                    seg.addend = p2.data_ptr()
                elif g is not None:
                    st2 = self._state(p2, row, st2_key)
                    seg.param2, seg.exp_avg2, seg.exp_avg_sq2, seg.grad2 = (p2.data_ptr(), st2["exp_avg"].data_ptr(),
                                                                            st2["exp_avg_sq"].data_ptr(), g2.data_ptr())
                    seg.step_size2, seg.bc2_sqrt2 = scalars(st2)
                    stepped.append(st2)
            else:
                st_key = "st"
            seg.param = p.data_ptr()
            if g is None:
                seg.grad = None
                continue
            st = self._state(p, row, st_key)
            seg.grad, seg.exp_avg, seg.exp_avg_sq = g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            seg.step_size, seg.bc2_sqrt = scalars(st)
            stepped.append(st)
        return keep, stepped

    # ------------------------------------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if len(self.param_groups) != 1:
            raise _lib.MhmrError("HeadsAdam keeps one parameter group")
        group = self.param_groups[0]
        if group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or group.get("maximize", False):
            raise ValueError("HeadsAdam supports lr, betas and eps only: no weight_decay, amsgrad or maximize")
        model = self.model
        with model._lock:
            dev = group["params"][0].device
            if dev.type != "cuda":
                raise _lib.MhmrError("HeadsAdam: the parameters are on the CPU; the step runs only on an MI355X (HIP) tensor, there is no CPU "
                                     "fallback")
            P = model._packed if (model._packed is not None and model._packed["device"] == dev) else None
            tab = self._table
            if tab is None or tab["P"] is not P or tab["dev"] != dev or (tab["partials"] is None) != (self.max_grad_norm is None):
                tab = self._table = self._build(P, dev)
            keep, stepped = self._fill(tab, group)
            if not stepped:
                return loss
            clip = self.max_grad_norm is not None
            with torch.cuda.device(dev):
                # the table travels through a pinned block of torch's caching host allocator: a non-blocking copy records an event on the
                # stream for the block, and the allocator hands the block out again only once that event has completed
                stage = torch.empty(tab["nbytes"], dtype=torch.uint8, pin_memory=True)
                C.memmove(stage.data_ptr(), C.addressof(tab["host"]), tab["nbytes"])
                tab["device"].copy_(stage, non_blocking=True)
                stream = torch.cuda.current_stream(dev).cuda_stream
                _lib.check(_lib.lib().mhmr_adam_step(tab["host"], tab["device"].data_ptr(), len(tab["rows"]), float(group["betas"][0]),
                                                     float(group["betas"][1]), float(group["eps"]),
                                                     float(self.max_grad_norm) if clip else 0.0,
                                                     tab["partials"].data_ptr() if clip else None, tab["chunks"] if clip else 0,
                                                     tab["norm"].data_ptr(), stream), "mhmr_adam_step")
            for st in stepped:
                st["step"] += 1
            if clip:
                self.last_grad_norm = tab["norm"]
            if P is not None:
                P["heads_generation"] += 1
        return loss


__all__ = ["HeadsAdam", "head_segments", "packed_target", "bias_corrections", "table_bytes"]
