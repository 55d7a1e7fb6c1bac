"""``HeadsAdam``: Adam over ``Model.heads_parameters()`` (+ ``detection_parameters()``) as ONE ``mhmr_adam_step`` call that also rewrites
the packed copies the forward reads.  After ``step()`` the model's packed head buffers hold exactly what
``Model.repack_heads()`` would have produced from the updated parameters -- ``repack_heads()`` afterwards changes no bit -- so the training
step is ``zero_grad(); backward(); step()``.

``head_segments(model)`` is the table in words: for every parameter, where its packed copy lives (``Model._head_tensors`` /
``Model._detect_tensors`` read off into (tensor, offset, cols, pitch, cast, addend, second parameter)).  It needs no GPU; the host tests
apply it in numpy and compare with the pack itself.

``ModelAdam``: the same over the whole model -- heads, detector, ``backbone_parameters(n)`` and the token embedding.
``encoder_segments(model)`` are the encoder's rows of that table (the packed tensors that are copies or casts), ``encoder_jobs(model)`` the
``mhmr_vit_repack`` jobs that derive the rest on the device: folded linears, column sums, low-half rows, triples, the position table."""
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
    if target[0] == "block":
        return P["vit"]["block_t"][target[1]][target[2]]
    if target[0] in ("norm", "embed"):
        return P["vit"][target[0] + "_t"][target[1]]
    return P[target[1]]


def bias_corrections(step, lr, beta1, beta2):
    """(lr / (1 - beta1^t), sqrt(1 - beta2^t)) in double, as torch's single-tensor Adam takes them."""
    return lr / (1.0 - beta1 ** step), (1.0 - beta2 ** step) ** 0.5


def table_bytes(table, jobs=()) -> int:
    """Bytes one ``mhmr_adam_step`` moves for a host table of ``_lib.AdamSegment``: per element of a segment with a gradient, parameter and
    two moments read and written and the gradient read (28 bytes; twice that with a second parameter), the addend read, the packed copy
    written.  Skipped segments move nothing.  The clip's first launch reads the gradients once more (not counted).  ``jobs``: the
    ``_lib.PackJob`` entries of the ``mhmr_vit_repack`` call that follows (``ModelAdam``); their reads and writes are added (``job_bytes``)."""
    total = 0
    for s in table:
        if not s.grad:
            continue
        per = 28 * (2 if s.param2 else 1) + (4 if s.addend else 0) + {_lib.ADAM_PACK_NONE: 0, _lib.ADAM_PACK_F32: 4}.get(s.packed_kind, 2)
        total += per * s.n
    return total + job_bytes(jobs)


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
        self._names = self._parameter_names()
        named = dict(model.named_parameters())
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None)
        super().__init__([named[n] for n in self._names], defaults)
        self._table = None
        self.last_grad_norm = None

    # ------------------------------------------------------------------------------------------------ the table
    def _parameter_names(self):
        """``named_parameters`` keys of the list this optimiser steps, in its order."""
        return head_parameter_names(self.model.xat_depth) + (list(DETECTION_PARAMETERS) if self.detection else [])

    def _specs(self, P):
        """The segments of the table for the pack ``P`` (None: nothing packed), as ``head_segments`` describes them."""
        return head_segments(self.model, self.detection)

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
        specs = self._specs(P)
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
            if P is not None and s["kind"] is not None:
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
        names = tab["stepped_names"] = set()

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
                    names.add(row["name2"] if st2_key == "st2" else row["name"])
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
            names.add(row["name"] if st_key == "st" else row["name2"])
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
            self._after_step(tab, P, stream)
        return loss

    def _after_step(self, tab, P, stream):
        """What follows the Adam launch, under the model's lock: the pack's counter moves as ``repack_heads()`` moves it."""
        if P is not None:
            P["heads_generation"] += 1


# ---------------------------------------------------------------------------------------------------- the whole model
def _encoder_names(model) -> list:
    """``backbone_parameters(model._backbone_n)`` + ``embedding_parameters()`` when any of those requires grad, by name."""
    from .backbone_train import backbone_parameter_names, embedding_parameter_names
    names = backbone_parameter_names(len(model.backbone.encoder.blocks), model._backbone_n)
    if any(p.requires_grad for p in model.embedding_parameters()):
        names += embedding_parameter_names()
    return names


def _derived(P) -> bool:
    """Whether the derived operands of the pack ``P`` have device jobs (``encoder_jobs``): every pack but one with fp8 low halves."""
    return P is not None and not P.get("lo8")


def encoder_segments(model, P=None) -> list:
    """The encoder's rows of the Adam table, laid out as ``head_segments``' rows, in ``backbone_parameters(n)`` (+
    ``embedding_parameters()`` when they require grad) order, for the pack ``P`` (default: the model's; its choices -- operand type, fold,
    low halves, f16x3 -- decide which packed tensors are copies).  ``target``: ``("norm", name)`` -> ``P["vit"]["norm_t"][name]``,
    ``("block", l, field)`` -> ``P["vit"]["block_t"][l][field]``, ``("embed", name)`` -> ``P["vit"]["embed_t"][name]``.  A parameter whose
    packed form is a copy (LayerNorm, LayerScale, plain biases, the final norm, ``patch_b``: fp32; the unfolded 16-bit weights; ``patch_w``
    with ``cols=588, pitch=Kp``) carries it, zero padding behind it untouched.  A parameter whose packed form is DERIVED -- a folded
    linear and its bias, every weight of an f16x3 pack, the position table, the class token -- has ``kind=None`` (``MHMR_ADAM_PACK_NONE``):
    ``encoder_jobs`` writes those.  With nothing packed, or an fp8 low-half pack (``MHMR_LO8=1``), every ``kind`` is None."""
    from .backbone_train import BLOCK_FIELDS, ENCODER
    P = model._packed if P is None else P
    live = _derived(P)
    x3, fold, Kp = (bool(P.get("x3")), bool(P["fold"]), P["Kp"]) if live else (False, False, 0)
    field_of = {v: k for k, v in BLOCK_FIELDS.items()}
    segs = []

    def seg(param, target, kind, cols=1, pitch=1):
        segs.append(dict(param=param, param2=None, target=target, offset=0, cols=cols, pitch=pitch, kind=kind if live else None, addend=None))

    for name in _encoder_names(model):
        short = name[len(ENCODER):]
        if short.startswith("norm."):
            seg(name, ("norm", "norm_w" if short == "norm.weight" else "norm_b"), "f32")
        elif short.startswith("blocks."):
            _, l, rest = short.split(".", 2)
            l, f = int(l), field_of[rest]
            folded = fold and ((f in ("qkv_w", "qkv_b") and l > 0) or f in ("fc1_w", "fc1_b"))
            if f.endswith("_w") and not f.startswith("ln"):
                seg(name, ("block", l, f), None if (x3 or folded) else "op16")
            else:
                seg(name, ("block", l, f), None if folded else "f32")
        elif short == "patch_embed.proj.weight":
            seg(name, ("embed", "patch_w"), None if x3 else "op16", cols=588, pitch=Kp if live else 588)
        elif short == "patch_embed.proj.bias":
            seg(name, ("embed", "patch_b"), "f32")
        else:                                            # pos_embed, cls_token: the resampled table and the class row
            seg(name, ("embed", "pos" if short == "pos_embed" else "cls_pos0"), None)
    return segs


def encoder_jobs(model, P=None) -> list:
    """The ``mhmr_vit_repack`` jobs of the derived operands of the pack ``P`` (default: the model's), in words -- one dict per job, the row
    jobs first.  Row job: ``kind="row"``, ``w`` (weight parameter name), ``rows`` ((first row, count) of it the job covers), ``K``, ``ln``
    ((weight, bias) names of the folded LayerNorm, or None), ``bias`` (name, or None), ``w16`` / ``bias_out`` / ``colsum`` / ``lo`` (targets
    as in ``encoder_segments``, or None), ``lo_form`` (None, "pair" = [hi | lo], "triple" = [hi | lo | hi]), ``lo_rows`` ((first, count)
    among the job's rows), ``section`` (elements between the sections of a ``lo`` row).  Position job: ``kind="pos"``, ``pos_embed``,
    ``cls_token`` (names), ``pos``, ``cls_pos0`` (targets), ``M``, ``G``.  ``params``: the parameters a job reads -- it runs in a step
    that updated any of them.  Empty with nothing packed or an fp8 low-half pack."""
    from .backbone_train import BLOCK_FIELDS, ENCODER
    P = model._packed if P is None else P
    if not _derived(P):
        return []
    enc = model.backbone.encoder
    L, Cd, x3, fold = len(enc.blocks), P["C"], bool(P.get("x3")), bool(P["fold"])
    jobs = []

    def row(l, f, ln=None, rows=None, w16=False, lo=None, lo_form=None, lo_rows=None, folded=False):
        w = f"{ENCODER}blocks.{l}.{BLOCK_FIELDS[f]}"
        N, K = dict(model.named_parameters())[w].shape
        rows = (0, N) if rows is None else rows
        lnn = (f"{ENCODER}blocks.{l}.{ln}.weight", f"{ENCODER}blocks.{l}.{ln}.bias") if folded else None
        bias = w[:-len("weight")] + "bias" if folded else None
        fb = f[:-2]
        jobs.append(dict(kind="row", w=w, rows=rows, K=K, ln=lnn, bias=bias, w16=("block", l, f) if w16 else None,
                         bias_out=("block", l, fb + "_b") if folded else None, colsum=("block", l, fb + "_colsum") if folded else None,
                         lo=lo, lo_form=lo_form, lo_rows=(0, rows[1]) if (lo is not None and lo_rows is None) else lo_rows, section=K,
                         params=[w] + (list(lnn) + [bias] if folded else [])))

    for l in range(L - model._backbone_n, L):
        if x3:
            for f in ("qkv_w", "proj_w", "fc1_w", "fc2_w"):
                row(l, f, lo=("block", l, f), lo_form="triple")
            continue
        passes = P["lo_passes"].get(l, ())
        v2 = ("block", l, "v_w2") if "v" in passes else None
        if fold and l > 0:
            row(l, "qkv_w", ln="norm1", w16=True, folded=True, lo=v2, lo_form="pair" if v2 else None, lo_rows=(2 * Cd, Cd) if v2 else None)
        elif v2:
            row(l, "qkv_w", rows=(2 * Cd, Cd), lo=v2, lo_form="pair")
        if "proj" in passes:
            row(l, "proj_w", lo=("block", l, "proj_w2"), lo_form="pair")
        if fold:
            row(l, "fc1_w", ln="norm2", w16=True, folded=True)
    if any(p.requires_grad for p in model.embedding_parameters()):
        if x3:
            w = ENCODER + "patch_embed.proj.weight"
            jobs.append(dict(kind="row", w=w, rows=(0, Cd), K=588, ln=None, bias=None, w16=None, bias_out=None, colsum=None,
                             lo=("embed", "patch_w"), lo_form="triple", lo_rows=(0, Cd), section=P["Kp"], params=[w]))
        M = int(round((enc.pos_embed.shape[1] - 1) ** 0.5))
        jobs.append(dict(kind="pos", pos_embed=ENCODER + "pos_embed", cls_token=ENCODER + "cls_token", pos=("embed", "pos"),
                         cls_pos0=("embed", "cls_pos0"), M=M, G=P["G"], params=[ENCODER + "pos_embed", ENCODER + "cls_token"]))
    return jobs


def job_bytes(jobs) -> int:
    """Bytes a ``mhmr_vit_repack`` call moves for a host table of ``_lib.PackJob``: per row job the fp32 weight read once, the LayerNorm
    vectors (cached: counted once per job), each 16-bit section written, bias and column sum; per position job 16 source rows read per
    output row (an upper bound: neighbours share them in cache) and the table written."""
    total = 0
    for j in jobs:
        if j.kind == _lib.PACK_ROW:
            sections = {_lib.PACK_LO_NONE: 0, _lib.PACK_LO_PAIR: 2, _lib.PACK_LO_TRIPLE: 3}[j.lo_form]
            total += 4 * j.N * j.K + (8 * j.K if j.ln_w else 0) + (2 * j.N * j.K if j.w16 else 0) + 2 * sections * j.lo_rows * j.K
            total += (8 * j.N if j.bias_out else 0) + (4 * j.N if j.colsum else 0)
        else:
            total += 4 * j.C * (1 + j.G * j.G) * (1 if j.G == j.M else 17) + 12 * j.C
    return total


class ModelAdam(HeadsAdam):
    """Adam over the whole model -- ``heads_parameters()`` + ``detection_parameters()`` (with ``detection=True``) +
    ``backbone_parameters(model._backbone_n)`` + ``embedding_parameters()`` (when they require grad at construction): the list and the
    order of the command line's ``torch.optim.Adam``, the same state layout (a ``state_dict()`` moves between the two in both directions),
    the same refusals as ``HeadsAdam``.  Call ``train_backbone_(n)`` / ``train_embeddings_()`` first.

    ``step()``, under the model's lock: ONE ``mhmr_adam_step`` call over ``head_segments`` + ``encoder_segments`` (with ``max_grad_norm``
    the clip is global over the whole table), then ONE ``mhmr_vit_repack`` call with the ``encoder_jobs`` whose parameters were stepped:
    folded linears with their biases and column sums, ``[hi | lo]`` rows, f16x3 triples, the resampled position table.  A block without a
    gradient keeps its bits.  Nothing goes to the host; the bicubic taps are made once per pack.  ``heads_generation`` moves, and
    ``backbone_generation`` when an encoder parameter was stepped, as ``repack_heads()`` / ``repack_backbone()`` move them.  Before the
    first forward it updates the parameters only.

    After ``step()`` the packed encoder holds what ``repack_backbone()`` writes from the updated parameters, bit for bit -- except the
    entries that are fp64 sums (folded biases, bf16 column sums, the resampled position table): the kernels add them in a fixed order,
    torch and numpy in an order of their own, and the fp32 results may differ in the last bit.  So a model reloaded from ``state_dict()``
    may differ from the stepped one in the last bit of such an entry (DESIGN.md section 34 has the measured counts).

    An fp8 low-half pack (``MHMR_LO8=1``) has no device jobs: ``step()`` does the Adam launch and then calls ``repack_backbone()``."""

    def _parameter_names(self):
        return super()._parameter_names() + _encoder_names(self.model)

    def _specs(self, P):
        from .backbone_train import ENCODER
        enc = encoder_segments(self.model, P)
        if [s["param"] for s in enc] != [n for n in self._names if n.startswith(ENCODER)]:
            raise _lib.MhmrError("ModelAdam: train_backbone_() / train_embeddings_() changed the trained encoder parameters after this "
                                 "optimiser was made; make a new one")
        return head_segments(self.model, self.detection) + enc

    def _build(self, P, dev):
        from .backbone_train import ENCODER
        tab = super()._build(P, dev)
        specs = encoder_jobs(self.model, P)
        named = dict(self.model.named_parameters())
        tab["encoder"] = {n for n in self._names if n.startswith(ENCODER)}
        tab["jobs"] = []
        for s in specs:
            j = _lib.PackJob()
            if s["kind"] == "pos":
                t_pos, t_cls = packed_target(P, s["pos"]), packed_target(P, s["cls_pos0"])
                M, G, Cd = s["M"], s["G"], t_pos.shape[1]
                if t_pos.shape != (1 + G * G, Cd) or t_cls.numel() != Cd or named[s["pos_embed"]].shape != (1, 1 + M * M, Cd):
                    raise _lib.MhmrError("ModelAdam: the packed position table is not laid out as vit.pack_embeddings makes it")
                j.kind, j.M, j.G, j.C, j.pos, j.cls_pos0 = _lib.PACK_POS, M, G, Cd, t_pos.data_ptr(), t_cls.data_ptr()
                if G != M:
                    if "taps" not in tab:
                        from . import packing
                        w, idx = packing._cubic_taps(M, G)
                        tab["taps"] = (torch.from_numpy(w).to(dev).contiguous(), torch.from_numpy(idx.astype("int32")).to(dev).contiguous())
                    j.tap_w, j.tap_i = tab["taps"][0].data_ptr(), tab["taps"][1].data_ptr()
                tab["jobs"].append(dict(job=j, spec=s, p=dict(pos_embed=named[s["pos_embed"]], cls_token=named[s["cls_token"]])))
                continue
            (r0, N), K = s["rows"], s["K"]
            j.kind, j.dtype, j.N, j.K = _lib.PACK_ROW, (_lib.ADAM_PACK_F16 if P["tdt"] == torch.float16 else _lib.ADAM_PACK_BF16), N, K
            keep = []

            def tgt(target, dtype, numel):
                t = packed_target(P, target)
                if t is None or t.dtype != dtype or not t.is_contiguous() or t.numel() < numel:
                    raise _lib.MhmrError(f"ModelAdam: the packed tensor {target} is not laid out as vit.pack_block makes it")
                keep.append(t)
                return t.data_ptr()
            if s["w16"] is not None:
                j.w16, j.pitch16 = tgt(s["w16"], P["tdt"], N * K), K
            if s["lo"] is not None:
                sections = 2 if s["lo_form"] == "pair" else 3
                j.lo_form = _lib.PACK_LO_PAIR if sections == 2 else _lib.PACK_LO_TRIPLE
                (j.lo_row0, j.lo_rows), j.lo_section, j.lo_pitch = s["lo_rows"], s["section"], sections * s["section"]
                j.lo = tgt(s["lo"], P["tdt"], j.lo_rows * j.lo_pitch)
            if s["bias_out"] is not None:
                j.bias_out, j.colsum = tgt(s["bias_out"], torch.float32, N), tgt(s["colsum"], torch.float32, N)
            p = dict(w=named[s["w"]])
            if s["ln"]:
                p.update(ln_w=named[s["ln"][0]], ln_b=named[s["ln"][1]], bias=named[s["bias"]])
            tab["jobs"].append(dict(job=j, spec=s, p=p, keep=keep, w_offset=r0 * K * 4))
        n = max(len(tab["jobs"]), 1)
        tab["jobs_host"] = (_lib.PackJob * n)()
        tab["jobs_device"] = torch.empty(C.sizeof(tab["jobs_host"]), dtype=torch.uint8, device=dev)
        return tab

    def _active_jobs(self, tab):
        """Fill the host job table with the jobs that read a parameter stepped in this call; -> their count."""
        host, stepped = tab["jobs_host"], tab["stepped_names"]
        n = rows = prow = 0
        for e in tab["jobs"]:
            if stepped.isdisjoint(e["spec"]["params"]):
                continue
            j = e["job"]
            for k, p in e["p"].items():
                self._check(p, e["spec"]["params"][0])
                setattr(j, k, p.data_ptr() + (e["w_offset"] if k == "w" else 0))
            if j.kind == _lib.PACK_ROW:
                j.row0, rows = rows, rows + j.N
            else:
                j.row0, prow = prow, prow + 1 + j.G * j.G
            C.memmove(C.addressof(host) + n * C.sizeof(_lib.PackJob), C.addressof(j), C.sizeof(_lib.PackJob))
            n += 1
        return n

    def _after_step(self, tab, P, stream):
        super()._after_step(tab, P, stream)
        if P is None or tab["stepped_names"].isdisjoint(tab["encoder"]):
            return
        if not _derived(P):
            self.model.repack_backbone()                 # (an fp8 low-half pack: the host re-pack, which moves the counter itself)
            return
        n = tab["njobs"] = self._active_jobs(tab)
        if n:
            nbytes = n * C.sizeof(_lib.PackJob)
            with torch.cuda.device(tab["dev"]):
                stage = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
                C.memmove(stage.data_ptr(), C.addressof(tab["jobs_host"]), nbytes)
                tab["jobs_device"][:nbytes].copy_(stage, non_blocking=True)
                _lib.check(_lib.lib().mhmr_vit_repack(tab["jobs_host"], tab["jobs_device"].data_ptr(), n, stream), "mhmr_vit_repack")
        P["backbone_generation"] += 1


__all__ = ["HeadsAdam", "ModelAdam", "head_segments", "encoder_segments", "encoder_jobs", "packed_target", "bias_corrections", "table_bytes",
           "job_bytes"]
