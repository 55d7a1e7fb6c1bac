"""Drop-in for the Anny-variant Human Perception Head ``multi_hmr_anny.hph.HPH`` (reference multi_hmr_anny/hph.py:142-151):
the same pre-norm (self-attention, cross-attention, feed-forward) stack as the Multi-HMR HPH with other constants
(dim 512, 16 heads x 32, mlp 2048, depth 8, context_dim = dim, no mask multiplies) -- SURVEY.md section 8 row a10.
Same constructor, same ``state_dict`` keys, same ``forward(x, context, mask)``; compute = ``mhmr_xattn_layers_forward``."""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib, packing
from .model import _ca, _ff, _Holder, _PreNorm, _sa
from .packing import roundup


class _Stack(_Holder):
    def __init__(self, dim, depth, heads, dim_head, mlp_dim):
        super().__init__()
        inner = heads * dim_head
        self.layers = nn.ModuleList([nn.ModuleList([_PreNorm(dim, _sa(dim, inner)), _PreNorm(dim, _ca(dim, dim, inner)),
                                                    _PreNorm(dim, _ff(dim, mlp_dim))]) for _ in range(depth)])


class HPH(nn.Module):
    def __init__(self, dim, depth, heads, dim_head, mlp_dim, dropout=0.0, precision="f16"):
        super().__init__()
        if dim_head != 32:
            raise NotImplementedError("the attention kernels are built for dim_head = 32 (both released HPH variants)")
        if dropout:
            raise NotImplementedError("inference path: dropout must be 0")
        self.dim, self.depth, self.heads, self.mlp_dim, self.precision = dim, depth, heads, mlp_dim, precision
        self.transformer = _Stack(dim, depth, heads, dim_head, mlp_dim)
        self._packed = None
        for p in self.parameters():
            p.requires_grad_(False)

    def load_state_dict(self, *a, **k):
        self._packed = None
        return super().load_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def _pack(self, device):
        dt_id, tdt = packing.OP_DTYPES[self.precision]
        f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()
        keep, layers = [], (_lib.HphLayer * self.depth)()

        def k(t):
            keep.append(t)
            return t.data_ptr()
        Kc = roundup(self.dim, 64)
        for l, (sa, ca, ff) in enumerate(self.transformer.layers):
            y = layers[l]
            y.ln_sa_w, y.ln_sa_b, y.to_qkv = k(f32(sa.norm.weight)), k(f32(sa.norm.bias)), k(f32(sa.fn.to_qkv.weight))
            y.sa_out_w, y.sa_out_b = k(f32(sa.fn.to_out[0].weight)), k(f32(sa.fn.to_out[0].bias))
            y.ln_ca_w, y.ln_ca_b = k(f32(ca.norm.weight)), k(f32(ca.norm.bias))
            kvw = torch.zeros(64 * self.heads, Kc, device=device)
            kvw[:, : self.dim] = f32(ca.fn.to_kv.weight)
            y.to_kv16, y.to_q = k(kvw.to(tdt).contiguous()), k(f32(ca.fn.to_q.weight))
            y.ca_out_w, y.ca_out_b = k(f32(ca.fn.to_out[0].weight)), k(f32(ca.fn.to_out[0].bias))
            y.ln_ff_w, y.ln_ff_b = k(f32(ff.norm.weight)), k(f32(ff.norm.bias))
            y.ff1_w, y.ff1_b = k(f32(ff.fn.net[0].weight)), k(f32(ff.fn.net[0].bias))
            y.ff2_w, y.ff2_b = k(f32(ff.fn.net[3].weight)), k(f32(ff.fn.net[3].bias))
        self._packed = dict(device=device, dt_id=dt_id, tdt=tdt, layers=layers, keep=keep, Kc=Kc)
        return self._packed

    def repack(self):
        """Drop the packed fp32 / 16-bit copies of the weights: the next call packs the parameters again (after an optimiser step)."""
        self._packed = None

    #: (packed field of mhmr_hph_layer, parameter) in the order of _lib.HphLayerGrads.FIELDS
    def _layer_params(self):
        out = []
        for sa, ca, ff in self.transformer.layers:
            out.append([sa.norm.weight, sa.norm.bias, sa.fn.to_qkv.weight, sa.fn.to_out[0].weight, sa.fn.to_out[0].bias, ca.norm.weight,
                        ca.norm.bias, ca.fn.to_kv.weight, ca.fn.to_q.weight, ca.fn.to_out[0].weight, ca.fn.to_out[0].bias, ff.norm.weight,
                        ff.norm.bias, ff.fn.net[0].weight, ff.fn.net[0].bias, ff.fn.net[3].weight, ff.fn.net[3].bias])
        return out

    def _prepare(self, x, context, mask):
        """Ragged rows, the work tables and the 16-bit context operand of one call (shared by forward and differentiable)."""
        if not x.is_cuda:
            raise _lib.MhmrError("multi_hmr_amd.anny_hph.HPH runs only on an MI355X (HIP) tensor; there is no CPU fallback")
        P_ = self._packed if self._packed is not None and self._packed["device"] == x.device else self._pack(x.device)
        dev, (Bp, nmax, dim), N = x.device, x.shape, context.shape[1]
        assert dim == self.dim and context.shape == (Bp, N, dim)
        if mask is None:
            mask = torch.ones(Bp, nmax, device=dev)
        counts = [int(c) for c in mask.sum(1).round().long().tolist()]
        keep_rows = mask.reshape(-1) > 0.5
        gstart, chunks, start = [0], [], 0
        for b, c in enumerate(counts):
            if c == 0:
                continue
            for q0 in range(0, c, 8):
                chunks += [b, start + q0, min(8, c - q0)]
            start += c
            gstart.append(start)
        st = dict(P_=P_, dev=dev, Bp=Bp, nmax=nmax, dim=dim, N=N, counts=counts, keep_rows=keep_rows, Pn=start, gstart=gstart, chunks=chunks)
        if start == 0:
            return st
        st["meta"] = torch.tensor(gstart + chunks, dtype=torch.int32).to(dev)
        Kc = P_["Kc"]
        Mctx = roundup(Bp * N, 128)
        ctx16 = torch.zeros(Mctx, Kc, dtype=P_["tdt"], device=dev)
        ctx16[: Bp * N, :dim] = context.detach().reshape(Bp * N, dim).float().to(P_["tdt"])
        st.update(Kc=Kc, Mctx=Mctx, ctx16=ctx16)
        return st

    def _run(self, st, xr):
        """mhmr_xattn_layers_forward on the ragged rows xr [P, dim], in place."""
        P_, dev, dim, inner = st["P_"], st["dev"], st["dim"], 32 * self.heads
        Pn, ng = st["Pn"], len(st["gstart"])
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        xn, t1, t2, kv = f(Pn, dim), f(Pn, max(3 * inner, self.mlp_dim)), f(Pn, inner), f(st["Mctx"], 2 * inner)
        _lib.check(_lib.lib().mhmr_xattn_layers_forward(C.cast(P_["layers"], C.POINTER(_lib.HphLayer)), self.depth, dim, self.heads,
                                                        self.mlp_dim, st["Kc"], st["N"], st["Bp"], P_["dt_id"], xr.data_ptr(), xn.data_ptr(),
                                                        t1.data_ptr(), t2.data_ptr(), kv.data_ptr(), st["ctx16"].data_ptr(),
                                                        st["meta"][:ng].data_ptr(), ng - 1, max(st["counts"]), st["meta"][ng:].data_ptr(),
                                                        len(st["chunks"]) // 3, Pn, torch.cuda.current_stream(dev).cuda_stream),
                   "mhmr_xattn_layers_forward")
        return xr

    @torch.no_grad()
    def forward(self, x, context, mask=None):
        """x [B', nmax, dim] padded queries, context [B', N, dim], mask [B', nmax] (1 = real query) -> [B', nmax, dim].
        Real rows equal the reference's; padded rows (garbage in the reference, dropped by its caller at
        multi_hmr_anny/multi_hmr.py:141) are returned as zeros."""
        with torch.autocast("cuda", enabled=False):
            st = self._prepare(x, context, mask)
            out = torch.zeros(st["Bp"], st["nmax"], st["dim"], device=st["dev"])
            if st["Pn"] == 0:
                return out
            xr = x.reshape(st["Bp"] * st["nmax"], st["dim"])[st["keep_rows"]].float().contiguous()              # ragged [P, dim]
            out.reshape(st["Bp"] * st["nmax"], st["dim"])[st["keep_rows"]] = self._run(st, xr)
            return out

    def differentiable(self, x, context, mask=None):
        """``forward`` attached to autograd with respect to ``x`` and the stack's parameters (those that require grad): the same
        launches, hence the same bits; ``backward`` is ``mhmr_xattn_layers_backward``.  ``context`` gets no
        gradient.  The gradient of ``to_kv.weight`` is that of the weight rounded to the 16-bit operand type (straight-through).  The
        packed copies of the weights are the ones the forward ran with: after changing a parameter in place call ``repack()``.  With no
        real query at all the output is zeros and every gradient is zero."""
        with torch.autocast("cuda", enabled=False):
            st = self._prepare(x, context, mask)
            rows = torch.nonzero(st["keep_rows"]).reshape(-1)
            xr = x.reshape(st["Bp"] * st["nmax"], st["dim"]).index_select(0, rows).float().contiguous()
            flat = [p for layer in self._layer_params() for p in layer]
            y = _StackFn.apply(self, st, xr, *flat)
            out = torch.zeros(st["Bp"] * st["nmax"], st["dim"], device=st["dev"]).index_put((rows,), y)
            return out.reshape(st["Bp"], st["nmax"], st["dim"])


class _StackFn(torch.autograd.Function):
    """mhmr_xattn_layers_forward / mhmr_xattn_layers_backward on ragged rows."""

    @staticmethod
    def forward(ctx, hph, st, xr, *params):
        ctx.hph, ctx.st = hph, st
        x0 = xr.detach()
        ctx.save_for_backward(x0)
        ctx.shapes = [tuple(p.shape) for p in params]
        if st["Pn"] == 0:
            return x0.clone()
        return hph._run(st, x0.clone())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        hph, st = ctx.hph, ctx.st
        (x0,) = ctx.saved_tensors
        dev, dim, Pn = st["dev"], st["dim"], st["Pn"]
        need = ctx.needs_input_grad[3:]
        if Pn == 0:
            return (None, None, torch.zeros_like(x0)) + tuple(torch.zeros(s, device=dev) if n else None for s, n in zip(ctx.shapes, need))
        P_, L, inner, Kc = st["P_"], _lib.lib(), 32 * hph.heads, st["Kc"]
        F = _lib.HphLayerGrads.FIELDS
        grads, bufs = (_lib.HphLayerGrads * hph.depth)(), []
        for l in range(hph.depth):
            row = []
            for i, name in enumerate(F):
                shape = (2 * inner, Kc) if name == "to_kv" else ctx.shapes[l * len(F) + i]
                t = torch.empty(shape, dtype=torch.float32, device=dev)
                setattr(grads[l], name, t.data_ptr())
                row.append(t)
            bufs.append(row)
        nbytes = _lib.workspace_bytes("mhmr_xattn_layers_backward_workspace_bytes", hph.depth, dim, hph.heads, hph.mlp_dim, Kc, st["N"], st["Bp"], Pn)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        g = g.float().contiguous()
        g_x0 = torch.empty(Pn, dim, dtype=torch.float32, device=dev)
        ng = len(st["gstart"])
        d = _lib.XattnBackwardDesc(layers=C.cast(P_["layers"], C.POINTER(_lib.HphLayer)), grads=C.cast(grads, C.POINTER(_lib.HphLayerGrads)),
                                   depth=hph.depth, dim=dim, heads=hph.heads, mlp=hph.mlp_dim, Kc=Kc, N=st["N"], B=st["Bp"], dtype=P_["dt_id"],
                                   P=Pn, ngroups=ng - 1, nmax=max(st["counts"]), nchunks=len(st["chunks"]) // 3, ctx_valid=dim,
                                   x0=x0.data_ptr(), ctx16=st["ctx16"].data_ptr(), gstart=st["meta"][:ng].data_ptr(),
                                   chunks=st["meta"][ng:].data_ptr(), g_x_out=g.data_ptr(), g_x0=g_x0.data_ptr(), workspace=ws.data_ptr(),
                                   workspace_bytes=nbytes)
        _lib.check(L.mhmr_xattn_layers_backward(C.byref(d), torch.cuda.current_stream(dev).cuda_stream), "mhmr_xattn_layers_backward")
        out = []
        for l in range(hph.depth):
            for i, name in enumerate(F):
                t = bufs[l][i]
                if name == "to_kv":
                    t = t[:, :dim].contiguous()
                out.append(t if need[l * len(F) + i] else None)
        return (None, None, g_x0) + tuple(out)
