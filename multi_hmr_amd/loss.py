"""Training loss of the reference (loss.py) on the device: ``Loss`` is a drop-in for the reference's class, ``loss_and_grads`` the
functional form the backward kernels start from.

The eleven values -- ``total, bce, offset, rotmat, shape, dist, transl, j3d, v3d, j2d, v2d`` -- and the gradient of ``total`` with
respect to every prediction come from ``mhmr_loss_forward`` / ``mhmr_loss_backward`` (csrc/loss.hip): one streaming pass each, fp32
elements in the reference's operation order, fp64 sums in a fixed order, no host synchronisation anywhere (the reference's
``if num_pos == 0`` and ``torch.where`` are decided on the device).

Differences from the reference, all deliberate:
  * a term that is NaN or +-inf becomes 0 (as the reference's ``nan_to_num``) AND all its gradients are 0 -- torch gives 0 behind an
    inf and NaN behind a NaN; one bad element should not poison a training step;
  * only ``total`` carries an autograd graph; the ``dict_loss`` entries (``dict_loss['total']`` included) are detached 0-d device
    tensors -- the reference's ``.item()`` calls stay with the caller;
  * a ``y_hat`` that holds only ``scores`` (a batch without persons) is accepted: the person terms are 0;
  * a ground truth whose ``v3d`` / ``j3d`` has another vertex / joint count than the prediction (the SMPL meshes of 3DPW) raises
    instead of failing inside a subtraction.
"""
from __future__ import annotations

import ctypes as C
from argparse import ArgumentParser

import torch

from . import _lib

#: the keys of ``dict_loss``, in the reference's order (= the order of the values in the device block)
LOSS_KEYS = ("total", "bce", "offset", "rotmat", "shape", "dist", "transl", "j3d", "v3d", "j2d", "v2d")
#: ``y_hat`` / ``y`` key of every tensor of ``_lib.LossDesc.TENSORS``
_KEYS = {"dist": "dist_postprocessed", "pelvis": "transl_pelvis"}
_ALPHAS = ("alpha_bce", "alpha_offset", "alpha_rotmat", "alpha_shape", "alpha_dist", "alpha_transl", "alpha_j3d", "alpha_v3d",
           "alpha_j2d", "alpha_v2d")


def _f32c(t):
    """fp32, contiguous (a no-op for what Model and GroundTruth return, except the transl_pelvis view of j3d)."""
    return t.detach().to(torch.float32).contiguous()


class _Prepared:
    """The tensors of one call, checked and laid out for the C entry, and its descriptor."""

    def __init__(self, y_hat, y, epoch, img_size, args):
        if epoch is None or img_size is None:
            raise _lib.MhmrError("Loss.forward needs epoch= and img_size= (loss.py:70, 96)")
        sh = y_hat["scores"]
        dev = sh.device
        if dev.type != "cuda":
            raise _lib.MhmrError("the loss runs on the HIP device only (no CPU fallback)")
        self.dev = dev
        self.hat, self.gt = {"scores": _f32c(sh)}, {"scores": _f32c(y["scores"].to(dev))}
        if sh.dim() != 4 or sh.shape[-1] != 1 or sh.shape[1] != sh.shape[2] or tuple(self.gt["scores"].shape) != tuple(sh.shape[:3]):
            raise _lib.MhmrError(f"scores: prediction {tuple(sh.shape)} must be [B,G,G,1] and the target {tuple(y['scores'].shape)} [B,G,G]")
        B, G = int(sh.shape[0]), int(sh.shape[1])
        P = int(y_hat["v3d"].shape[0]) if "v3d" in y_hat else 0
        V = J = nrot = nb_hat = nb_gt = 1
        if P > 0:
            for n in _lib.LossDesc.TENSORS[1:]:
                k = _KEYS.get(n, n)
                if k not in y:
                    raise _lib.MhmrError(f"the ground truth has no '{k}' (annotations without body-model parameters carry no rotmat / shape)")
                self.hat[n], self.gt[n] = _f32c(y_hat[k]), _f32c(y[k].to(dev))
            V, J = int(self.hat["v3d"].shape[1]), int(self.hat["j3d"].shape[1])
            if tuple(self.gt["v3d"].shape) != (P, V, 3):
                raise _lib.MhmrError(f"the ground truth's v3d {tuple(self.gt['v3d'].shape)} is not the prediction's {(P, V, 3)}: an SMPL "
                                     "ground truth (3DPW) cannot be compared vertex by vertex with an SMPL-X prediction")
            if tuple(self.gt["j3d"].shape) != (P, J, 3):
                raise _lib.MhmrError(f"the ground truth's j3d {tuple(self.gt['j3d'].shape)} is not the prediction's {(P, J, 3)}")
            nrot = self.hat["rotmat"].numel() // P
            nb_hat, nb_gt = int(self.hat["shape"].shape[1]), int(self.gt["shape"].shape[1])
            want = {"offset": (2,), "rotmat": None, "shape": None, "dist": (), "transl": (3,), "pelvis": (3,), "j3d": (J, 3), "v3d": (V, 3),
                    "j2d": (J, 2), "v2d": (V, 2)}
            for n, shp in want.items():
                for side, t in (("prediction", self.hat[n]), ("ground truth", self.gt[n])):
                    if t.shape[0] != P or (shp is not None and t.numel() != P * int(torch.Size(shp).numel())):
                        raise _lib.MhmrError(f"{side} '{_KEYS.get(n, n)}' has shape {tuple(t.shape)} for {P} persons")
            if self.gt["rotmat"].numel() != P * nrot:
                raise _lib.MhmrError(f"rotmat: prediction {tuple(self.hat['rotmat'].shape)} against ground truth {tuple(self.gt['rotmat'].shape)}")
        d = _lib.LossDesc()
        for n in self.hat:
            setattr(d, n + "_hat", self.hat[n].data_ptr())
            setattr(d, n, self.gt[n].data_ptr())
        d.B, d.G, d.P, d.V, d.J, d.nrot, d.nb_hat, d.nb_gt = B, G, P, V, J, nrot, nb_hat, nb_gt
        d.img_size = float(img_size)
        d.use_2d = int(epoch >= args.start_2d_epoch)
        for i, a in enumerate(_ALPHAS):
            d.alpha[i] = float(getattr(args, a))
        self.desc, self.P = d, P
        self.out = None

    def forward(self):
        """-> the 32-word device block of mhmr_loss_forward (values, counts, finite flags) as an fp32 tensor."""
        L = _lib.lib()
        with torch.cuda.device(self.dev):
            ws = torch.empty(L.mhmr_loss_workspace_bytes() // 8, dtype=torch.float64, device=self.dev)
            self.out = torch.empty(_lib.LOSS_OUT_BYTES // 4, dtype=torch.float32, device=self.dev)
            _lib.check(L.mhmr_loss_forward(C.byref(self.desc), ws.data_ptr(), ws.numel() * 8, self.out.data_ptr(),
                                           torch.cuda.current_stream(self.dev).cuda_stream), "mhmr_loss_forward")
        return self.out

    def backward(self, grad_total, names):
        """Gradients of ``total`` for the tensors ``names`` (of ``_lib.LossDesc.TENSORS``) -> dict name -> tensor shaped like the
        prepared prediction."""
        L = _lib.lib()
        names = [n for n in names if n in self.hat]
        with torch.cuda.device(self.dev):
            grads = {n: torch.empty_like(self.hat[n]) for n in names}
            g = _lib.LossGrads()
            for n, t in grads.items():
                setattr(g, n, t.data_ptr())
            gt = grad_total.detach().to(device=self.dev, dtype=torch.float32).reshape(1).contiguous()
            _lib.check(L.mhmr_loss_backward(C.byref(self.desc), self.out.data_ptr(), gt.data_ptr(), C.byref(g),
                                            torch.cuda.current_stream(self.dev).cuda_stream), "mhmr_loss_backward")
        return grads


def _dict(vals):
    return {k: vals[i] for i, k in enumerate(LOSS_KEYS)}


def loss_and_grads(y_hat, y, epoch, img_size, args, grad_total=None):
    """The functional form, without autograd: one forward and one backward launch set.  -> ``(dict_loss, grads)``: the eleven values
    as 0-d device tensors and ``d total / d y_hat[key]`` for every person key the loss reads (plus ``scores``), shaped like
    ``y_hat[key]``.  ``grad_total``: the upstream gradient of ``total`` (a 0-d tensor; default 1)."""
    pr = _Prepared(y_hat, y, epoch, img_size, args)
    vals = pr.forward()[:11]
    if grad_total is None:
        grad_total = torch.ones((), device=pr.dev)
    grads = pr.backward(grad_total, _lib.LossDesc.TENSORS)
    return _dict(vals), {_KEYS.get(n, n): t.view(y_hat[_KEYS.get(n, n)].shape) for n, t in grads.items()}


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pr, names, *tensors):
        ctx.pr, ctx.names = pr, names
        ctx.meta = [(t.shape, t.dtype) for t in tensors]
        vals = pr.forward()[:11]
        ctx.mark_non_differentiable(vals)
        return vals[0].clone(), vals

    @staticmethod
    def backward(ctx, g_total, _g_vals):
        need = [n for n, w in zip(ctx.names, ctx.needs_input_grad[2:]) if w]
        grads = ctx.pr.backward(g_total, need)
        out = [grads[n].view(shp).to(dt) if n in grads else None for n, (shp, dt) in zip(ctx.names, ctx.meta)]
        return (None, None, *out)


class Loss(torch.nn.Module):
    """Drop-in for the reference's ``loss.Loss``: ``forward(y_hat, y, epoch=None, img_size=None) -> (total, dict_loss)``.
    ``total.backward()`` fills ``.grad`` of whichever ``y_hat`` tensors require grad (a ``transl_pelvis`` that is a view of ``j3d``
    accumulates into ``j3d.grad[:, 0]`` through autograd as usual).  Only ``total`` carries a graph: the ``dict_loss`` entries are
    detached 0-d device tensors, and nothing here synchronises with the host."""

    def __init__(self, parser_args, *args, **kwargs):
        super().__init__()
        self.parser_args = parser_args

    def forward(self, y_hat, y, epoch=None, img_size=None):
        pr = _Prepared(y_hat, y, epoch, img_size, self.parser_args)
        names = tuple(pr.hat)
        total, vals = _LossFn.apply(pr, names, *(y_hat[_KEYS.get(n, n)] for n in names))
        return total, _dict(vals)

    @staticmethod
    def add_specific_args(parent_parser):
        parser = ArgumentParser(parents=[parent_parser], add_help=False)
        parser.add_argument("--alpha_bce", type=float, default=10.0)          # detection
        parser.add_argument("--alpha_offset", type=float, default=1.0)
        parser.add_argument("--alpha_rotmat", type=float, default=0.1)        # SMPL-X parameters
        parser.add_argument("--alpha_shape", type=float, default=1.0)
        parser.add_argument("--alpha_dist", type=float, default=1.0)
        parser.add_argument("--alpha_transl", type=float, default=1.0)
        parser.add_argument("--alpha_j3d", type=float, default=100.0)         # 3D points
        parser.add_argument("--alpha_v3d", type=float, default=100.0)
        parser.add_argument("--alpha_j2d", type=float, default=1.0)           # 2D reprojection
        parser.add_argument("--alpha_v2d", type=float, default=1.0)
        parser.add_argument("--start_2d_epoch", type=int, default=10)
        return parser
