"""``Trainer``: the loop around the training step -- epochs, meters, the log line, checkpoints, evaluation -- with the surface of the
reference's ``train.py`` ``Trainer``, for what this package trains.

Two differences from the reference, both on purpose:

* by default it trains the heads (``x_attention_head``, ``mlp_offset``) and the detector (``mlp_classif``) on a FROZEN backbone, so the
  optimiser holds ``model.heads_parameters()`` (+ ``model.detection_parameters()``), not ``model.parameters()``; ``--train_backbone N``
  adds the final norm and the last N encoder blocks (and, with N = the depth, the token embedding) under ``torch.optim.Adam``, or
  under ``ModelAdam`` with ``--fused_adam 1``;
* the master weights are fp32 and there is no autocast: the 16-bit operands of the forward are the model's packed copies, which the
  optimiser step rewrites (``HeadsAdam``, ``ModelAdam``) or ``repack_heads()`` / ``repack_backbone()`` refresh (any other ``torch.optim`` optimiser).
  ``--amp 1`` (the reference's default) gives the linears of the backbone BACKWARD bf16 operands with fp32 accumulation (DESIGN.md
  section 30), ``--amp_attention 1`` (default 0) its attention tape and backward as well (section 31); the heads' backward and every
  forward are what they are without them.

The step has one legal order -- forward, ``decode_readout``, loss, ``backward()``, optimiser step, re-pack -- because ``backward()`` reads
the forward's workspace and the packed weights; ``train_step`` / ``train_step_features`` are that order.  ``data`` is any iterable of
``(x, y)`` as the reference's ``collate_fn`` yields them: a ``data.TrainLoader`` (section 27), or a list.  ``main`` is the command line:
``python -m multi_hmr_amd.train --pretrained NAME --train_data BEDLAM ...``."""
from __future__ import annotations

import os
import sys
import time

import torch

from . import _lib
from .evaluate import Evaluator, evaluate_dataset
from .optim import HeadsAdam, ModelAdam


class AverageMeter:
    """Running mean of a scalar (``val``: the last value, ``avg``: the mean so far)."""

    def __init__(self, name):
        self.name, self.val, self.sum, self.count, self.avg = name, 0.0, 0.0, 0, 0.0

    def update(self, val, n=1):
        self.val = float(val)
        self.sum += float(val) * n
        self.count += n
        self.avg = self.sum / max(self.count, 1)


class _NoWriter:
    """The default ``writer``: scalars go nowhere (pass a tensorboard ``SummaryWriter`` -- or anything with ``add_scalar`` and ``flush`` --
    to keep them)."""

    def add_scalar(self, *a, **k):
        pass

    def flush(self):
        pass


def _arg(args, name, default):
    v = getattr(args, name, None)
    return default if v is None else v


class Trainer:
    """``Trainer(model, loss, optimizer, args, gt_builder, evaluator=None, writer=None)``.

    ``model``: a ``Model`` on the GPU with ``train_heads_(True)`` and / or ``train_detection_(True)``; ``loss``: a ``Loss``; ``optimizer``: a
    ``HeadsAdam`` / ``ModelAdam`` (the step rewrites the packed weights) or any ``torch.optim`` optimiser over the same parameters (``repack_heads()`` then
    runs after every step); ``gt_builder``: a ``GroundTruth``; ``evaluator``: an ``Evaluator`` whose regressors the evaluation uses.
    ``args`` (a namespace) is read for ``save_dir`` ("logs"), ``name`` ("trainval"), ``max_epochs`` (1), ``log_freq`` (100), ``nb_max_ckpt``
    (10), ``det_thresh`` (0.3) and ``nms_kernel_size`` (3); ``log_dir``, ``ckpt_dir`` and ``visu_dir`` are written back into it as the reference
    does.  ``writer``: an object with ``add_scalar(tag, value, step)`` and ``flush()``; none by default (tensorboard is not a dependency)."""

    def __init__(self, model, loss, optimizer, args, gt_builder, evaluator=None, writer=None, best_val=1e5):
        self.model, self.loss, self.optimizer, self.args, self.gt_builder = model, loss, optimizer, args, gt_builder
        self.evaluator, self.best_val = evaluator, best_val
        self.current_epoch = self.current_iter = 0
        self.device = next(iter(model.parameters())).device
        args.log_dir = os.path.join(_arg(args, "save_dir", "logs"), _arg(args, "name", "trainval"))
        args.ckpt_dir, args.visu_dir = os.path.join(args.log_dir, "checkpoints"), os.path.join(args.log_dir, "visu")
        for d in (args.log_dir, args.ckpt_dir, args.visu_dir):
            os.makedirs(d, exist_ok=True)
        self.writer = writer if writer is not None else _NoWriter()

    # ------------------------------------------------------------------------------------------------ one step
    def prepare_gt(self, y):
        """Annotations of a batch -> the training targets (``GroundTruth.prepare``; None for a batch without humans)."""
        return self.gt_builder.prepare(y)

    def _step(self, forward, x, y):
        model, opt = self.model, self.optimizer
        if "idx" not in y:                                    # (already prepared targets are taken as they are)
            y = self.prepare_gt({k: (v.to(self.device) if isinstance(v, torch.Tensor) else v) for k, v in y.items()})
        gt = y
        if gt is None:
            return None
        heads = any(p.requires_grad for p in model.heads_parameters())
        detection = any(p.requires_grad for p in model.detection_parameters())
        # backbone parameters in the optimiser's groups (ModelAdam or any torch.optim optimiser; HeadsAdam covers the heads and the detector only)
        in_opt = {id(p) for g in getattr(opt, "param_groups", ()) for p in g["params"]}
        backbone = any(p.requires_grad and id(p) in in_opt for p in model.backbone_parameters(model._backbone_n) + model.embedding_parameters())
        if not (heads or detection or backbone):
            raise _lib.MhmrError("Trainer: nothing to train -- call model.train_heads_(True) and / or model.train_detection_(True) first")
        kw = {}
        if backbone:
            if forward is not model:
                raise ValueError("Trainer.train_step_features: stored features cannot follow a backbone that is being trained "
                                 "(backbone parameters that require grad are in the optimiser); use train_step")
            kw["train_backbone"] = True
        out = forward(x, idx=gt["idx"], K=gt["K"], is_training=True, return_readout=True, train_heads=heads, train_detection=detection, **kw)
        pred = model.decode_readout(out["readout"], out["offset"], gt["idx"], gt["K"])
        total, dict_loss = self.loss(dict(pred, scores=out["scores"]), gt, epoch=self.current_epoch, img_size=model.img_size)
        total.backward()                                      # before the optimiser step: it reads the packed weights the step rewrites
        opt.step()
        if not isinstance(opt, HeadsAdam):
            model.repack_heads()
        if backbone and not isinstance(opt, ModelAdam):           # (ModelAdam's step has rewritten the packed encoder as well)
            model.repack_backbone()
        opt.zero_grad(set_to_none=True)
        return dict_loss

    def train_step(self, x, y):
        """Forward from the images ``x [B, 3, S, S]``, decode, loss, backward, optimiser step (and re-pack) -> ``dict_loss`` (detached 0-d
        device tensors; None for a batch without humans, which is skipped)."""
        return self._step(self.model, x.to(self.device), y)

    def train_step_features(self, features, y):
        """``train_step`` from stored backbone features (``Model.forward_features``)."""
        return self._step(self.model.forward_features, features.to(self.device), y)

    @torch.no_grad()
    def cache_features(self, batches, dtype=torch.float32):
        """The backbone once per batch: ``[(features [B, N, C] of ``dtype``, y)]`` for ``train_step_features`` / ``train_n_iters``.  fp16 halves
        the store (the features are widened again and the results are those of the rounded features)."""
        if dtype not in (torch.float32, torch.float16):
            raise ValueError("cache_features: dtype is torch.float32 or torch.float16")
        return [(self.model.backbone_features(x.to(self.device)).clone().to(dtype), y) for x, y in batches]

    # ------------------------------------------------------------------------------------------------ the loop
    def train_n_iters(self, data):
        """One pass over ``data``: ``(x, y)`` with images ``x [B, 3, S, S]`` or stored features ``x [B, N, C]``."""
        print("\nTRAIN: ")
        self.model.train()
        meters = {k: AverageMeter(k) for k in ("workload/data", "workload/batch", "workload/ratio_data")}
        n_total = len(data) if hasattr(data, "__len__") else 0
        log_freq = max(int(_arg(self.args, "log_freq", 100)), 1)
        t_end = time.time()
        for i, (x, y) in enumerate(data):
            y = {k: (v.to(self.device) if isinstance(v, torch.Tensor) else v) for k, v in y.items()}
            t_data = time.time() - t_end
            dict_loss = self.train_step(x, y) if x.dim() == 4 else self.train_step_features(x, y)
            if dict_loss is None:
                t_end = time.time()
                continue
            keys = list(dict_loss)
            vals = torch.stack([dict_loss[k].detach().float() for k in keys]).tolist()      # the one host read of the step
            t_batch = time.time() - t_end
            meters["workload/data"].update(t_data)
            meters["workload/batch"].update(t_batch)
            meters["workload/ratio_data"].update(t_data / t_batch)
            for k, v in zip(keys, vals):
                meters.setdefault(f"loss/{k}", AverageMeter(f"loss/{k}")).update(v)
            if i % log_freq == 0:
                avg = lambda k: meters[k].avg if k in meters else float("nan")
                print(f"EPOCH={self.current_epoch:03d} - i={i:05d}/{n_total:05d} - workload/ratio_data={avg('workload/ratio_data'):.2f} - "
                      f"loss={avg('loss/total'):.2f} - bce={avg('loss/bce'):.2f} - v3d={avg('loss/v3d'):.2f} - transl={avg('loss/transl'):.2f}")
                for k, m in meters.items():
                    self.writer.add_scalar(k, m.avg, self.current_iter)
                self.writer.flush()
                sys.stdout.flush()
            self.current_iter += 1
            t_end = time.time()
        return 1

    def save_checkpoint(self):
        """``ckpt_dir/{epoch:05d}.pt`` = ``{epoch, iter, model_state_dict, args, optimizer_state_dict}``; the body-model layers
        (``smpl_layer_*``) are left out of the state dict as in the reference, and only the newest ``nb_max_ckpt`` files stay."""
        sd = {k: v for k, v in self.model.state_dict().items() if "smpl_layer_" not in k}
        path = os.path.join(self.args.ckpt_dir, f"{self.current_epoch:05d}.pt")
        torch.save({"epoch": self.current_epoch, "iter": self.current_iter, "model_state_dict": sd, "args": self.args,
                    "optimizer_state_dict": self.optimizer.state_dict()}, path)
        epochs = sorted(int(f[:-3]) for f in os.listdir(self.args.ckpt_dir) if f.endswith(".pt") and f[:-3].isdigit())
        keep = epochs[-max(int(_arg(self.args, "nb_max_ckpt", 10)), 1):]
        for e in epochs:
            if e not in keep:
                try:
                    os.remove(os.path.join(self.args.ckpt_dir, f"{e:05d}.pt"))
                except OSError:
                    print(f"could not remove checkpoint {e:05d}.pt")
        return path

    def resume(self, path):
        """Restore a checkpoint written by ``save_checkpoint``: the model's weights (the packed copies are dropped and rebuilt by the next
        forward), the optimiser state, the iteration count; training continues with the epoch AFTER the saved one."""
        ckpt = torch.load(path, map_location=self.device, weights_only=False)
        self.model.load_state_dict(ckpt["model_state_dict"], strict=False)
        if ckpt.get("optimizer_state_dict") is not None:
            self.optimizer.load_state_dict(ckpt["optimizer_state_dict"])
        self.current_epoch, self.current_iter = int(ckpt["epoch"]) + 1, int(ckpt["iter"])
        return ckpt

    def fit(self, data_train, l_data_val=()):
        """Epochs ``current_epoch .. args.max_epochs - 1``: train, checkpoint, evaluate every set of ``l_data_val``."""
        for _ in range(self.current_epoch, int(_arg(self.args, "max_epochs", 1))):
            t0 = time.time()
            self.train_n_iters(data_train)
            t_train = time.time() - t0
            self.save_checkpoint()
            t0 = time.time()
            for data_val in l_data_val:
                self.evaluate(data_val)
            t_eval = time.time() - t0
            self.writer.add_scalar("workload/train_n_iters", t_train, self.current_epoch)
            self.writer.add_scalar("workload/evaluate", t_eval, self.current_epoch)
            self.writer.add_scalar("workload/ratio_trainVal", t_eval / max(t_train + t_eval, 1e-12), self.current_epoch)
            self.current_epoch += 1
        return 1

    @torch.no_grad()
    def evaluate(self, data):
        """``evaluate_dataset`` over ``data`` with the args' ``det_thresh`` / ``nms_kernel_size``; the metrics go to the writer under the data
        set's ``name`` (``data.dataset.name`` or ``data.name``, "val" otherwise); returns the PVE in mm.  ``args.val_batch_size`` (1) above 1
        says that ``data`` holds batches of several images: they are evaluated whole, on the device (``batched=True``)."""
        print("\nEVAL: ")
        self.model.eval()
        ev = Evaluator(self.evaluator.smplx2smpl, self.evaluator.h36m_regressor) if self.evaluator is not None else Evaluator()
        summary = evaluate_dataset(self.model, data, self.gt_builder, det_thresh=_arg(self.args, "det_thresh", 0.3),
                                   nms_kernel_size=_arg(self.args, "nms_kernel_size", 3), evaluator=ev,
                                   batched=int(_arg(self.args, "val_batch_size", 1)) > 1)
        name = getattr(getattr(data, "dataset", data), "name", "val")
        print(f"***EVAL METRICS - {name}***")
        for k, v in summary.items():
            self.writer.add_scalar(f"{name}/{k}", v, self.current_iter)
            print(f"    - {k}: {v:.1f}")
        self.writer.flush()
        sys.stdout.flush()
        self.last_eval = summary
        return summary["pve"]


def build_parser():
    """The reference's ``train.py`` arguments where they apply to what this package trains, with its names and defaults; ``--n_iter``
    (``--n_iters_per_epoch``, ``-iter``) training batches make an epoch and ``--max_epochs`` epochs are run (``--max_iter``, if given, sets
    ``max_epochs = max_iter // n_iter`` as the reference does).  The loss weights are ``Loss.add_specific_args``."""
    from argparse import ArgumentParser
    from .loss import Loss
    p = ArgumentParser(description="Train the heads and the detector of a Multi-HMR checkpoint, on a frozen backbone or with its last blocks")
    p.add_argument("--train_data", type=str, default="BEDLAM", choices=["BEDLAM"])
    p.add_argument("--train_split", type=str, default="training")
    p.add_argument("--train_n", type=int, default=-1)
    p.add_argument("--train_subsample", type=int, default=1)
    p.add_argument("--val_data", type=str, nargs="*", default=["BEDLAM"], choices=["BEDLAM", "EHF", "THREEDPW"])
    p.add_argument("--val_split", type=str, nargs="*", default=["validation"])
    p.add_argument("--val_n", type=int, nargs="*", default=None)
    p.add_argument("--val_subsample", type=int, nargs="*", default=None)
    p.add_argument("--save_dir", type=str, default="logs")
    p.add_argument("--name", type=str, default="trainval")
    p.add_argument("--pretrained", type=str, required=True, help="checkpoint name under models/multiHMR (demo.load_model); its backbone stays frozen unless --train_backbone is given")
    p.add_argument("--train_backbone", type=int, default=0,
                   help="train the final norm and the last N encoder blocks as well (0: frozen backbone; N = the depth also trains the token embedding)")
    p.add_argument("--amp", type=int, default=1, choices=[0, 1],
                   help="with --train_backbone: 1 = bf16 operands, fp32 accumulation in the backbone backward's linears, 0 = exact fp32")
    p.add_argument("--amp_attention", type=int, default=0, choices=[0, 1],
                   help="with --train_backbone: 1 = bf16 operands in the backbone backward's attention tape and backward as well, 0 = exact fp32")
    p.add_argument("--batch_size", type=int, default=2)
    p.add_argument("--val_batch_size", type=int, default=1,
                   help="images per validation batch; 1 = image by image with the host matching, as the reference; above 1 the batch is matched "
                        "per image and measured on the device (its metrics are those of the forward at that batch size)")
    p.add_argument("--num_workers", "-j", type=int, default=8)
    p.add_argument("--img_size", type=int, default=None, help="default: the checkpoint's")
    p.add_argument("--n_iter", "--n_iters_per_epoch", "-iter", type=int, default=100)
    p.add_argument("--max_epochs", type=int, default=1)
    p.add_argument("--max_iter", type=int, default=None)
    p.add_argument("--log_freq", type=int, default=100)
    p.add_argument("--nb_max_ckpt", type=int, default=10)
    p.add_argument("--learning_rate", "-lr", type=float, default=5e-6)
    p.add_argument("--train_detection", type=int, default=1, choices=[0, 1])
    p.add_argument("--fused_adam", type=int, default=0, choices=[0, 1],
                   help="with --train_backbone N > 0: 1 = ModelAdam, one fused step over the whole model that rewrites the packed weights; "
                        "0 = torch.optim.Adam and a re-pack after every step")
    p.add_argument("--max_grad_norm", type=float, default=None, help="global gradient-norm clipping inside HeadsAdam / ModelAdam (default: none)")
    p.add_argument("--extension", type=str, default="png", choices=["png", "jpg"])
    p.add_argument("--res", type=int, default=None)
    p.add_argument("--flip", type=int, default=1, choices=[0, 1])
    p.add_argument("--det_thresh", type=float, default=0.2)
    p.add_argument("--nms_kernel_size", type=int, default=3)
    p.add_argument("--seed", type=int, default=None, help="seeds the draws of the training set (images and flips)")
    p.add_argument("--data_dir", type=str, default="data", help="annotation pickles, and BEDLAM/ EHF/ 3DPW/ below it")
    p.add_argument("--smplx_dir", type=str, default="models", help="smplx/SMPLX_NEUTRAL.npz, smpl/SMPL_MALE.pkl, smpl/SMPL_FEMALE.pkl")
    return Loss.add_specific_args(p)


def make_optimizer(model, args):
    """The optimiser of the command line.  ``--train_backbone 0``: ``HeadsAdam`` over the heads (and the detector).  ``--train_backbone N``:
    ``train_backbone_(N, precision="bf16" if --amp else "f32", attention="bf16" if --amp_attention else "f32")``, ``train_embeddings_()`` when N is the encoder's depth, and ``torch.optim.Adam``
    over heads, detector, backbone and embedding parameters (the ``Trainer`` re-packs after each step) -- or, with ``--fused_adam 1``,
    ``ModelAdam`` over the same list (its step rewrites the packed weights).  ``--max_grad_norm`` goes to ``HeadsAdam`` / ``ModelAdam``."""
    n, detection = int(getattr(args, "train_backbone", 0) or 0), bool(args.train_detection)
    clip = getattr(args, "max_grad_norm", None)
    if n <= 0:
        return HeadsAdam(model, lr=args.learning_rate, detection=detection, max_grad_norm=clip)
    model.train_backbone_(n, precision="bf16" if int(getattr(args, "amp", 1)) else "f32",
                          attention="bf16" if int(getattr(args, "amp_attention", 0)) else "f32")
    params = model.heads_parameters() + (model.detection_parameters() if detection else []) + model.backbone_parameters(n)
    if n == len(model.backbone.encoder.blocks):
        model.train_embeddings_()
        params += model.embedding_parameters()
    if int(getattr(args, "fused_adam", 0) or 0):
        return ModelAdam(model, lr=args.learning_rate, detection=detection, max_grad_norm=clip)
    return torch.optim.Adam(params, lr=args.learning_rate)


def main(argv=None):
    """``python -m multi_hmr_amd.train --pretrained NAME ...``: ``load_model`` -> ``train_heads_`` / ``train_detection_`` -> ``make_optimizer``
    -> ``Trainer.fit`` over a ``TrainLoader`` of the training set, with one loader per validation set."""
    from . import data
    from .bodymodel import BodyModel
    from .demo import load_model
    from .groundtruth import GroundTruth
    from .loss import Loss
    args = build_parser().parse_args(argv)
    if args.max_iter is not None:
        args.max_epochs = args.max_iter // max(args.n_iter, 1)
    device = torch.device("cuda")
    model = load_model(args.pretrained, device=device, **({} if args.img_size is None else {"img_size": args.img_size}))
    args.img_size = S = int(model.img_size)
    model = model.eval().train_heads_(True).train_detection_(bool(args.train_detection))
    optimizer = make_optimizer(model, args)
    body = lambda *parts: os.path.join(args.smplx_dir, *parts)
    smpl = {g: (BodyModel(body("smpl", f"SMPL_{g.upper()}.pkl"), "smpl", num_betas=10) if os.path.isfile(body("smpl", f"SMPL_{g.upper()}.pkl")) else None)
            for g in ("male", "female")}
    gt = GroundTruth(S, patch_size=14, nearness=getattr(model, "nearness", True), person_center=getattr(model, "person_center", "head"),
                     smplx_neutral=BodyModel(body("smplx", "SMPLX_NEUTRAL.npz"), "smplx", num_betas=11), smpl_male=smpl["male"],
                     smpl_female=smpl["female"])
    roots = {"BEDLAM": "BEDLAM", "EHF": "EHF", "THREEDPW": "3DPW"}
    make = lambda name, **kw: getattr(data, name)(img_size=S, root_dir=os.path.join(args.data_dir, roots[name]), annotations_dir=args.data_dir, **kw)
    train_set = make(args.train_data, split=args.train_split, training=True, n_iter=args.batch_size * args.n_iter, subsample=args.train_subsample,
                     n=args.train_n, extension=args.extension, res=args.res, flip=args.flip, seed=args.seed)
    print(train_set)
    train = data.TrainLoader(train_set, args.batch_size, device, workers=args.num_workers)
    vals = []
    for i, (name, split) in enumerate(zip(args.val_data, args.val_split)):
        kw = dict(split=split, training=False, subsample=args.val_subsample[i] if args.val_subsample else 1)
        if name == "BEDLAM":
            kw.update(n=args.val_n[i] if args.val_n else -1, extension=args.extension, res=args.res)
        # the reference evaluates image by image; above 1, Trainer.evaluate takes the whole batch on the device
        vals.append(data.TrainLoader(make(name, **kw), args.val_batch_size, device, workers=args.num_workers))
        print(vals[-1].dataset)
    trainer = Trainer(model, Loss(args), optimizer, args, gt)
    trainer.fit(train, vals)
    return trainer


__all__ = ["AverageMeter", "Trainer", "build_parser", "make_optimizer", "main"]


if __name__ == "__main__":
    main()
