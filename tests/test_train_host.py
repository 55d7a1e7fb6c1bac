"""-m "not gpu": the Trainer's host side (multi_hmr_amd/train.py) -- checkpoint contents, the clean-up of old
checkpoints, resume, the writer default -- on a stand-in model: nothing here runs a forward."""
import argparse
import ast
import os

import torch
from torch import nn

import multi_hmr_amd
from multi_hmr_amd import HeadsAdam, Trainer
from multi_hmr_amd import train as train_mod


class _Tiny(nn.Module):
    """Parameter names as a checkpoint of the reference has them, body-model layers included."""

    def __init__(self):
        super().__init__()
        self.mlp_classif = nn.Linear(3, 2)
        self.smpl_layer_neutral_10 = nn.Linear(2, 2)
        self.register_buffer("smpl_layer_faces", torch.arange(6.0))


class _Writer:
    def __init__(self):
        self.scalars, self.flushed = [], 0

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), int(step)))

    def flush(self):
        self.flushed += 1


def _trainer(tmp_path, nb_max_ckpt=2, writer=None):
    torch.manual_seed(0)
    model = _Tiny()
    opt = torch.optim.Adam(model.mlp_classif.parameters(), lr=1e-2)
    args = argparse.Namespace(save_dir=str(tmp_path), name="run", nb_max_ckpt=nb_max_ckpt, max_epochs=3, log_freq=1)
    return Trainer(model, loss=None, optimizer=opt, args=args, gt_builder=None, writer=writer), model, opt


def _one_update(model, opt):
    opt.zero_grad()
    model.mlp_classif(torch.ones(1, 3)).sum().backward()
    opt.step()


def test_exports_and_no_tensorboard_at_module_level():
    assert multi_hmr_amd.Trainer is Trainer and multi_hmr_amd.HeadsAdam is HeadsAdam
    assert {"Trainer", "HeadsAdam"} <= set(multi_hmr_amd.__all__)
    for mod in (train_mod, multi_hmr_amd.optim):
        tree = ast.parse(open(mod.__file__).read())
        for node in tree.body:
            names = ([a.name for a in node.names] if isinstance(node, ast.Import) else
                     [node.module or ""] if isinstance(node, ast.ImportFrom) else [])
            assert not any("tensorboard" in n for n in names), names
    doc = Trainer.__doc__ + train_mod.__doc__
    assert "FROZEN backbone" in doc and "no autocast" in doc          # the two stated differences from the reference


def test_directories_and_default_writer(tmp_path):
    tr, model, opt = _trainer(tmp_path)
    a = tr.args
    assert a.log_dir == os.path.join(str(tmp_path), "run") and a.ckpt_dir == os.path.join(a.log_dir, "checkpoints")
    assert os.path.isdir(a.ckpt_dir) and os.path.isdir(a.visu_dir)
    tr.writer.add_scalar("x", 1.0, 0)
    tr.writer.flush()
    assert (tr.current_epoch, tr.current_iter) == (0, 0)


def test_checkpoint_keys_smpl_layer_removal_and_cleanup(tmp_path):
    tr, model, opt = _trainer(tmp_path, nb_max_ckpt=2)
    for epoch in range(4):
        _one_update(model, opt)
        tr.current_epoch, tr.current_iter = epoch, 10 * (epoch + 1)
        path = tr.save_checkpoint()
        assert path == os.path.join(tr.args.ckpt_dir, f"{epoch:05d}.pt") and os.path.isfile(path)
    assert sorted(os.listdir(tr.args.ckpt_dir)) == ["00002.pt", "00003.pt"]            # the newest nb_max_ckpt
    ckpt = torch.load(path, weights_only=False)
    assert set(ckpt) == {"epoch", "iter", "model_state_dict", "args", "optimizer_state_dict"}
    assert ckpt["epoch"] == 3 and ckpt["iter"] == 40 and ckpt["args"].name == "run"
    assert set(ckpt["model_state_dict"]) == {"mlp_classif.weight", "mlp_classif.bias"}
    assert any("smpl_layer_" in k for k in model.state_dict())
    assert set(ckpt["optimizer_state_dict"]) == {"state", "param_groups"} and len(ckpt["optimizer_state_dict"]["state"]) == 2


def test_resume_restores_epoch_iteration_weights_and_optimiser_state(tmp_path):
    tr, model, opt = _trainer(tmp_path)
    _one_update(model, opt)
    _one_update(model, opt)
    tr.current_epoch, tr.current_iter = 4, 123
    path = tr.save_checkpoint()
    want_w = model.mlp_classif.weight.detach().clone()
    want = {k: v.clone() for k, v in opt.state[model.mlp_classif.weight].items()}
    _one_update(model, opt)                                                           # what a continued run does next
    after = model.mlp_classif.weight.detach().clone()

    tr2, model2, opt2 = _trainer(tmp_path / "other")
    with torch.no_grad():
        model2.smpl_layer_neutral_10.weight.fill_(7.0)
    tr2.resume(path)
    assert (tr2.current_epoch, tr2.current_iter) == (5, 123)                          # the epoch after the saved one
    assert torch.equal(model2.mlp_classif.weight, want_w)
    assert bool((model2.smpl_layer_neutral_10.weight == 7.0).all())                   # not in the checkpoint: untouched
    got = opt2.state[model2.mlp_classif.weight]
    assert float(got["step"]) == 2.0 and all(torch.equal(got[k], want[k]) for k in ("exp_avg", "exp_avg_sq"))
    _one_update(model2, opt2)
    assert torch.equal(model2.mlp_classif.weight, after)                              # and it continues with the same bits


def test_fit_runs_the_epoch_loop_with_checkpoints_and_writer(tmp_path):
    """fit() over an empty training set: three epochs, three checkpoints (two kept), the workload scalars per epoch."""
    w = _Writer()
    tr, model, opt = _trainer(tmp_path, writer=w)
    calls = []
    tr.evaluate = lambda data: calls.append(data)
    assert tr.fit([], ["val_a", "val_b"]) == 1
    assert tr.current_epoch == 3 and calls == ["val_a", "val_b"] * 3
    assert sorted(os.listdir(tr.args.ckpt_dir)) == ["00001.pt", "00002.pt"]
    tags = [t for t, _, _ in w.scalars]
    assert tags == ["workload/train_n_iters", "workload/evaluate", "workload/ratio_trainVal"] * 3
    assert [s for _, _, s in w.scalars] == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    tr.fit([], [])                                                                    # nothing left to do
    assert tr.current_epoch == 3


def test_average_meter():
    m = train_mod.AverageMeter("x")
    m.update(1.0)
    m.update(4.0, n=2)
    assert (m.val, m.count, m.avg) == (4.0, 3, 3.0)
