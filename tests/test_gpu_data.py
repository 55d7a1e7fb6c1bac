"""-m gpu: the training-data path on the GPU (multi_hmr_amd/data.py).

* ``Preprocessor.batch_oriented`` (mhmr_preprocess_u8_batch_oriented) is bit-exact against Pillow running the reference's operations
  (tests/data_oracle.py: rotate(-90, expand=True), ImageOps.mirror, contain, pad, normalize_rgb) for every orient code, equals
  ``Preprocessor.batch`` on a host-oriented copy, and writes nothing outside its output and its tmp slices;
* PNG files made from the golden's pixels go through ``TrainLoader`` into exactly the ``x`` and ``y`` the reference's readers produced;
* ``Trainer.train_n_iters`` over a loader gives the losses of ``train_step`` called by hand on the same batches."""
import os

import numpy as np
import pytest
import torch

import data_oracle as do
from multi_hmr_amd import data
from multi_hmr_amd import preprocess as pp

pytestmark = pytest.mark.gpu

# (W, H): both aspects with S - ow odd at S = 56, a square, two down-scales (one 33x), a source narrower than the filter support
SOURCES = [(53, 37), (37, 53), (64, 64), (500, 300), (1000, 30), (3, 200)]
DEV = "cuda:0"


def _cases():
    """Every source under every orient code: 24 images, as (uint8 [H, W, 3] array, orient)."""
    return [(do.make_image(H, W, seed=o), o) for W, H in SOURCES for o in range(4)]


@pytest.mark.parametrize("S", [56, 224])
def test_batch_oriented_is_bit_exact_against_pillow_for_host_device_and_mixed_inputs(S):
    cases = _cases()
    want = np.stack([do.pil_x(a, o, S) for a, o in cases])
    pre = pp.Preprocessor(S, DEV)
    orient = [o for _, o in cases]
    host = [torch.from_numpy(a) for a, _ in cases]
    for name, imgs in (("host", host), ("device", [t.cuda() for t in host]), ("mixed", [t.cuda() if j % 3 == 1 else t for j, t in enumerate(host)])):
        x = pre.batch_oriented(imgs, orient)
        assert x.shape == (len(cases), 3, S, S) and x.dtype == torch.float32 and x.is_cuda
        got = x.cpu().numpy()
        for j, (a, o) in enumerate(cases):
            assert np.array_equal(got[j], want[j]), (name, S, a.shape, o)


@pytest.mark.parametrize("S", [56, 224])
def test_every_code_equals_batch_on_a_host_oriented_copy_and_code_0_equals_batch(S):
    cases = _cases()
    pre = pp.Preprocessor(S, DEV)
    x = pre.batch_oriented([torch.from_numpy(a) for a, _ in cases], [o for _, o in cases])
    copies = pre.batch([torch.from_numpy(do.host_oriented(a, o)) for a, o in cases])
    assert torch.equal(x, copies)
    plain = [torch.from_numpy(a) for a, o in cases if o == 0]
    assert torch.equal(pre.batch_oriented(plain, [0] * len(plain)), pre.batch(plain))
    with pytest.raises(ValueError):
        pre.batch_oriented(plain, [4] * len(plain))
    with pytest.raises(ValueError):
        pre.batch_oriented(plain, [0])
    # the plan of a rotated image is that of its oriented size: 24 images, (W, H) and (H, W) of six sources, 64 x 64 once
    assert set(pre._tables) == {(H, W) for W, H in SOURCES} | {(W, H) for W, H in SOURCES}


def test_the_output_and_every_tmp_slice_sit_between_sentinels():
    S = 56
    cases = _cases()
    imgs, orient = [torch.from_numpy(a) for a, _ in cases], [o for _, o in cases]
    pre = pp.Preprocessor(S, DEV)
    want = pre.batch_oriented(imgs, orient).clone()      # sizes the workspace
    guard = float(np.float32(-12345.678))
    big = torch.full((len(cases) + 4, 3, S, S), guard, device=DEV)
    pre._tmp.fill_(0xA5)
    ret = pre.batch_oriented(imgs, orient, out=big[2:-2])
    assert ret.data_ptr() == big[2].data_ptr() and torch.equal(big[2:-2], want)
    assert bool((big[:2] == guard).all()) and bool((big[-2:] == guard).all())
    # the layout of the workspace: slice b = rows x ow x 3 bytes of the ORIENTED image's plan at the next multiple of 256
    tmp, off = pre._tmp.cpu().numpy(), 0
    for (a, o), img in zip(cases, imgs):
        H, W = (a.shape[1], a.shape[0]) if o & 2 else (a.shape[0], a.shape[1])
        t = pre._plan(H, W)
        used = t["rows"] * t["ow"] * 3
        end = off + -(-used // 256) * 256
        assert (tmp[off + used:end] == 0xA5).all(), (a.shape, o)
        off = end
    assert off <= tmp.size and (tmp[off:] == 0xA5).all()


def test_batch_and_batch_oriented_in_turn_share_the_staging_buffers():
    """The two methods stage through the same pinned buffers, device copy and tmp workspace, with descriptors of different sizes -- so the
    image offsets differ from call to call.  Four calls back to back on one Preprocessor, no synchronisation in between: each result is
    bit-equal to the same call on a Preprocessor of its own."""
    S = 56
    host = [torch.from_numpy(do.make_image(H, W, seed=7 + j)) for j, (W, H) in enumerate([(37, 53), (64, 48), (50, 50)])]
    a, b, c = host
    calls = [(None, [a, b.cuda(), c]),                       # batch, B = 3, mixed
             ([2, 1], [a.cuda(), b]),                        # batch_oriented, B = 2, mixed
             (None, [c]),                                    # batch, B = 1: the pinned buffer of the first call again
             ([3, 0, 2], [a, b, c.cuda()])]                  # batch_oriented, B = 3, mixed

    def run(pre, orient, imgs):
        return pre.batch(imgs) if orient is None else pre.batch_oriented(imgs, orient)
    shared = pp.Preprocessor(S, DEV)
    got = [run(shared, orient, imgs) for orient, imgs in calls]
    for j, (orient, imgs) in enumerate(calls):
        want = run(pp.Preprocessor(S, DEV), orient, imgs)
        assert got[j].shape == (len(imgs), 3, S, S) and torch.equal(got[j], want), (j, orient)


# ------------------------------------------------------------------------------------------------------- end to end
def _assert_y(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        if k == "imagename":
            assert got[k].tolist() == w.tolist()
            continue
        assert got[k].is_cuda and got[k].dtype == torch.float32 and tuple(got[k].shape) == w.shape, k
        assert np.array_equal(got[k].cpu().numpy(), w), k


def _files(name, tmp_path):
    layout = {"bedlam": (["training", "validation"], ["BEDLAM/training", "BEDLAM/validation"]), "3dpw": (["test"], ["3DPW/imageFiles"]),
              "ehf": (["test"], ["EHF"])}[name]
    return do.write_files(name, str(tmp_path), *layout)


@pytest.mark.parametrize("name,tag", [("bedlam", "bedlam/val_all"), ("3dpw", "3dpw/all"), ("ehf", "ehf/all")])
def test_files_through_the_loader_equal_the_reference_batch(name, tag, tmp_path):
    root = _files(name, tmp_path)
    make = {"bedlam": lambda: data.BEDLAM(split="validation", img_size=56, root_dir=os.path.join(root, "BEDLAM"), annotations_dir=root),
            "3dpw": lambda: data.THREEDPW(img_size=56, root_dir=os.path.join(root, "3DPW"), annotations_dir=root),
            "ehf": lambda: data.EHF(img_size=56, root_dir=os.path.join(root, "EHF"), annotations_dir=root)}[name]
    want_x, want_y = do.batch(tag)
    loader = data.TrainLoader(make(), len(want_x), DEV, workers=4)
    (x, y), = list(loader)
    assert x.is_cuda and x.dtype == torch.float32 and np.array_equal(x.cpu().numpy(), want_x)
    _assert_y(y, want_y)


@pytest.mark.parametrize("which", [0, 1])
def test_seeded_training_batches_through_the_loader_equal_the_reference(which, tmp_path, smplx_data):
    """The reference under random.seed(seed): the same picks, flips, pixels and annotations; GroundTruth.prepare takes the y."""
    from multi_hmr_amd import BodyModel, GroundTruth
    root = _files("bedlam", tmp_path)
    seed = int(do.golden()["bedlam/train_seeds"][which])
    want_x, want_y = do.batch(f"bedlam/train_{seed}")
    ds = data.BEDLAM(split="training", training=True, img_size=56, root_dir=os.path.join(root, "BEDLAM"), annotations_dir=root,
                     n_iter=len(want_x), seed=seed)
    loader = data.TrainLoader(ds, len(want_x), DEV, workers=4)
    assert len(loader) == 1
    (x, y), = list(loader)
    assert np.array_equal(x.cpu().numpy(), want_x)
    _assert_y(y, want_y)
    gt = GroundTruth(56, patch_size=14, smplx_neutral=BodyModel(smplx_data, "smplx", num_betas=11)).prepare(y)
    assert gt is not None and "idx" in gt and "K" in gt and bool(torch.isfinite(gt["v3d"]).all())


def test_train_n_iters_over_a_loader_gives_the_losses_of_train_step_by_hand(tmp_path):
    """Two batches with persons and one without (skipped) on the ViT-S 224 fixture of tests/test_gpu_train.py."""
    import gt_oracle as go
    from PIL import Image
    from test_gpu_train import S, _trainer
    counts = [2, 1, 1, 2, 0, 0]
    y0 = go.make_y("smplx", 51, S, counts, depth=2.6)
    g = np.random.default_rng(3)
    annots = {}
    os.makedirs(tmp_path / "img" / "validation")
    for i, c in enumerate(counts):
        name = f"im_{i:02d}.png"
        Image.fromarray(g.integers(0, 256, (S, S, 3), dtype=np.uint8)).save(tmp_path / "img" / "validation" / name)
        K = y0["K"][i].numpy()
        humans = [dict({k: v[i, j].numpy().copy() for k, v in y0.items() if k.startswith("smplx_")}, smplx_gender="neutral") for j in range(c)]
        annots[name] = {"focal": np.asarray([K[0, 0], K[1, 1]], np.float32), "princpt": np.asarray([K[0, 2], K[1, 2]], np.float32),
                        "size": np.asarray([S, S], np.int32), "humans": humans}
    ds = data.BEDLAM(split="validation", img_size=S, root_dir=str(tmp_path / "img"), annots=annots)
    batches = [(x.clone(), y) for x, y in data.TrainLoader(ds, 2, DEV, workers=4)]
    assert [int(y["n_humans"].sum()) for _, y in batches] == [3, 3, 0]

    by_hand = _trainer(tmp_path / "a")
    want = [by_hand.train_step(x, y) for x, y in batches]
    assert want[2] is None and all(float(w["total"]) == float(w["total"]) for w in want[:2])

    tr = _trainer(tmp_path / "b")
    got, step = [], tr.train_step
    tr.train_step = lambda x, y: got.append(step(x, y)) or got[-1]
    assert tr.train_n_iters(data.TrainLoader(ds, 2, DEV, workers=4)) == 1
    assert len(got) == 3 and got[2] is None and tr.current_iter == 2          # the batch without humans is skipped
    for a, b in zip(got[:2], want[:2]):
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a), (a, b)
