"""Host side of the training-data path (no GPU), multi_hmr_amd/data.py and the ABI of ``mhmr_preprocess_u8_batch_oriented``:

* the orientation index map against Pillow's rotate(-90, expand=True) and ImageOps.mirror, in the reference's order;
* ``sample`` + ``collate`` against the ``y`` the reference's own readers produced on the fixture set (tests/golden/data_pipeline.npz):
  shape, dtype and exact values -- the arithmetic is the reference's numpy, no tolerance;
* the new entry point: declared, exported, bound; the ctypes struct against the compiled header; the checks before any launch;
* ``TrainLoader``: sampler order under a slow decoder, ``len()``."""
import ctypes
import os
import random
import shutil
import subprocess
import threading

import numpy as np
import pytest
import torch

import data_oracle as do
from multi_hmr_amd import _lib, data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE = -1, -2
FIELDS = ["img", "H", "W", "ow", "oh", "y0", "rows", "pad_x", "pad_y", "ksh", "ksv", "kh", "bh", "kv", "bv", "tmp", "orient"]
S = 56


# -------------------------------------------------------------------------------------------------------- orientation
@pytest.mark.parametrize("H,W", [(4, 6), (5, 3), (1, 7)])
@pytest.mark.parametrize("orient", [0, 1, 2, 3])
def test_orientation_index_map_is_pillows_rotate_then_mirror(H, W, orient):
    arr = np.arange(H * W * 3, dtype=np.uint8).reshape(H, W, 3)
    want = np.asarray(do.pil_oriented(arr, orient))
    ys, xs = do.orient_index_map(H, W, orient)
    assert want.shape == ((W, H, 3) if orient & 2 else (H, W, 3))
    assert np.array_equal(arr[ys, xs], want)
    assert np.array_equal(do.host_oriented(arr, orient), want)       # the oracle of the GPU tests says the same


def test_the_mirror_is_applied_after_the_rotation_not_before():
    arr = np.arange(4 * 6 * 3, dtype=np.uint8).reshape(4, 6, 3)
    from PIL import Image, ImageOps
    other = np.asarray(ImageOps.mirror(Image.fromarray(arr)).rotate(-90, expand=True))
    ys, xs = do.orient_index_map(4, 6, 3)
    assert not np.array_equal(arr[ys, xs], other)


# -------------------------------------------------------------------------------------------------------- annotations
def _dataset(name, training=False, **kw):
    annots, _ = do.annotations(name)
    make = {"bedlam": data.BEDLAM, "3dpw": data.THREEDPW, "ehf": data.EHF}[name]
    if name == "bedlam":
        kw.setdefault("split", "training" if training else "validation")
    return make(training=training, img_size=S, root_dir="/nowhere", annots=annots, **kw)


def _assert_y(got, want):
    assert set(got) == set(want), set(got) ^ set(want)
    for k, w in want.items():
        g = got[k]
        if k == "imagename":
            assert isinstance(g, np.ndarray) and g.dtype.kind == "U" and g.tolist() == w.tolist()
            continue
        assert isinstance(g, torch.Tensor) and g.dtype == torch.float32 and w.dtype == np.float32, k
        assert tuple(g.shape) == w.shape, (k, tuple(g.shape), w.shape)
        assert np.array_equal(g.numpy(), w), k


@pytest.mark.parametrize("name,tag", [("bedlam", "bedlam/val_all"), ("3dpw", "3dpw/all"), ("ehf", "ehf/all")])
def test_evaluation_batches_equal_the_reference(name, tag):
    ds = _dataset(name)
    _, want = do.batch(tag)
    assert len(ds) == len(want["imagename"])
    samples = [ds.sample(i) for i in range(len(ds))]
    assert all(s.orient == (2 if "closeup" in s.imagename else 0) for s in samples)      # rotated, never mirrored
    _assert_y(data.collate(samples), want)


def test_a_batch_without_any_person_has_no_person_keys():
    ds = _dataset("bedlam")
    _, want = do.batch("bedlam/val_empty")
    y = data.collate([ds.sample(ds.imagenames.index("seq_d/empty_0004.png"))])
    _assert_y(y, want)
    assert tuple(y["valid_humans"].shape) == (1, 0) and set(y) == {"imagename", "K", "n_humans", "valid_humans"}


def _training_seeds():
    return [int(s) for s in do.golden()["bedlam/train_seeds"]]


@pytest.mark.parametrize("drawn", [False, True])
@pytest.mark.parametrize("which", [0, 1])
def test_training_batches_equal_the_reference(which, drawn):
    """Flips forced from the record, then drawn from the seeded generator; either way the picks are the recorded ones.  The batches
    hold a mirrored three-person image with two persons at equal depth, the closeup with and without the mirror, the image whose only
    person is behind the camera (dropped: an image without persons inside a batch that has some) and the image without persons."""
    seed = _training_seeds()[which]
    g = do.golden()
    picks, flips = g[f"bedlam/train_{seed}/picks"].tolist(), g[f"bedlam/train_{seed}/flips"].tolist()
    _, want = do.batch(f"bedlam/train_{seed}")
    ds = _dataset("bedlam", training=True, n_iter=len(picks), seed=seed)
    assert len(ds) == len(picks)
    samples = [ds.sample(i) if drawn else ds.sample(i, flip=flips[i]) for i in range(len(picks))]
    assert [s.index for s in samples] == picks
    assert [int(s.flip) for s in samples] == flips
    assert [s.orient for s in samples] == [f | (2 if "closeup" in ds.imagenames[p] else 0) for p, f in zip(picks, flips)]
    _assert_y(data.collate(samples), want)
    assert 0.0 in want["n_humans"] and want["n_humans"].max() == 3.0


def test_the_fixture_set_covers_what_it_should():
    g = do.golden()
    flips = sum((g[f"bedlam/train_{s}/flips"].tolist() for s in _training_seeds()), [])
    assert set(flips) == {0, 1}
    annots, pixels = do.annotations("bedlam")
    sizes = {n: p.shape[:2] for n, p in pixels.items()}
    assert any(h > w for h, w in sizes.values()) and any(w > h for h, w in sizes.values()) and any("closeup" in n for n in sizes)
    from multi_hmr_amd.preprocess import contain_size
    assert any((S - contain_size(w, h, S)[0]) % 2 == 1 for h, w in sizes.values())
    three = annots["seq_a/land_0000.png"]["humans"]
    z = [float(h["smplx_transl"][2]) for h in three]
    assert len(z) == 3 and z != sorted(z) and len(set(z)) == 2
    assert [float(h["smplx_transl"][2]) <= 0.01 for h in annots["seq_c/behind_0003.png"]["humans"]] == [True]


def test_the_depth_sort_is_stable_and_crops_other_than_0_raise():
    ds = _dataset("bedlam")
    s = ds.sample(ds.imagenames.index("seq_a/land_0000.png"))
    src = do.annotations("bedlam")[0]["seq_a/land_0000.png"]["humans"]
    order = [next(j for j, h in enumerate(src) if np.array_equal(h["smplx_shape"], p["smplx_shape"])) for p in s.humans]
    assert order == [1, 0, 2]                              # the nearest first; the two at 3.5 m keep their stored order
    ds = _dataset("bedlam", training=True, n_iter=4, seed=0, crops=[1])
    with pytest.raises(NameError):
        ds.sample(0)


def test_a_pickle_path_is_a_source_of_annotations(tmp_path):
    do.write_files("bedlam", str(tmp_path), ["validation"], [])
    ds = data.BEDLAM(split="validation", img_size=S, root_dir=str(tmp_path / "BEDLAM"), annotations_dir=str(tmp_path))
    assert len(ds) == 5 and ds.sample(0).path == os.path.join(str(tmp_path / "BEDLAM"), "validation", "seq_a/land_0000.png")
    jpg = data.BEDLAM(split="validation", img_size=S, annotations_dir=str(tmp_path), extension="jpg", res=512)
    assert jpg.imagenames[0] == "seq_a/land_0000_512.jpg"


def test_package_exports_and_the_command_line_takes_the_reference_argument_names():
    import multi_hmr_amd
    from multi_hmr_amd import collate, train
    assert {"AnnotatedImages", "BEDLAM", "THREEDPW", "EHF", "TrainLoader"} <= set(multi_hmr_amd.__all__)
    assert hasattr(collate, "allgather_persons_async")     # the multi-GPU module keeps its name; the batch's y is data.collate
    a = train.build_parser().parse_args(["--pretrained", "ckpt", "--train_data", "BEDLAM", "--val_data", "BEDLAM", "EHF", "--val_split",
                                         "validation", "test", "--batch_size", "32", "-lr", "1e-5", "--img_size", "896", "--max_epochs", "3",
                                         "--n_iter", "50", "--num_workers", "16", "--save_dir", "out", "--name", "run", "--log_freq", "10"])
    assert (a.train_split, a.val_data, a.val_split, a.batch_size, a.learning_rate, a.img_size, a.max_epochs, a.n_iter, a.num_workers,
            a.save_dir, a.name, a.pretrained, a.log_freq) == ("training", ["BEDLAM", "EHF"], ["validation", "test"], 32, 1e-5, 896, 3, 50, 16,
                                                             "out", "run", "ckpt", 10)
    assert a.alpha_bce == 10.0 and callable(train.main)    # the loss weights are Loss.add_specific_args


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_oriented_entry_point_is_declared_exported_and_bound():
    name = "mhmr_preprocess_u8_batch_oriented"
    assert name in _lib.EXPORTS and name in _lib._SIGS
    args, res = _lib._SIGS[name]
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert args == [ctypes.POINTER(_lib.PreImageO), vp, i, i, vp, vp, vp] and res is i
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    assert "int mhmr_preprocess_u8_batch_oriented(const mhmr_pre_image_o* host, const mhmr_pre_image_o* dev, int B, int S," in header
    assert "#define MHMR_VERSION 106 " in header and _lib.VERSION == 106        # additive
    assert [n for n, _ in _lib.PreImageO._fields_] == FIELDS
    assert [n for n, _ in _lib.PreImage._fields_] == FIELDS[:-1]                 # the existing descriptor is as it was
    assert (_lib.ORIENT_MIRROR, _lib.ORIENT_ROT90) == (1, 2) == (data.ORIENT_MIRROR, data.ORIENT_ROT90)
    assert "#define MHMR_ORIENT_MIRROR 1\n" in header and "#define MHMR_ORIENT_ROT90 2\n" in header


def test_oriented_descriptor_matches_compiled_sizeof_and_offsetof(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mhmr.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(mhmr_pre_image_o));\n' +
                   "".join(f'  printf(" %zu", offsetof(mhmr_pre_image_o, {n}));\n' for n in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.PreImageO)] + [getattr(_lib.PreImageO, n).offset for n in FIELDS]


def _descriptors(n, orient=0):
    """n descriptors that pass every check with made-up pointers (a stored 640 x 480 image at S = 224; rotated: 480 wide, 640 high):
    every call below must fail a check, a call that passed them all would launch on those pointers."""
    d = (_lib.PreImageO * n)()
    for x in d:
        x.img = x.kh = x.bh = x.kv = x.bv = x.tmp = 4096
        x.H, x.W, x.y0, x.ksh, x.ksv, x.orient = 480, 640, 0, 13, 13, orient
        if orient & 2:
            x.ow, x.oh, x.rows, x.pad_x, x.pad_y = 168, 224, 640, 28, 0
        else:
            x.ow, x.oh, x.rows, x.pad_x, x.pad_y = 224, 168, 480, 0, 28
    return d


def test_oriented_entry_point_rejects_bad_input_before_any_launch():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("libmhmr.so is not built")
    lib = _lib.lib()
    call = lambda d, B, S, dev=4096, lut=4096, out=4096: lib.mhmr_preprocess_u8_batch_oriented(d, dev, B, S, lut, out, None)
    d = _descriptors(2)
    for B in (0, -1, 65536):
        assert call(d, B, 224) == BAD_SHAPE
    assert call(d, 2, 0) == BAD_SHAPE
    assert call(None, 2, 224) == BAD_ARG
    assert call(d, 2, 224, dev=None) == BAD_ARG
    assert call(d, 2, 224, lut=None) == BAD_ARG
    assert call(d, 2, 224, out=None) == BAD_ARG
    for orient in (4, 8, 7, -1, 1 << 30):
        d = _descriptors(2)
        d[1].orient = orient
        assert call(d, 2, 224) == BAD_ARG, orient
    for field in ("img", "kh", "bh", "kv", "bv", "tmp"):
        for orient in (0, 3):
            d = _descriptors(2, orient)
            setattr(d[1], field, None)
            assert call(d, 2, 224) == BAD_ARG, field
    for orient, field, value in ((0, "rows", 481), (2, "rows", 641), (3, "y0", 1), (0, "pad_x", 1), (2, "pad_y", 1), (1, "ow", 225), (2, "H", 0)):
        d = _descriptors(2, orient)
        setattr(d[1], field, value)
        assert call(d, 2, 224) == BAD_SHAPE, (orient, field)


# ------------------------------------------------------------------------------------------------------------- loader
class _FakePre:
    def __init__(self):
        self.calls = []

    def batch_oriented(self, images, orient, out=None):
        self.calls.append(([int(i[0, 0, 0]) for i in images], list(orient)))
        return torch.tensor([float(i[0, 0, 0]) for i in images])


class _Indexed:
    """A dataset whose sample i names image i; no persons."""
    img_size = S

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def sample(self, i):
        return data.Sample(f"{i}.png", str(i), i % 4, np.eye(3), [], i)


@pytest.mark.parametrize("n,drop_last,want", [(10, False, [4, 4, 2]), (10, True, [4, 4]), (8, False, [4, 4]), (3, True, []), (3, False, [3])])
def test_loader_yields_batches_in_sampler_order_whatever_the_thread_timing(n, drop_last, want):
    """The decoder finishes the images of a batch in reverse: image i waits until image i + 1 of its batch is done (events, no clocks)."""
    last = sum(want) - 1
    done = {i: threading.Event() for i in range(n + 1)}
    starts = np.cumsum([0] + want).tolist()

    def decode(path):
        i = int(path)
        if i != last and (i + 1) not in starts:
            assert done[i + 1].wait(timeout=30)
        done[i].set()
        return torch.full((2, 2, 3), i, dtype=torch.uint8), (2, 2)

    pre = _FakePre()
    loader = data.TrainLoader(_Indexed(n), 4, "cpu", workers=4, drop_last=drop_last, decode=decode, preprocessor=pre)
    assert len(loader) == len(want)
    got = list(loader)
    assert [x.tolist() for x, _ in got] == [[float(i) for i in range(a, a + b)] for a, b in zip(starts, want)]
    assert [y["imagename"].tolist() for _, y in got] == [[f"{i}.png" for i in range(a, a + b)] for a, b in zip(starts, want)]
    assert [c[1] for c in pre.calls] == [[i % 4 for i in range(a, a + b)] for a, b in zip(starts, want)]
    assert all(tuple(y["valid_humans"].shape) == (b, 0) for (_, y), b in zip(got, want))
    assert not [t for t in threading.enumerate() if t.name.startswith("mhmr-")]


def test_loader_shuffle_is_a_seeded_permutation_and_the_pool_ignores_the_cpu_count():
    decode = lambda path: (torch.full((2, 2, 3), int(path), dtype=torch.uint8), (2, 2))
    order = lambda seed: [int(v) for x, _ in data.TrainLoader(_Indexed(9), 4, "cpu", shuffle=True, seed=seed, decode=decode,
                                                               preprocessor=_FakePre()) for v in x.tolist()]
    a, b = order(5), order(5)
    assert a == b and sorted(a) == list(range(9)) and a != list(range(9))
    want = list(range(9))
    random.Random(5).shuffle(want)
    assert a == want
    assert data.TrainLoader(_Indexed(9), 4, "cpu", workers=64).workers == 16
    import inspect
    src = inspect.getsource(data)
    for word in ("cpu_count", "nproc", "sched_getaffinity", "multiprocessing"):
        assert word not in src
