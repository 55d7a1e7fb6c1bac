"""Host side of the batched input path (no GPU): the C ABI of ``mhmr_preprocess_u8_batch`` (signature, descriptor layout, the
checks it makes before any launch) and ``pipeline.run_batched`` -- ordering, batching, look-ahead, memory bound and error policy --
driven with fake decode / preprocess / forward callables; the full-resolution intrinsics and the worker count of ``predict_images``."""
import ctypes
import glob
import inspect
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest
import torch

from multi_hmr_amd import _lib, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, BAD_SHAPE = -1, -2
FIELDS = ["img", "H", "W", "ow", "oh", "y0", "rows", "pad_x", "pad_y", "ksh", "ksv", "kh", "bh", "kv", "bv", "tmp"]


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_batch_entry_point_is_declared_with_the_documented_signature():
    assert "mhmr_preprocess_u8_batch" in _lib.EXPORTS
    args, res = _lib._SIGS["mhmr_preprocess_u8_batch"]
    vp, i = ctypes.c_void_p, ctypes.c_int
    # (host descriptors, device descriptors, B, S, lut, out, stream) -> int
    assert args == [ctypes.POINTER(_lib.PreImage), vp, i, i, vp, vp, vp] and res is i
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    assert "int mhmr_preprocess_u8_batch(const mhmr_pre_image* host, const mhmr_pre_image* dev, int B, int S, const float* lut," in header
    assert "#define MHMR_VERSION 106 " in header and _lib.VERSION == 106
    assert "preprocess.hip" in _lib.SOURCES                # the entry point lives in the existing translation unit


def test_descriptor_struct_has_the_field_order_of_the_header():
    assert [n for n, _ in _lib.PreImage._fields_] == FIELDS
    header = open(os.path.join(ROOT, "include", "mhmr.h")).read()
    body = header[header.index("typedef struct {\n    const void* img;"):header.index("} mhmr_pre_image;")]
    pos = [body.index(tok) for tok in ("img;", "H,", "W,", "ow,", "oh,", "y0,", "rows,", "pad_x,", "pad_y,", "ksh,", "ksv;",
                                       "*kh,", "*bh,", "*kv,", "*bv;", "tmp;")]
    assert pos == sorted(pos)
    assert ctypes.sizeof(_lib.PreImage) == 8 + 10 * 4 + 5 * 8


def test_descriptor_struct_matches_compiled_sizeof_and_offsetof(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if not os.path.isfile(_lib.LIB_PATH) or cc is None:
        pytest.skip("the compiled layout is compared only where libmhmr.so is built and a C compiler is present")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mhmr.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(mhmr_pre_image));\n' +
                   "".join(f'  printf(" %zu", offsetof(mhmr_pre_image, {n}));\n' for n in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.PreImage)] + [getattr(_lib.PreImage, n).offset for n in FIELDS]


def _descriptors(n, S=224):
    """n descriptors that pass every check (a 640x480 image at S = 224) with made-up pointers: every call below must fail a check,
    a call that passed them all would launch on those pointers."""
    d = (_lib.PreImage * n)()
    for x in d:
        x.img = x.kh = x.bh = x.kv = x.bv = x.tmp = 4096
        x.H, x.W, x.ow, x.oh, x.y0, x.rows, x.pad_x, x.pad_y, x.ksh, x.ksv = 480, 640, S, 168, 0, 480, 0, 28, 13, 13
    return d


def test_batch_entry_point_rejects_bad_input_before_any_launch():
    """Every call here returns before it touches the device, so it runs without a GPU (the pattern of
    test_host.py::test_person_head_entry_points_reject_bad_shapes_before_any_launch)."""
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("libmhmr.so is not built")
    lib = _lib.lib()
    call = lambda d, B, S, dev=4096, lut=4096, out=4096: lib.mhmr_preprocess_u8_batch(d, dev, B, S, lut, out, None)
    d = _descriptors(2)
    assert call(d, 0, 224) == BAD_SHAPE
    assert call(d, -1, 224) == BAD_SHAPE
    assert call(d, 65536, 224) == BAD_SHAPE                # the image index is a grid dimension
    assert call(d, 2, 0) == BAD_SHAPE
    assert call(None, 2, 224) == BAD_ARG                   # null host descriptors
    assert call(d, 2, 224, dev=None) == BAD_ARG            # null device descriptors
    assert call(d, 2, 224, lut=None) == BAD_ARG
    assert call(d, 2, 224, out=None) == BAD_ARG
    d = _descriptors(2)
    d[1].pad_x = 1                                         # pad_x + ow > S, in the SECOND descriptor (so the stride is right too)
    assert call(d, 2, 224) == BAD_SHAPE
    for field, value in (("pad_y", 57), ("rows", 481), ("y0", -1), ("ow", 225), ("ksv", 0), ("H", 0)):
        d = _descriptors(2)
        setattr(d[1], field, value)
        assert call(d, 2, 224) == BAD_SHAPE, field
    for field in ("img", "kh", "bh", "kv", "bv", "tmp"):
        d = _descriptors(2)
        setattr(d[1], field, None)
        assert call(d, 2, 224) == BAD_ARG, field


# ---------------------------------------------------------------------------------------------------- scheduling core
class Fakes:
    """decode / preprocess / forward that record what they were given; a source that is an Exception instance fails to decode."""

    def __init__(self):
        self.lock = threading.Lock()
        self.decoded = self.forwarded = self.max_ahead = 0
        self.batches = []

    def decode(self, s):
        if isinstance(s, Exception):
            raise s
        with self.lock:
            self.decoded += 1
        return ("item", s)

    def preprocess(self, items):
        return ("staged", tuple(items))

    def forward(self, staged, items):
        assert staged == ("staged", tuple(items))
        with self.lock:
            self.max_ahead = max(self.max_ahead, self.decoded - self.forwarded - len(items))
            self.forwarded += len(items)
        self.batches.append(len(items))
        return [("out", s) for _, s in items]


def _pipeline_threads():
    return [t for t in threading.enumerate() if t.name.startswith("mhmr-")]


@pytest.mark.parametrize("n", [0, 1, 4, 5, 11])            # 0, 1, batch_size, batch_size + 1, 2 batch_size + 3
def test_results_come_in_input_order_and_the_last_batch_has_the_remainder(n):
    f = Fakes()
    got = list(pipeline.run_batched(list(range(100, 100 + n)), f.decode, f.preprocess, f.forward, batch_size=4, workers=3))
    assert got == [(i, 100 + i, ("item", 100 + i), ("out", 100 + i), None) for i in range(n)]
    assert f.batches == [4] * (n // 4) + ([n % 4] if n % 4 else [])
    assert not _pipeline_threads()


def test_an_iterator_of_unknown_length_is_a_source():
    def frames():
        for i in range(7):
            yield f"frame{i}"
    f = Fakes()
    got = list(pipeline.run_batched(frames(), f.decode, f.preprocess, f.forward, batch_size=3))
    assert [g[1] for g in got] == [f"frame{i}" for i in range(7)] and [g[0] for g in got] == list(range(7))
    assert f.batches == [3, 3, 1]


def test_the_next_batch_is_decoded_while_a_forward_is_in_flight():
    """Events, no clocks: the decode of batch 1 waits until the forward of batch 0 has begun, and that forward does not return until
    a decode of batch 1 has said so.  A pipeline that decoded batch 1 only after the forward of batch 0 would stop here (and fail
    at the timeouts)."""
    in_forward, next_decoding = threading.Event(), threading.Event()
    seen = []

    def decode(s):
        if 4 <= s < 8 and in_forward.wait(timeout=30):
            next_decoding.set()
        return s

    def forward(staged, items):
        if items[0] == 0:
            in_forward.set()
            seen.append(next_decoding.wait(timeout=30))
        return items

    got = list(pipeline.run_batched(range(12), decode, lambda items: None, forward, batch_size=4, workers=2))
    assert [g[3] for g in got] == list(range(12))
    assert seen == [True]


def test_never_more_than_two_decoded_batches_wait_for_the_forward():
    """A forward that lets the decoders run as far as they may: the sources decoded beyond the batch in the forward never exceed two
    batches, however long the input."""
    f = Fakes()
    idle = threading.Event()
    inner = f.forward

    def slow_forward(staged, items):
        idle.wait(timeout=0.05)                            # never set: gives the producer time; the bound does not depend on it
        return inner(staged, items)

    got = list(pipeline.run_batched(range(64), f.decode, f.preprocess, slow_forward, batch_size=4, workers=4))
    assert len(got) == 64 and f.batches == [4] * 16
    assert f.max_ahead <= 2 * 4
    assert pipeline.LOOKAHEAD == 2


def test_on_error_raise_names_the_source_and_leaves_no_thread():
    f = Fakes()
    broken = type("Broken", (Exception,), {"filename": "folder/f.jpg"})("truncated file")
    sources = ["a.jpg", "b.jpg", "c.jpg", "d.jpg", "e.jpg", broken, "g.jpg"]
    gen = pipeline.run_batched(sources, f.decode, f.preprocess, f.forward, batch_size=4)
    got = [next(gen) for _ in range(4)]                    # the batch before the bad one is delivered
    assert [g[1] for g in got] == sources[:4]
    with pytest.raises(pipeline.PipelineError, match="folder/f.jpg") as info:
        next(gen)
    assert info.value.__cause__ is sources[5]
    assert f.batches == [4]                                # no forward was spent on the batch that holds it
    assert not _pipeline_threads()
    with pytest.raises(pipeline.PipelineError, match="missing.png"):
        list(pipeline.run_batched(["missing.png"], lambda s: open(s, "rb"), f.preprocess, f.forward))
    assert not _pipeline_threads()


def test_on_error_skip_yields_the_error_and_goes_on():
    f = Fakes()
    bad1, bad2 = ValueError("one"), ValueError("two")
    sources = [0, bad1, 2, 3, bad2, 5]
    got = list(pipeline.run_batched(sources, f.decode, f.preprocess, f.forward, batch_size=4, on_error="skip"))
    assert [g[0] for g in got] == list(range(6))
    assert [g[4] for g in got] == [None, bad1, None, None, bad2, None]
    assert [g[3] for g in got] == [("out", 0), None, ("out", 2), ("out", 3), None, ("out", 5)]
    assert f.batches == [3, 1]                             # the failed sources take no part in their batch
    got = list(pipeline.run_batched([bad1, bad2], f.decode, f.preprocess, f.forward, batch_size=4, on_error="skip"))
    assert [g[4] for g in got] == [bad1, bad2] and f.batches == [3, 1]        # a batch of failures alone: no forward
    with pytest.raises(ValueError):
        list(pipeline.run_batched([], f.decode, f.preprocess, f.forward, on_error="ignore"))


def test_closing_the_generator_early_and_a_failing_forward_leave_no_thread():
    f = Fakes()
    gen = pipeline.run_batched(range(1000), f.decode, f.preprocess, f.forward, batch_size=4)
    assert next(gen)[0] == 0
    gen.close()
    assert not _pipeline_threads() and f.decoded <= 3 * 4

    def forward(staged, items):
        raise RuntimeError("device lost")
    with pytest.raises(RuntimeError, match="device lost"):
        list(pipeline.run_batched(range(20), f.decode, f.preprocess, forward, batch_size=4))
    assert not _pipeline_threads()

    def preprocess(items):
        raise RuntimeError("no staging memory")
    with pytest.raises(RuntimeError, match="no staging memory"):
        list(pipeline.run_batched(range(20), f.decode, preprocess, f.forward, batch_size=4))
    assert not _pipeline_threads()


# -------------------------------------------------------------------------------------------- predict_images, host parts
@pytest.mark.parametrize("S", [672, 896])
def test_full_resolution_intrinsics_follow_the_reference_formula(S):
    """The reference's demo, before it draws: ratio = max(size) / S; K[0,0,2] = width / 2; K[0,1,2] = height / 2;
    K[0,0,0] and K[0,1,1] times ratio -- on K = get_camera_parameters(S, fov) (focal = S / (2 tan(fov / 2)), principal point S // 2)."""
    from PIL import Image
    from multi_hmr_amd.preprocess import get_camera_parameters
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "example_data", "*.jpg")))
    assert len(paths) == 7
    Kb = get_camera_parameters(S, fov=60, device="cpu", batch=7)
    for i, p in enumerate(paths):
        size = Image.open(p).size
        K = Kb[i:i + 1]
        want = torch.eye(3)[None]
        focal = S / (2 * np.tan(np.radians(60) / 2))
        want[0, 0, 0] = want[0, 1, 1] = focal
        want[0, 0, 2] = want[0, 1, 2] = S // 2
        ratio = max(size) / S
        want[0, 0, 2] = size[0] / 2.0
        want[0, 1, 2] = size[1] / 2.0
        want[0, [0, 1], [0, 1]] = ratio * want[0, [0, 1], [0, 1]]
        got = pipeline.full_resolution_K(K, size, S)
        assert torch.equal(got, want), (p, got, want)
        assert float(K[0, 0, 2]) == S // 2                 # the input K is left as it was
        assert abs(float(got[0, 0, 0]) - max(size) / (2 * np.tan(np.radians(30)))) < 1e-3


def test_workers_default_to_8_are_capped_at_16_and_ignore_the_cpu_count():
    assert inspect.signature(pipeline.predict_images).parameters["workers"].default == 8
    assert inspect.signature(pipeline.run_batched).parameters["workers"].default == 8
    assert pipeline.clamp_workers(64) == 16 and pipeline.clamp_workers(8) == 8 and pipeline.clamp_workers(0) == 1
    started = set()

    def decode(s):
        started.add(threading.current_thread().name)
        return s
    list(pipeline.run_batched(range(400), decode, lambda items: None, lambda staged, items: items, batch_size=100, workers=64))
    assert 1 <= len(started) <= 16
    src = inspect.getsource(pipeline)
    for word in ("cpu_count", "nproc", "sched_getaffinity", "multiprocessing"):
        assert word not in src


def test_decode_image_takes_paths_pil_images_and_arrays(tmp_path):
    from PIL import Image
    arr = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)
    Image.fromarray(arr).save(tmp_path / "a.png")
    for source in (str(tmp_path / "a.png"), tmp_path / "a.png", Image.fromarray(arr), arr, torch.from_numpy(arr)):
        img, size = pipeline.decode_image(source)
        assert size == (7, 5) and img.dtype == torch.uint8 and np.array_equal(img.numpy(), arr)
    grey = Image.fromarray(arr[..., 0])                    # converted to RGB as the reference's open_image does
    assert pipeline.decode_image(grey)[0].shape == (5, 7, 3)
    with pytest.raises(ValueError):
        pipeline.decode_image(arr.astype(np.float32))
    with pytest.raises(ValueError):
        pipeline.decode_image(np.zeros((500, 3, 3), np.uint8))        # taller than 100x its width: the guard of Preprocessor
