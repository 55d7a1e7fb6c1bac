"""The batched input path on the GPU: ``Preprocessor.batch`` (mhmr_preprocess_u8_batch, two launches for a whole batch of images of
different sizes) is bit-exact against Pillow running the reference's arithmetic and against the one-image entry point;
``predict_images`` returns, per batch, exactly the persons of a direct ``Model.forward`` on the same images; the demo's
``--batch_size`` writes the same files."""
import glob
import os

import numpy as np
import pytest
import torch

from multi_hmr_amd import pipeline
from multi_hmr_amd import preprocess as pp
import synthetic
from oracle import preprocess_ref as ref

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

pytestmark = pytest.mark.gpu

# (W, H): the ten geometries of tests/test_preprocess.py::SIZES, the five distinct sizes of the example photographs, a video frame
GEOMETRIES = [(640, 480), (480, 640), (1920, 1080), (333, 500), (896, 896), (100, 75), (1000, 37), (224, 224), (500, 499), (61, 4000),
              (533, 800), (452, 500), (800, 555), (800, 451), (799, 533), (1920, 1080)]
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "demo_672_s.npz"))
EXAMPLES = os.path.join(os.path.dirname(__file__), "golden", "example_data")


def _image(W, H, seed):
    """tests/test_preprocess.py::_image."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx * 255 // max(W - 1, 1)), (yy * 255 // max(H - 1, 1)), ((xx + yy) % 256)], -1).astype(np.int32)
    noise = rng.integers(-60, 60, size=(H, W, 3))
    img = np.clip(base + noise, 0, 255).astype(np.uint8)
    img[: H // 7, : W // 5] = 255                      # saturated block: exercises the clip after negative bicubic lobes
    img[H // 2:H // 2 + 3, :] = 0
    return img


def _batch_images(S):
    return [_image(W, H, W + H + S + 7 * j) for j, (W, H) in enumerate(GEOMETRIES)]


@pytest.mark.parametrize("S", [224, 448, 896])
def test_batch_of_sixteen_geometries_is_bit_exact_against_pillow(S):
    imgs = _batch_images(S)
    assert len(imgs) == 16
    pre = pp.Preprocessor(S, "cuda:0")
    x = pre.batch([torch.from_numpy(a) for a in imgs])
    assert x.shape == (16, 3, S, S) and x.dtype == torch.float32 and x.is_cuda
    got = x.cpu().numpy()
    for j, a in enumerate(imgs):
        x_ref, _ = ref.open_image_ref(Image.fromarray(a), S)
        assert np.array_equal(got[j:j + 1], x_ref), (j, GEOMETRIES[j], S)


@pytest.mark.parametrize("S", [224, 448, 896])
def test_batch_equals_the_one_image_calls_for_host_device_and_mixed_inputs(S):
    imgs = [torch.from_numpy(a) for a in _batch_images(S)]
    pre = pp.Preprocessor(S, "cuda:0")
    single = torch.cat([pre(t).clone() for t in imgs])
    host = pre.batch(imgs)
    assert torch.equal(host, single)
    device = pre.batch([t.cuda() for t in imgs])
    assert torch.equal(device, single)
    mixed = pre.batch([t.cuda() if j % 3 == 1 else t for j, t in enumerate(imgs)])
    assert torch.equal(mixed, single)
    strided = pre.batch([imgs[0].cuda().permute(1, 0, 2).contiguous().permute(1, 0, 2), imgs[1]])      # a non-contiguous device image
    assert torch.equal(strided, single[:2])
    torch.cuda.synchronize()
    assert torch.equal(host, single)                   # earlier results are not touched by later calls


def test_batch_of_one_and_of_thirty_three_with_shared_tables():
    S = 448
    pre = pp.Preprocessor(S, "cuda:0")
    sizes = [(640, 480), (333, 500), (799, 533)]
    imgs = [torch.from_numpy(_image(*sizes[j % 3], seed=j)) for j in range(33)]
    one = pre.batch(imgs[:1])
    assert one.shape == (1, 3, S, S) and torch.equal(one, pre(imgs[0]))
    x = pre.batch(imgs)
    assert x.shape == (33, 3, S, S) and len(pre._tables) == 3              # 33 images, three plans: equal sizes share their tables
    for j in range(33):
        assert torch.equal(x[j:j + 1], pre(imgs[j])), j
    with pytest.raises(ValueError):
        pre.batch([])
    with pytest.raises(ValueError):
        pre.batch([imgs[0].float()])
    with pytest.raises(ValueError):
        pre.batch([imgs[0], torch.zeros(500, 3, 3, dtype=torch.uint8)])   # the 100x aspect guard of __call__


def test_out_writes_the_callers_slice_and_nothing_else():
    S = 224
    pre = pp.Preprocessor(S, "cuda:0")
    imgs = [torch.from_numpy(_image(W, H, 3 + j)) for j, (W, H) in enumerate(GEOMETRIES[:5])]
    guard = float(np.float32(-12345.678))
    big = torch.full((9, 3, S, S), guard, device="cuda:0")
    ret = pre.batch(imgs, out=big[2:7])
    assert ret.data_ptr() == big[2].data_ptr() and ret.shape == (5, 3, S, S)
    assert torch.equal(big[2:7], pre.batch(imgs))
    assert bool((big[:2] == guard).all()) and bool((big[7:] == guard).all())
    assert not bool((big[2:7] == guard).any())


# ------------------------------------------------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def model(smplx_data, mean_params):
    """The ViT-S 672 model of tests/test_demo_config1.py."""
    from multi_hmr_amd import Model
    sd = synthetic.make_state_dict("dinov2_vits14", 672, seed=31)
    sd["mlp_classif.2.bias"] = torch.from_numpy(GOLD["classif_bias"])
    m = Model(backbone="dinov2_vits14", img_size=672, smplx_data=smplx_data, mean_params=mean_params, precision="f16")
    m.load_state_dict(sd, strict=True)
    return m.to("cuda:0").eval()


def _same_persons(a, b):
    assert len(a) == len(b)
    for ha, hb in zip(a, b):
        assert list(ha.keys()) == list(hb.keys())
        for k in ha:
            assert torch.equal(ha[k], hb[k]), k


def test_predict_images_equals_a_direct_forward_per_batch(model):
    from multi_hmr_amd import get_camera_parameters, open_image, predict_images
    S = 672
    paths = sorted(glob.glob(os.path.join(EXAMPLES, "*.jpg")))
    assert len(paths) == 7
    kw = dict(det_thresh=float(GOLD["det_thresh"]), nms_kernel_size=int(GOLD["nms_kernel_size"]))
    results = list(predict_images(model, paths, batch_size=4, fov=60, **kw))
    assert [r.index for r in results] == list(range(7)) and [r.source for r in results] == paths
    assert all(r.error is None for r in results)
    counts = [len(r.humans) for r in results]
    print("persons per image:", counts)
    assert any(counts)

    for lo, hi in ((0, 4), (4, 7)):                                        # batches of 4 and 3
        x = torch.cat([open_image(p, S, torch.device("cuda:0"))[0] for p in paths[lo:hi]])
        K = get_camera_parameters(S, fov=60, device=torch.device("cuda:0"), batch=hi - lo)
        humans, ids = model(x, is_training=False, K=K, return_image_index=True, **kw)
        ids = ids.tolist()
        for b in range(hi - lo):
            r = results[lo + b]
            _same_persons(r.humans, [h for h, i in zip(humans, ids) if i == b])
            assert torch.equal(r.K, K[b:b + 1])

    for r, p in zip(results, paths):
        size = Image.open(p).size
        assert r.size == size
        want = get_camera_parameters(S, fov=60, device=torch.device("cuda:0"))          # the reference's demo, before it draws
        ratio = max(size) / S
        want[0, 0, 2] = size[0] / 2.0
        want[0, 1, 2] = size[1] / 2.0
        want[0, [0, 1], [0, 1]] = ratio * want[0, [0, 1], [0, 1]]
        assert torch.equal(r.K_full, want)

    again = list(predict_images(model, paths, batch_size=4, fov=60, **kw))
    for r, r2 in zip(results, again):
        _same_persons(r.humans, r2.humans)
        assert torch.equal(r.K_full, r2.K_full)


def test_predict_images_takes_mixed_sources_and_skips_a_broken_file(model, tmp_path):
    from multi_hmr_amd import predict_images
    paths = sorted(glob.glob(os.path.join(EXAMPLES, "*.jpg")))[:3]
    broken = tmp_path / "broken.jpg"
    broken.write_bytes(b"not an image")
    kw = dict(det_thresh=float(GOLD["det_thresh"]), nms_kernel_size=int(GOLD["nms_kernel_size"]), batch_size=4)
    base = list(predict_images(model, paths, **kw))
    sources = iter([paths[0], str(broken), Image.open(paths[1]), np.asarray(Image.open(paths[2]).convert("RGB"))])
    got = list(predict_images(model, sources, on_error="skip", **kw))
    assert [r.index for r in got] == [0, 1, 2, 3]
    assert got[1].humans is None and got[1].error is not None and got[1].K_full is None
    for r, r0 in zip([got[0], got[2], got[3]], base):                      # the same three images in one batch of three
        _same_persons(r.humans, r0.humans)
        assert r.size == r0.size
    with pytest.raises(pipeline.PipelineError, match="broken.jpg"):
        list(predict_images(model, [paths[0], str(broken)], **kw))


def test_demo_batch_size_writes_the_same_files(model, tmp_path, monkeypatch):
    from multi_hmr_amd import demo
    monkeypatch.setattr(demo, "load_model", lambda name, *a, **k: model)
    base = ["--model_name", "synthetic_672_S", "--img_folder", EXAMPLES, "--det_thresh", str(float(GOLD["det_thresh"])),
            "--nms_kernel_size", str(int(GOLD["nms_kernel_size"])), "--extra_views", "1", "--save_rotating_video", "0"]
    one = demo.main(base + ["--out_folder", str(tmp_path / "b1")])
    four = demo.main(base + ["--out_folder", str(tmp_path / "b4"), "--batch_size", "4"])
    assert len(one) == 7 and [os.path.basename(p) for p in one] == [os.path.basename(p) for p in four]
    assert sorted(os.listdir(tmp_path / "b1")) == sorted(os.listdir(tmp_path / "b4"))
    for p1, p4, src in zip(one, four, sorted(glob.glob(os.path.join(EXAMPLES, "*.jpg")))):
        W, H = Image.open(src).size
        assert Image.open(p4).size == (3 * W, H) == Image.open(p1).size   # [input | overlay | view]


def test_default_device_preprocessor_batches_with_and_without_out():
    """``Preprocessor(S)`` keeps the index-less default device ("cuda"), which compares unequal to every tensor's "cuda:0"."""
    S = 224
    pre = pp.Preprocessor(S)
    assert pre.device == torch.device("cuda")
    imgs = [torch.from_numpy(_image(W, H, 11 + j)) for j, (W, H) in enumerate(GEOMETRIES[:3])]
    want = torch.cat([pp.Preprocessor(S, "cuda:0")(t) for t in imgs])
    x = pre.batch(imgs)
    assert x.device == torch.device("cuda", torch.cuda.current_device()) and torch.equal(x, want)
    out = torch.zeros(3, 3, S, S, device="cuda")
    assert pre.batch([t.cuda() for t in imgs], out=out).data_ptr() == out.data_ptr() and torch.equal(out, want)
    for bad in (torch.zeros(2, 3, S, S, device="cuda"), torch.zeros(3, 3, S, S, device="cuda", dtype=torch.float64),
                torch.zeros(3, 3, S, S), torch.zeros(3, 3, S, 2 * S, device="cuda")[..., ::2]):
        with pytest.raises(ValueError):
            pre.batch(imgs, out=bad)
