#!/usr/bin/env python
"""Throughput of mhmr_preprocess_u8 (device-resident decoded frames -> normalised [3,S,S]) vs PIL on the host cores, and of
Preprocessor.batch (mhmr_preprocess_u8_batch) against the loop of one-image calls it replaces (``batch_leg``)."""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multi_hmr_amd import preprocess as pp
from oracle import preprocess_ref as ref
from PIL import Image

W, H, S, n = 1920, 1080, 896, 200
rng = np.random.default_rng(0)
img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
pre = pp.Preprocessor(S, "cuda:0")
d = torch.from_numpy(img).cuda()
out = torch.empty(32, 3, S, S, device="cuda:0")
for i in range(4):
    pre(d, out=out[i % 32])
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for i in range(n):
    pre(d, out=out[i % 32])
e1.record(); torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / n
bytes_alg = H * W * 3 + 3 * S * S * 4
print(f"GPU  {W}x{H} -> {S}: {ms*1e3:.1f} us/image, {1e3/ms:.0f} images/s, {bytes_alg/ms/1e6:.1f} GB/s algorithmic (in u8 + out f32)")
pil = Image.fromarray(img)
t0 = time.perf_counter()
for _ in range(5):
    ref.open_image_ref(pil, S)
t = (time.perf_counter() - t0) / 5
print(f"PIL (1 core) {t*1e3:.1f} ms/image, {1/t:.1f} images/s")


def batch_leg(reps=30, warm=3):
    """Preprocessor.batch against a loop of Preprocessor.__call__ over the same 32 images (S = 896: the seven example-photograph sizes
    cycled + four 1920x1080 frames), in this process, alternating, device events around work that ends in a synchronise; once with
    device-resident inputs and once with host inputs (copies included).  Prints medians, spreads and the algorithmic bytes."""
    photo = [(533, 800), (452, 500), (800, 555), (800, 451), (799, 533), (799, 533), (799, 533)]
    sizes = [photo[j % 7] for j in range(28)] + [(1920, 1080)] * 4
    host = [torch.from_numpy(np.random.default_rng(j).integers(0, 256, size=(h, w, 3), dtype=np.uint8)) for j, (w, h) in enumerate(sizes)]
    dev = [t.cuda() for t in host]
    B = len(host)
    x_loop, x_batch = torch.empty(B, 3, S, S, device="cuda:0"), torch.empty(B, 3, S, S, device="cuda:0")
    bytes_alg = sum(t.numel() for t in host) + B * 3 * S * S * 4

    def loop(imgs):
        for b, t in enumerate(imgs):
            pre(t, out=x_loop[b])

    def timed(fn, imgs):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn(imgs)
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z)

    print(f"batch leg: {B} images -> {S}, {bytes_alg / 1e6:.1f} MB algorithmic (sum H W 3 in + B 3 S^2 4 out), {reps} alternating repetitions")
    for name, imgs in (("device inputs", dev), ("host inputs", host)):
        for _ in range(warm):
            loop(imgs)
            pre.batch(imgs, out=x_batch)
        torch.cuda.synchronize()
        assert torch.equal(x_loop, x_batch)
        t_loop, t_batch = [], []
        for _ in range(reps):
            t_loop.append(timed(loop, imgs))
            t_batch.append(timed(lambda im: pre.batch(im, out=x_batch), imgs))
        q = lambda v: np.percentile(v, [50, 10, 90])
        (ml, l10, l90), (mb, b10, b90) = q(t_loop), q(t_batch)
        print(f"  {name}: loop of {B} calls (2 launches each) median {ml:.3f} ms [p10 {l10:.3f}, p90 {l90:.3f}]; "
              f"batch (2 launches) median {mb:.3f} ms [p10 {b10:.3f}, p90 {b90:.3f}]; loop / batch = {ml / mb:.2f}; "
              f"batch: {bytes_alg / mb / 1e6:.1f} GB/s algorithmic, {B / mb * 1e3:.0f} images/s")
        assert mb <= ml, "the batch call must not be slower than the loop it replaces"


batch_leg()
