"""Generator of tests/golden/distance_labels.npz: the reference's OWN ``get_bbox`` and ``print_distance_on_image``
(utils/render.py:365-405, imported by path with ``pyrender`` / ``trimesh`` stubbed as oracle/ref_shim.py stubs them) on seeded inputs.

Recorded: the inputs (2D joints, pelvis translations, colours, the image size), every person's box in both formats, and every label
the reference draws -- its text, its fill colour and the point it is centred on (the top centre of the box scaled by 1.35).  The
text's anchor is that point moved left by half the text's length in the default font; the generator checks that against the call the
reference makes, and the test derives it again with its own Pillow, so the golden does not depend on this machine's font.

Runs only where the reference tree exists:  python tests/golden/make_golden_distance.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.ref_shim import REFERENCE_ROOT  # noqa: E402


def main():
    import PIL
    from PIL import ImageFont
    for name in ("pyrender", "trimesh"):
        sys.modules.setdefault(name, types.ModuleType(name))
    import importlib.util
    spec = importlib.util.spec_from_file_location("reference_utils_render", os.path.join(REFERENCE_ROOT, "utils", "render.py"))
    ref = importlib.util.module_from_spec(spec)                           # the reference's utils/render.py, by path: the package's
    spec.loader.exec_module(ref)                                          # __init__ would import the whole model

    rng = np.random.default_rng(20240607)
    n, W, H = 6, 640, 480
    centre = rng.uniform([60, 80], [W - 60, H - 80], size=(n, 1, 2))
    spread = rng.uniform(15, 90, size=(n, 1, 2))
    j2d = (centre + spread * rng.standard_normal((n, 127, 2))).astype(np.float32)
    j2d[5] -= 300                                                         # one person mostly outside the image (negative boxes)
    transl = rng.uniform([-2, -1, 1.5], [2, 1, 9], size=(n, 1, 3)).astype(np.float32)
    colors = rng.integers(1, 225, size=(n, 3)).astype(np.float64) / 255
    image = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)

    xywh = np.array([ref.get_bbox(j, factor=1.35, output_format="xywh") for j in j2d], np.int64)
    x1y1x2y2 = np.array([ref.get_bbox(j, factor=1.35, output_format="x1y1x2y2") for j in j2d], np.int64)
    plain = np.array([ref.get_bbox(j) for j in j2d], np.int64)               # the defaults: factor 1, xywh

    calls = []

    class Draw:
        def __init__(self, real):
            self.real = real

        def text(self, xy, txt, fill=None, font=None):
            calls.append((tuple(float(v) for v in xy), txt, tuple(int(v) for v in fill)))
            return self.real.text(xy, txt, fill=fill, font=font)

    real_draw = ref.ImageDraw.Draw
    ref.ImageDraw = types.SimpleNamespace(Draw=lambda im: Draw(real_draw(im)))
    humans = [{"transl_pelvis": torch.from_numpy(transl[i]), "j2d_smplx": torch.from_numpy(j2d[i])} for i in range(n)]
    out = ref.print_distance_on_image(image.copy(), humans, [tuple(c) for c in colors])
    assert out.shape == image.shape and len(calls) == n and not np.array_equal(out, image)

    font = ImageFont.load_default()
    points = np.array([[(b[0] + b[2]) / 2.0, b[1]] for b in x1y1x2y2], np.float64)
    for (xy, txt, _), pt in zip(calls, points):                           # the reference anchors the text at point - length // 2
        assert xy == (pt[0] - font.getlength(txt) // 2, pt[1]), (xy, pt, txt)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "distance_labels.npz")
    np.savez_compressed(path, j2d=j2d, transl_pelvis=transl, colors=colors, image_size=np.array([W, H]), bbox_xywh=xywh,
                        bbox_x1y1x2y2=x1y1x2y2, bbox_default=plain, texts=np.array([c[1] for c in calls]),
                        fills=np.array([c[2] for c in calls], np.int64), points=points, pillow_version=np.array(PIL.__version__))
    print(path, os.path.getsize(path), "bytes;", [c[1] for c in calls], x1y1x2y2.tolist())


if __name__ == "__main__":
    main()
