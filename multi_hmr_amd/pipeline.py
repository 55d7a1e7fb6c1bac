"""From image files to persons at the batch size the model is fast at: ``predict_images(model, sources, batch_size=32)`` decodes
(PIL, on a thread pool), preprocesses each batch in one ``Preprocessor.batch`` call, runs ONE ``Model.forward`` per batch and yields
every image's persons in input order.

Two layers:
  * ``run_batched``: the scheduling core -- ordering, batching, the partial last batch, the error policy and the look-ahead -- over
    injected ``decode`` / ``preprocess`` / ``forward`` callables.  It knows nothing of the device (tests drive it with fakes).
  * ``predict_images``: the callables of the real thing and the per-image camera matrices; ``predict_video``: the same for the
    consecutive frames of a clip, with the persons tracked and smoothed across frames (``multi_hmr_amd.track``).

Threads, not processes: PIL releases the GIL while it decodes, and exactly one process has the GPU open.  While the forward of batch n
is in flight a producer thread decodes and stages batch n + 1 (its pinned staging buffer is packed, its copy and its two preprocessing
launches are enqueued behind the forward's on the same stream); at most ``LOOKAHEAD`` batches are decoded ahead of the forward, so host
memory stays bounded however long the folder is."""
from __future__ import annotations

import queue
import threading
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Any

DEFAULT_WORKERS = 8
MAX_WORKERS = 16                    # a fixed cap: the CPU count a machine shows is not the count a job may use
LOOKAHEAD = 2                       # decoded batches that may exist ahead of the forward


class PipelineError(RuntimeError):
    """A source could not be decoded (``on_error="raise"``); the message names it, ``__cause__`` is the decoder's exception."""


@dataclass
class ImageResult:
    index: int                      # position in ``sources``
    source: Any                     # the source as given
    humans: list | None             # the person dicts of Model.forward for this image; None if it could not be decoded
    K: Any = None                   # [1, 3, 3] intrinsics of the S x S model input
    K_full: Any = None              # [1, 3, 3] intrinsics of the full-resolution image (what overlay_human_meshes takes)
    size: tuple | None = None       # (width, height) of the decoded image
    error: BaseException | None = None


def clamp_workers(workers) -> int:
    return max(1, min(int(workers), MAX_WORKERS))


def describe(source) -> str:
    """How a source is named in an error: the path, a PIL image's file name if it has one, else its type."""
    if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
        return repr(source)
    name = getattr(source, "filename", None)
    return repr(name) if name else f"<{type(source).__name__}>"


def run_batched(sources, decode, preprocess, forward, batch_size=32, workers=DEFAULT_WORKERS, on_error="raise"):
    """Generator over ``(index, source, item, output, error)`` in input order.

    ``decode(source) -> item`` runs on ``workers`` threads; ``preprocess(items) -> staged`` runs once per batch on the producer
    thread, as soon as the batch is decoded; ``forward(staged, items) -> outputs`` (one per item) runs on the caller's thread.
    A batch is ``batch_size`` consecutive sources (the last one: what is left), less those whose decode raised.
    ``on_error="raise"``: the first such source raises ``PipelineError`` when its batch is reached -- every earlier batch has been
    delivered, nothing of its own batch is, and no forward is spent on it; ``"skip"``: it is yielded with
    ``item = output = None`` and its exception, and takes no part in the batch.  An exception of ``preprocess`` or ``forward`` is
    not a property of one source and is always raised.  However the generator ends (exhausted, closed early or by an exception),
    the producer thread and the pool have ended when it returns."""
    if on_error not in ("raise", "skip"):
        raise ValueError('on_error must be "raise" or "skip"')
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("batch_size must be at least 1")
    ready = queue.Queue()                              # bounded by `slots`, not by the queue
    slots = threading.Semaphore(LOOKAHEAD)             # one per batch decoded (or being decoded) that the consumer has not taken yet
    stop = threading.Event()
    pool = ThreadPoolExecutor(max_workers=clamp_workers(workers), thread_name_prefix="mhmr-decode")

    def produce():
        try:
            it, first, done = iter(sources), 0, False
            while not done:
                slots.acquire()
                if stop.is_set():
                    return
                srcs = []
                while len(srcs) < batch_size:
                    try:
                        srcs.append(next(it))
                    except StopIteration:
                        done = True
                        break
                if not srcs:
                    break
                futures = [pool.submit(decode, s) for s in srcs]
                items, errors = [], []
                for f in futures:
                    e = f.exception()
                    errors.append(e)
                    items.append(None if e is not None else f.result())
                good = [x for x, e in zip(items, errors) if e is None]
                failed = any(e is not None for e in errors)
                staged = preprocess(good) if good and not stop.is_set() and not (failed and on_error == "raise") else None
                ready.put(("batch", first, srcs, items, errors, staged))
                first += len(srcs)
            ready.put(("end",))
        except BaseException as e:                     # the sources iterator or preprocess raised: hand it to the consumer
            ready.put(("fail", e))

    producer = threading.Thread(target=produce, name="mhmr-pipeline", daemon=True)
    producer.start()
    try:
        while True:
            msg = ready.get()
            if msg[0] == "end":
                return
            if msg[0] == "fail":
                raise msg[1]
            _, first, srcs, items, errors, staged = msg
            slots.release()                            # the producer may start on the batch after the next one
            if on_error == "raise":
                for s, e in zip(srcs, errors):
                    if e is not None:
                        raise PipelineError(f"could not decode {describe(s)}: {type(e).__name__}: {e}") from e
            good = [x for x, e in zip(items, errors) if e is None]
            outputs = iter(forward(staged, good) if good else ())
            for j, (s, x, e) in enumerate(zip(srcs, items, errors)):
                yield first + j, s, x, (next(outputs) if e is None else None), e
    finally:
        stop.set()
        for _ in range(LOOKAHEAD):
            slots.release()
        producer.join()
        pool.shutdown(wait=True, cancel_futures=True)


def full_resolution_K(K, size, img_size):
    """The intrinsics of the full-resolution image from those of the S x S input, as the reference's demo makes them before it
    draws: focal lengths times ``max(size) / S``, principal point at the image centre.  ``K`` [1, 3, 3] is not modified."""
    K_full = K.clone()
    K_full[0, 0, 2] = size[0] / 2.0
    K_full[0, 1, 2] = size[1] / 2.0
    K_full[0, [0, 1], [0, 1]] = (max(size) / img_size) * K_full[0, [0, 1], [0, 1]]
    return K_full


def decode_image(source):
    """A file path, a PIL image or a uint8 ``[H, W, 3]`` array / tensor -> ``(uint8 [H, W, 3] tensor, (width, height))``.  Decoding is
    PIL's, as in the reference (``Image.open(path).convert("RGB")``)."""
    import numpy as np
    import torch
    if torch.is_tensor(source):
        img = source
    elif isinstance(source, np.ndarray):
        img = torch.from_numpy(source if source.flags.writeable else source.copy())       # torch refuses read-only arrays
    else:
        from PIL import Image
        pil = source if isinstance(source, Image.Image) else Image.open(source)
        img = torch.from_numpy(np.array(pil.convert("RGB")))
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError("expected a uint8 [H, W, 3] RGB image")
    H, W = int(img.shape[0]), int(img.shape[1])
    if H == 0 or W == 0 or H > W * 100:                # the guard of Preprocessor, here so that the error names the source
        raise ValueError(f"unsupported image size {W}x{H}")
    return img, (W, H)


class _Stages:
    """What ``predict_images`` and ``predict_video`` share: the device, the preprocessor, the ONE stream of the iteration, the stage timers
    and the ``decode`` / ``preprocess`` callables of ``run_batched``."""

    def __init__(self, model, stats):
        import torch
        from .preprocess import Preprocessor
        self.dev = next(model.parameters()).device
        self.S = int(model.img_size)
        self.pre = Preprocessor(self.S, self.dev)
        self.stream = torch.cuda.current_stream(self.dev)
        self.st = stats if stats is not None else {}
        for k in ("decode", "stage", "forward", "wait"):
            self.st.setdefault(k, 0.0)
        for k in ("images", "batches"):
            self.st.setdefault(k, 0)
        self.lock = threading.Lock()

    def decode(self, source):
        import time
        t0 = time.perf_counter()
        try:
            return decode_image(source)
        finally:
            dt = time.perf_counter() - t0
            with self.lock:
                self.st["decode"] += dt

    def preprocess(self, items):
        import time
        import torch
        t0 = time.perf_counter()
        with torch.cuda.stream(self.stream):           # the producer thread enqueues on the iteration's stream
            x = self.pre.batch([img for img, _ in items])
        self.st["stage"] += time.perf_counter() - t0
        return x

    def results(self, forward, sources, batch_size, workers, on_error):
        """``run_batched`` with these stages and ``forward(x, items) -> [(humans, K [1, 3, 3])]`` -> the ``ImageResult`` of every source."""
        import time
        st, S = self.st, self.S
        gen = run_batched(sources, self.decode, self.preprocess, forward, batch_size=batch_size, workers=workers, on_error=on_error)
        consumed = 0.0
        try:
            while True:
                t0 = time.perf_counter()
                try:
                    index, source, item, output, error = next(gen)
                except StopIteration:
                    return
                finally:
                    consumed += time.perf_counter() - t0
                    st["wait"] = consumed - st["forward"]
                if error is not None:
                    yield ImageResult(index, source, None, error=error)
                    continue
                humans, K = output
                size = item[1]
                yield ImageResult(index, source, humans, K, full_resolution_K(K, size, S), size)
        finally:
            gen.close()


OCCLUSION_KEYS = ("visible_px", "amodal_px", "occlusion", "bbox_visible")


def add_occlusion(model, persons, verts, image_index, K, size):
    """Adds ``OCCLUSION_KEYS`` to the person dicts of one batch (``persons`` in the row order of ``verts`` [P, V, 3] and ``image_index``
    [P]): one ``maps.render_maps`` call with geometry only, in the model-input camera ``K`` [B, 3, 3] at ``size`` x ``size`` pixels.
    ``visible_px`` / ``amodal_px`` (int32 scalars), ``occlusion`` (float32 scalar: the share of the person hidden behind others) and
    ``bbox_visible`` (int32 [4]: x0, y0, x1, y1 inclusive; W, H, -1, -1 when nothing is visible) are device tensors."""
    if not persons:
        return
    from .maps import render_maps
    faces = next(iter(model.smpl_layer.values())).bm_x.faces
    m = render_maps(verts, image_index, K, faces, (size, size))
    cols = [t.unbind(0) for t in (m.visible_px, m.amodal_px, m.occlusion, m.bbox)]
    for h, vals in zip(persons, zip(*cols)):
        h.update(zip(OCCLUSION_KEYS, vals))


CONTACT_KEYS = ("penetration_depth", "inside_vertices", "contact_vertices", "contact_with")


def add_contacts(model, persons, verts, image_index, max_dist=0.10, tau=0.01):
    """Adds ``CONTACT_KEYS`` to the person dicts of one batch (``persons`` in the row order of ``verts`` [P, V, 3] and ``image_index``
    [P]): one ``contact.contacts`` call and one copy to the host.  ``penetration_depth`` (float, metres: how deep the person's deepest
    vertex lies inside another person), ``inside_vertices`` and ``contact_vertices`` (int: vertices inside another person, and within
    ``tau`` of another person's surface) and ``contact_with`` (the indices, within the image's ``humans`` list, of the persons whose
    symmetric pair distance is <= ``tau``).  The margins are conventions (``contact.contacts``)."""
    if not persons:
        return
    import torch
    from .contact import contacts as _contacts
    faces = next(iter(model.smpl_layer.values())).bm_x.faces
    c = _contacts(verts, image_index, faces, max_dist=max_dist, tau=tau,
                  want=("penetration_depth", "inside_count", "contact_count", "pair_distance"))
    P = len(persons)
    ids = torch.as_tensor(image_index).reshape(-1).to(c.pair_distance.device)
    touching = torch.minimum(c.pair_distance, c.pair_distance.T) <= tau
    host = torch.cat([c.penetration_depth.double(), c.inside_count.double(), c.contact_count.double(), ids.double(),
                      touching.double().reshape(-1)]).tolist()                                      # the one copy to the host
    pen, nin, nct, img, touch = host[:P], host[P:2 * P], host[2 * P:3 * P], host[3 * P:4 * P], host[4 * P:]
    first = {}
    for p in range(P):                                                  # a person's index within their image: rows of one image are in order
        first.setdefault(img[p], []).append(p)
    rank = {p: j for rows in first.values() for j, p in enumerate(rows)}
    for p, h in enumerate(persons):
        h.update(zip(CONTACT_KEYS, (pen[p], int(nin[p]), int(nct[p]), [rank[q] for q in first[img[p]] if touch[p * P + q]])))


def predict_images(model, sources, batch_size=32, fov=60, det_thresh=0.3, nms_kernel_size=3, workers=DEFAULT_WORKERS,
                   on_error="raise", stats=None, occlusion=False, contacts=False):
    """Generator of one ``ImageResult`` per source, in input order.  ``sources``: file paths, PIL images or uint8 ``[H, W, 3]``
    arrays, in any mix; any iterable, an iterator of unknown length (video frames) included.  One ``Model.forward`` per
    ``batch_size`` images (the last batch at its own size), ``r.humans`` = that image's person dicts.  ``r.K`` is the camera of the
    model input, ``r.K_full`` the one of the full-resolution image, so ``overlay_human_meshes(r.humans, faces, r.K_full, model, img)``
    works unchanged.  ``on_error="skip"`` yields an undecodable source with ``humans=None`` and ``r.error`` instead of raising.
    Runs on the model's device, and all of it -- every batch's preprocessing and forward -- on ONE stream: the one that is current
    when the iteration starts, whatever the caller makes current between two results.  ``stats``: a dict that receives the seconds spent per stage
    (``decode`` summed over the worker threads, ``stage`` = packing + enqueueing on the producer thread, ``forward`` and ``wait`` =
    the consumer waiting for a staged batch) and the counts ``images`` / ``batches``.  ``occlusion=True`` adds ``visible_px``,
    ``amodal_px``, ``occlusion`` and ``bbox_visible`` to every person dict (``add_occlusion``: one ``maps.render_maps`` call per batch,
    in the model-input camera ``r.K``); the other keys are untouched.  ``contacts=True`` adds ``penetration_depth``, ``inside_vertices``,
    ``contact_vertices`` and ``contact_with`` (``add_contacts``: one ``contact.contacts`` call per batch, at its default margins); the other
    keys are untouched."""
    import time
    import torch
    from .preprocess import get_camera_parameters
    sg = _Stages(model, stats)
    st, S, dev = sg.st, sg.S, sg.dev

    def forward(x, items):
        t0 = time.perf_counter()
        B = x.shape[0]
        with torch.cuda.stream(sg.stream):             # the stream the batch was preprocessed on
            K = get_camera_parameters(S, fov=fov, device=dev, batch=B)
            humans, ids = model(x, is_training=False, nms_kernel_size=int(nms_kernel_size), det_thresh=det_thresh, K=K,
                                return_image_index=True)
            if occlusion and humans:
                from .demo import _stacked
                add_occlusion(model, humans, _stacked([h["v3d"] for h in humans]), ids, K, S)
            if contacts and humans:
                from .demo import _stacked
                add_contacts(model, humans, _stacked([h["v3d"] for h in humans]), ids)
        per_image = [[] for _ in range(B)]
        for h, i in zip(humans, ids.tolist()):
            per_image[i].append(h)
        st["forward"] += time.perf_counter() - t0
        st["batches"] += 1
        st["images"] += B
        return [(per_image[b], K[b:b + 1]) for b in range(B)]

    yield from sg.results(forward, sources, batch_size, workers, on_error)


def predict_video(model, frames, batch_size=32, tracker=None, fov=60, det_thresh=0.3, nms_kernel_size=3, workers=DEFAULT_WORKERS,
                  on_error="raise", stats=None, occlusion=False, contacts=False):
    """``predict_images`` for the consecutive frames of one clip: the same sources, batching, stream, ``ImageResult`` and ``stats``, with the
    persons TRACKED and SMOOTHED across frames and batches.  Per batch: one ``Model.forward`` (``return_batched=True,
    return_readout=True``), one ``Tracker.update`` and one ``decode_readout`` of the filtered rows.  Every person dict holds the ten
    ``Model.PERSON_KEYS`` of the smoothed person (``scores`` is the detection's) plus ``track_id`` (int; -1: the tracker's table was full)
    and ``hits`` (int; frames the track has been seen in).  ``tracker``: a ``Tracker`` of this model (its table persists, so a second clip
    needs ``tracker.reset()``); ``None``: ``Tracker(model)``.  ``occlusion`` and ``contacts`` as in ``predict_images``, of the smoothed persons.  A ``Tracker(model, smooth=None)`` only tracks: the persons are
    ``predict_images``' bit for bit.  The ids go to the host in one copy per batch, and the tracker's ``status`` is checked there (it raises
    ``RuntimeError``).  A source that ``on_error="skip"`` skips is not shown to the tracker: for it no time passes."""
    import time
    import torch
    from .preprocess import get_camera_parameters
    from .track import Tracker
    sg = _Stages(model, stats)
    st, S, dev = sg.st, sg.S, sg.dev
    tracker = tracker if tracker is not None else Tracker(model)
    keys = model.PERSON_KEYS

    def forward(x, items):
        t0 = time.perf_counter()
        B = x.shape[0]
        with torch.cuda.stream(sg.stream), torch.no_grad():
            K = get_camera_parameters(S, fov=fov, device=dev, batch=B)
            out, ids = model(x, is_training=False, nms_kernel_size=int(nms_kernel_size), det_thresh=det_thresh, K=K, return_batched=True,
                             return_readout=True)
            res = tracker.update(out, ids, B)
            per_image = [[] for _ in range(B)]
            if out:
                dec = model.decode_readout(res.readout, res.offset, out["idx"], K)
                cols = [(out["scores"] if n == "scores" else dec[n].detach()).unbind(0) for n in keys]
                Pn = int(ids.shape[0])
                host = torch.cat([res.status.long(), ids.long(), res.track_id, res.hits.long()]).tolist()     # the one copy to the host
            else:
                cols, Pn, host = [], 0, res.status.tolist()
            if host[0] != 0:
                raise RuntimeError(f"Tracker.update refused the batch (status {host[0]}): the image ids of the forward are not ascending")
            rows = []
            for p, vals in enumerate(zip(*cols)):
                h = dict(zip(keys, vals))
                h["track_id"], h["hits"] = host[1 + Pn + p], host[1 + 2 * Pn + p]
                per_image[host[1 + p]].append(h)
                rows.append(h)
            if occlusion and rows:
                add_occlusion(model, rows, dec["v3d"].detach(), ids, K, S)
            if contacts and rows:
                add_contacts(model, rows, dec["v3d"].detach(), ids)
        st["forward"] += time.perf_counter() - t0
        st["batches"] += 1
        st["images"] += B
        return [(per_image[b], K[b:b + 1]) for b in range(B)]

    yield from sg.results(forward, frames, batch_size, workers, on_error)
