"""Drop-in for the reference ``demo.py``: the inference helpers (lines 27-126: ``open_image``, ``get_camera_parameters``,
``load_model``, ``forward_model``), ``overlay_human_meshes`` (lines 128-158, drawn by ``render.render_batch`` on the GPU),
``create_rotating_video`` (lines 160-241, every rotated frame drawn by one ``render.render_views`` call) and the command line
(lines 231-386: ``python -m multi_hmr_amd.demo``, writing ``[input | overlay]`` side by side, ``[input | overlay | view]`` with
``--extra_views 1``, and the rotating video with ``--save_rotating_video 1``; ``--save_mesh 1`` adds the vertices as ``.npy`` and the
scene as ``.glb``, ``--distance 1`` writes every person's distance on the overlay: ``scene.py``).  The video is written as an animated
PNG, not mp4 (no video encoder here)."""
from __future__ import annotations

import os

import numpy as np
import torch

from .model import Model

from .preprocess import IMG_NORM_MEAN, IMG_NORM_STD, get_camera_parameters, open_image  # noqa: F401  (demo.py:27-68 on the GPU)
from .scene import create_scene, get_bbox, print_distance_on_image  # noqa: F401  (utils/render.py:62-173, 365-405)

CACHE_DIR_MULTIHMR = "models/multiHMR"          # reference utils/constants.py:9


def load_model(model_name, device=torch.device("cuda"), **model_kwargs):
    """demo.py:70-106: checkpoint -> ``Model(**vars(ckpt['args']))`` -> ``load_state_dict(strict=False)``.
    No download is attempted (no network); the checkpoint must exist under models/multiHMR/."""
    ckpt_path = os.path.join(CACHE_DIR_MULTIHMR, model_name + ".pt")
    if not os.path.isfile(ckpt_path):
        raise FileNotFoundError(f"{ckpt_path} not found")
    ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=False)
    kwargs = dict(vars(ckpt["args"]))
    if "anny" in ckpt_path:                      # demo.py:94-95: the Anny checkpoints build multi_hmr_anny.multi_hmr.Multi_HMR
        from .anny_model import Multi_HMR as ModelAnny
        kwargs.update(model_kwargs)
        model = ModelAnny(**kwargs).to(device)
    else:
        kwargs["type"] = ckpt["args"].train_return_type
        kwargs["img_size"] = ckpt["args"].img_size[0]
        kwargs.update(model_kwargs)
        model = Model(**kwargs).to(device)
    model.load_state_dict(ckpt["model_state_dict"], strict=False)
    return model


def forward_model(model, input_image, camera_parameters, det_thresh=0.3, nms_kernel_size=1, use_graph=False):
    """demo.py:108-126.  The reference wraps the call in fp16 autocast; ``Model.forward`` disables autocast for
    its own body, so the precision is whatever ``Model(precision=...)`` selected.
    Extension: ``use_graph=True`` replays the forward from a hipGraph recorded on first use for this batch size / threshold / NMS window
    (``graphed.GraphedForward``: same kernels, same results; what it saves is the host's per-launch work, which matters at batch 1)."""
    if use_graph:
        from .graphed import graphed
        return graphed(model, input_image.shape[0], det_thresh, nms_kernel_size)(input_image.float(), camera_parameters.float())
    with torch.no_grad():
        with torch.autocast("cuda", enabled=True):
            humans = model(input_image, is_training=False, nms_kernel_size=int(nms_kernel_size), det_thresh=det_thresh,
                           K=camera_parameters)
    return humans


def _stacked(tensors):
    """[P, V, 3] over the persons' vertex tensors: a strided view when they are equally spaced rows of one block (the forward's
    output block), a device-side stack otherwise; never a host copy of vertices that are already on the device."""
    t0 = tensors[0]
    if all(torch.is_tensor(t) and t.is_cuda for t in tensors):
        if t0.is_contiguous() and all(t.shape == t0.shape and t.dtype == t0.dtype and t.is_contiguous() and
                                      t.untyped_storage().data_ptr() == t0.untyped_storage().data_ptr() for t in tensors):
            step = (tensors[1].storage_offset() - t0.storage_offset()) if len(tensors) > 1 else t0.numel()
            if step >= t0.numel() and all(t.storage_offset() == t0.storage_offset() + j * step for j, t in enumerate(tensors)):
                return t0.as_strided((len(tensors),) + tuple(t0.shape), (step,) + tuple(t0.stride()))
        return torch.stack(tensors)
    return torch.stack([torch.as_tensor(np.asarray(t.cpu() if torch.is_tensor(t) else t, np.float32)) for t in tensors]).cuda()


def overlay_human_meshes(humans, faces, K, model, img_pil, unique_color=False, alpha=0.8, _color=None):
    """demo.py:128-158: the persons' meshes (``verts_smplx`` if present, else ``v3d``) drawn over ``img_pil`` with the camera
    K[0] -> ``(np.uint8 [H, W, 3], colours)``.  One ``render.render_batch`` call on the vertices' device.  Unlike the reference,
    a rendering error is raised, not printed."""
    from .render import PALETTE, render_batch
    if _color is None:
        _color = [PALETTE[0] for _ in range(len(humans))] if unique_color else PALETTE
    img = np.asarray(img_pil)
    if len(humans) == 0:
        return img, _color
    name = "verts_smplx" if "verts_smplx" in humans[0] else "v3d"
    verts = _stacked([h[name] for h in humans])
    Kc = torch.as_tensor(K)[0].detach().float().cpu().reshape(1, 3, 3)
    images = torch.from_numpy(np.array(img[..., :3], np.uint8))[None].to(verts.device)
    cols = [_color[j % len(_color)] for j in range(len(humans))]
    out = render_batch(images, verts, torch.zeros(len(humans), dtype=torch.int32), Kc, faces, colors=cols, alpha=alpha)
    return out[0].cpu().numpy(), _color


def orbit_extrinsics(center, axis, angles):
    """View extrinsics [n, 3, 4] float64 that turn the scene about ``center`` (3,) by each angle (degrees) about the camera's 'x' or
    'y' axis: the reference's ``x' = (x - c) R^T + c`` (demo.py:160-186, its R_y / R_x) written as ``[R | c - R c]``."""
    c = np.asarray(center, np.float64).reshape(3)
    out = []
    for angle in angles:
        th = np.deg2rad(angle)
        cs, sn = np.cos(th), np.sin(th)
        if axis == "y":
            R = np.array([[cs, 0, sn], [0, 1, 0], [-sn, 0, cs]])
        elif axis == "x":
            R = np.array([[1, 0, 0], [0, cs, -sn], [0, sn, cs]])
        else:
            raise ValueError("Axis must be 'x' or 'y'")
        out.append(np.concatenate([R, (c - R @ c)[:, None]], 1))
    return np.stack(out) if out else np.zeros((0, 3, 4))


def create_rotating_video(humans, faces, K, model, img_pil_visu, unique_color=False, alpha=0.8, fn='rotating.mp4', n_frames=20,
                          angle_range=60, _color=None):
    """demo.py:188-241: the persons turned about person 0's centre, swept to +angle_range about y, to -angle_range about y and to
    +angle_range about x and back, over a white image, with ``n_frames // 4`` copies of the overlay over the photograph at the start
    and between the sweeps -> the frame list (np.uint8 [H, W, 3]), None when there are no persons.  The 3 n_frames rotated frames
    are one ``render.render_views`` call (the vertex normals computed once, not once per frame).  fn: the frames are written as an
    animated PNG (100 ms per frame, the reference's 10 fps) to ``splitext(fn)[0] + '.png'``; the reference's mp4 needs cv2.
    ``_color``: the persons' colours (``overlay_human_meshes``' argument), None: the palette by row."""
    from PIL import Image
    from . import render
    if len(humans) == 0:
        return None
    central, _color = overlay_human_meshes(humans, faces, K, model, img_pil_visu, unique_color=unique_color, alpha=alpha, _color=_color)
    central = central.astype(np.uint8)
    name = "verts_smplx" if "verts_smplx" in humans[0] else "v3d"
    center = humans[0][name].mean(0).detach().cpu().numpy()
    angles = [angle_range * i / (n_frames - 1) for i in range(n_frames)]
    Rt = np.concatenate([orbit_extrinsics(center, "y", angles), orbit_extrinsics(center, "y", [-a for a in angles]),
                         orbit_extrinsics(center, "x", angles)])
    verts = _stacked([h[name] for h in humans])
    W, H = img_pil_visu.size
    white = torch.full((1, H, W, 3), 255, dtype=torch.uint8, device=verts.device)
    Kc = torch.as_tensor(K)[0].detach().float().cpu().reshape(1, 3, 3)
    cols = [_color[j % len(_color)] for j in range(len(humans))]
    views = render.render_views(white, verts, torch.zeros(len(humans), dtype=torch.int32), Kc, faces, torch.from_numpy(Rt)[None],
                                colors=cols, alpha=alpha)[0].cpu().numpy()
    sweeps = [list(views[k * n_frames:(k + 1) * n_frames]) for k in range(3)]
    pause = [central for _ in range(n_frames // 4)]
    frames = list(pause)
    for sweep in sweeps:
        frames += sweep + sweep[::-1][1:-1] + pause
    if fn is not None:
        path = os.path.splitext(fn)[0] + ".png"
        imgs = [Image.fromarray(f) for f in frames]
        imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=100, loop=0)
        print(f"Saved video to {path}")
    return frames


CONTACT_TAU = 0.01   # contact.contacts' default tau: what --contacts 1 calls touching


def main(argv=None):
    """demo.py:231-386: every image of --img_folder -> forward -> overlay -> ``<out_folder>/<image>_<model>.png`` = [input | overlay],
    or [input | overlay | view] with --extra_views 1 (the persons turned 30 degrees about y, over white; a white panel where nobody
    was detected); --save_rotating_video 1 adds ``<image>_<model>_rotating.png`` (animated, when somebody was detected); --distance 1
    writes every person's distance from the camera on the overlay panel; --save_mesh 1 adds ``<image>_<model>.png.npy`` (float32
    [P, V, 3], the persons' vertices) and ``<image>_<model>.png.glb`` (``scene.create_scene``: the persons in the overlay's colours,
    the photograph and the camera); --save_masks 1 adds ``<image>_<model>_mask.png`` (per pixel the person's index + 1, 0 = background;
    8-bit up to 255 persons, 16-bit beyond) and ``<image>_<model>_parts.png`` (the body part + 1 of ``constants.SMPLX_BODY_PARTS``, 0 =
    background), both at the photograph's size (``maps.render_maps``), and prints each person's occlusion; --contacts 1 prints the image's touching
    pairs of persons (symmetric pair distance <= 0.01 m) and each person's penetration depth (``contact.contacts``) and writes nothing.  ``--batch_size N`` > 1 infers N images per forward (``pipeline.predict_images``) and draws each
    result as before.  ``--video 1`` treats the sorted folder as the consecutive frames of one clip (``pipeline.predict_video`` at
    ``--batch_size``, 32 when that is 1, and ``--fps``): the persons are tracked and smoothed across the frames and every mesh is
    coloured by ``track_id % len(PALETTE)``, so a person keeps their colour.  Returns every path written."""
    from argparse import ArgumentParser
    from PIL import Image
    from .preprocess import open_image
    parser = ArgumentParser()
    parser.add_argument("--model_name", type=str, default="multiHMR_896_L_synth")
    parser.add_argument("--img_folder", type=str, default="example_data")
    parser.add_argument("--out_folder", type=str, default="demo_out")
    parser.add_argument("--det_thresh", type=float, default=0.3)
    parser.add_argument("--nms_kernel_size", type=float, default=3)
    parser.add_argument("--fov", type=float, default=60)
    parser.add_argument("--alpha", type=float, default=1.0)
    parser.add_argument("--unique_color", type=int, default=0, choices=[0, 1])
    parser.add_argument("--extra_views", type=int, default=0, choices=[0, 1])
    parser.add_argument("--save_rotating_video", type=int, default=0, choices=[0, 1])
    parser.add_argument("--distance", type=int, default=0, choices=[0, 1])
    parser.add_argument("--save_mesh", type=int, default=0, choices=[0, 1])
    parser.add_argument("--save_masks", type=int, default=0, choices=[0, 1], help="1: instance mask and body-part PNGs, and each "
                        "person's occlusion on the terminal")
    parser.add_argument("--contacts", type=int, default=0, choices=[0, 1], help="1: each image's touching pairs of persons and every "
                        "person's penetration depth on the terminal (contact.contacts at its default margins)")
    parser.add_argument("--batch_size", type=int, default=1, help="> 1: decode, preprocess and infer that many images per forward "
                        "(pipeline.predict_images); the files written are the same")
    parser.add_argument("--video", type=int, default=0, choices=[0, 1], help="1: the sorted folder is one clip (pipeline.predict_video): "
                        "tracked, smoothed persons, one colour per track")
    parser.add_argument("--fps", type=float, default=30.0, help="frame rate of the clip (--video 1)")
    args = parser.parse_args(argv)
    assert torch.cuda.is_available()
    suffixes = (".jpg", ".jpeg", ".png", ".webp")
    if os.path.isfile(args.img_folder) and args.img_folder.lower().endswith(suffixes):
        l_img_path = [os.path.basename(args.img_folder)]
        args.img_folder = os.path.dirname(args.img_folder)
    else:
        root_dir = os.path.abspath(args.img_folder)
        l_img_path = sorted(os.path.relpath(os.path.join(r, f), root_dir) for r, _, fs in os.walk(root_dir) for f in fs
                            if f.lower().endswith(suffixes) and not f.startswith("."))
    model = load_model(args.model_name)
    faces = model.smpl_layer["neutral_10"].bm_x.faces
    model_name = os.path.basename(args.model_name)
    os.makedirs(args.out_folder, exist_ok=True)
    written = []

    def write(img_path, humans, K, img_pil_visu, colors=None):
        """Overlay (+ side view, + rotating video) of one image with its full-resolution camera K -> the files of that image.  ``colors``:
        one per person (the clip's track colours), None: the palette by row."""
        save_fn = os.path.join(args.out_folder, f"{img_path}_{model_name}.png")
        os.makedirs(os.path.dirname(save_fn), exist_ok=True)
        pred, _color = overlay_human_meshes(humans, faces, K, model, img_pil_visu, unique_color=args.unique_color, alpha=args.alpha,
                                            _color=colors)
        if args.distance:                                                # demo.py:348-350, with the camera of the photograph
            pred = print_distance_on_image(pred, humans, _color, K=K)
        l_img = [np.asarray(img_pil_visu), pred]
        if args.extra_views:                                             # demo.py:351-354: the side view, 30 degrees about y
            frames = create_rotating_video(humans, faces, K, model, img_pil_visu, unique_color=args.unique_color, alpha=args.alpha,
                                           fn=None, n_frames=2, angle_range=30, _color=colors)
            l_img.append(frames[1] if frames is not None else np.full_like(pred, 255))
        Image.fromarray(np.concatenate(l_img, 1).astype(np.uint8)).save(save_fn)
        print(f"{len(humans)} persons -> {save_fn}")
        written.append(save_fn)
        if args.save_rotating_video:                                     # demo.py:362-364, an animated PNG for the mp4
            fn = os.path.splitext(save_fn)[0] + "_rotating.mp4"
            if create_rotating_video(humans, faces, K, model, img_pil_visu, unique_color=args.unique_color, alpha=args.alpha, fn=fn,
                                     n_frames=20, angle_range=60, _color=colors) is not None:
                written.append(os.path.splitext(fn)[0] + ".png")
        if args.save_mesh:                                               # demo.py:370-384
            name = "verts_smplx" if humans and "verts_smplx" in humans[0] else "v3d"
            l_mesh = [h[name] for h in humans]
            V = int(model.smpl_layer["neutral_10"].bm_x.num_vertices)
            verts = _stacked(l_mesh).detach().float().cpu().numpy() if humans else np.zeros((0, V, 3), np.float32)
            np.save(save_fn + ".npy", verts)
            cols = [_color[j % len(_color)] for j in range(len(humans))]  # the overlay's colours, where the reference draws new ones
            scene = create_scene(img_pil_visu, l_mesh, [faces for _ in humans], color=cols, metallicFactor=0., roughnessFactor=0.5, K=K)
            scene.export(save_fn + ".glb")
            written.extend([save_fn + ".npy", save_fn + ".glb"])

        if args.save_masks:
            from .maps import render_maps
            name = "verts_smplx" if humans and "verts_smplx" in humans[0] else "v3d"
            V = int(model.smpl_layer["neutral_10"].bm_x.num_vertices)
            verts = _stacked([h[name] for h in humans]) if humans else torch.zeros(0, V, 3, device="cuda")
            size = (img_pil_visu.size[1], img_pil_visu.size[0])
            m = render_maps(verts, torch.zeros(len(humans), dtype=torch.int32), torch.as_tensor(K)[:1].detach().float(), faces, size,
                            face_labels=model.face_part_labels())
            stem = os.path.splitext(save_fn)[0]
            ids = (m.person[0] + 1).cpu().numpy()
            Image.fromarray(ids.astype(np.uint8 if len(humans) <= 255 else np.uint16)).save(stem + "_mask.png")
            Image.fromarray(((m.label[0].to(torch.int32) + 1) % 256).cpu().numpy().astype(np.uint8)).save(stem + "_parts.png")
            for j, (o, v, a) in enumerate(zip(m.occlusion.tolist(), m.visible_px.tolist(), m.amodal_px.tolist())):
                print(f"  person {j}: occlusion {o:.3f} ({v} of {a} px visible)")
            written.extend([stem + "_mask.png", stem + "_parts.png"])

        if args.contacts and humans:
            from .contact import contacts
            name = "verts_smplx" if "verts_smplx" in humans[0] else "v3d"
            c = contacts(_stacked([h[name] for h in humans]), [0] * len(humans), faces,
                         want=("penetration_depth", "inside_count", "contact_count", "pair_distance"))
            pd = torch.minimum(c.pair_distance, c.pair_distance.T).tolist()
            pairs = [(i, j) for i in range(len(humans)) for j in range(i + 1, len(humans)) if pd[i][j] <= CONTACT_TAU]
            print("  touching: " + (", ".join(f"{i}-{j} ({pd[i][j]:+.3f} m)" for i, j in pairs) if pairs else "nobody"))
            for j, (d, ni, nc) in enumerate(zip(c.penetration_depth.tolist(), c.inside_count.tolist(), c.contact_count.tolist())):
                print(f"  person {j}: penetration depth {d:.3f} m ({ni} vertices inside another person, {nc} in contact)")

    if args.video:                                                       # the folder is one clip: track, smooth, one colour per track
        from .pipeline import predict_video
        from .render import PALETTE
        from .track import Tracker
        opened = (Image.open(os.path.join(args.img_folder, p)) for p in l_img_path)
        for r in predict_video(model, opened, batch_size=args.batch_size if args.batch_size > 1 else 32, tracker=Tracker(model, fps=args.fps),
                               fov=args.fov, det_thresh=args.det_thresh, nms_kernel_size=args.nms_kernel_size):
            colors = [PALETTE[h["track_id"] % len(PALETTE)] for h in r.humans] or None
            write(l_img_path[r.index], r.humans, r.K_full, r.source.convert("RGB"), colors)
        return written
    if args.batch_size > 1:                                              # one forward per batch_size images, then the same drawing
        from .pipeline import predict_images
        opened = (Image.open(os.path.join(args.img_folder, p)) for p in l_img_path)      # decoded on the pipeline's threads
        for r in predict_images(model, opened, batch_size=args.batch_size, fov=args.fov, det_thresh=args.det_thresh,
                                nms_kernel_size=args.nms_kernel_size):
            write(l_img_path[r.index], r.humans, r.K_full, r.source.convert("RGB"))
        return written
    for img_path in l_img_path:
        x, img_pil_visu = open_image(os.path.join(args.img_folder, img_path), model.img_size)
        K = get_camera_parameters(model.img_size, fov=args.fov)
        humans = forward_model(model, x, K, det_thresh=args.det_thresh, nms_kernel_size=args.nms_kernel_size)
        ratio = max(img_pil_visu.size) / x.shape[-1]                     # demo.py:340-344: K for the full-resolution image
        K[0, 0, 2] = img_pil_visu.size[0] / 2.0
        K[0, 1, 2] = img_pil_visu.size[1] / 2.0
        K[0, [0, 1], [0, 1]] = ratio * K[0, [0, 1], [0, 1]]
        write(img_path, humans, K, img_pil_visu)
    return written


if __name__ == "__main__":
    main()
