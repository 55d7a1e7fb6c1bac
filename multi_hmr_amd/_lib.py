"""ctypes binding of ``libmhmr.so`` (C ABI declared in include/mhmr.h).

The HIP library is the product: there is NO CPU / PyTorch fallback.  If the shared object is missing or an
entry point fails, loading raises and every op raises -- loudly, by design.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libmhmr.so")
SOURCES = ["gemm.hip", "gemm256.hip", "attention.hip", "attention_f32.hip", "vit_misc.hip", "vit_cls.hip", "hph.hip", "lbs.hip", "preprocess.hip", "evalm.hip", "bodymodel.hip", "bodymodel_bwd.hip", "heads_bwd.hip", "hph_bwd.hip", "detect_bwd.hip", "feature_grad.hip", "vit_bwd.hip", "linear_bf16.hip", "attention_bf16.hip", "vit_embed_bwd.hip", "optim.hip", "encoder_pack.hip", "fit.hip", "track.hip", "anny.hip", "render.hip", "render_maps.hip", "raster_grad.hip", "silhouette.hip", "contact.hip", "scene.hip", "loss.hip", "capi.hip"]
HEADERS = ["mhmr_common.h", "mhmr_internal.h", "vit_plan.h", "ln_stats.h", "hph_shared.h", "body_shared.h", "row_sums.h", "adam_element.h", "render_shared.h", os.path.join("..", "..", "include", "mhmr.h")]

VERSION = 106                       # include/mhmr.h MHMR_VERSION (struct layouts and entry-point semantics)
DT_BF16, DT_F16 = 0, 1
ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
EPI_OP16, EPI_OP16_GELU, EPI_OP16_RELU, EPI_RESID, EPI_PATCH, EPI_F32, EPI_VT, EPI_OP16_QK = range(8)
ATTN_QSCALE = 0.18033688011112042   # include/mhmr.h MHMR_ATTN_QSCALE

#: include/mhmr.h MHMR_VIT_FORM_*: the bits of mhmr_vit_form_bits, in bit order
VIT_FORM_BITS = ("rowmap", "allrows256", "nmask", "fold", "lo8_ranges", "cst", "ao", "splitk", "qkv_merge", "fc1map", "x3")

#: include/mhmr.h MHMR_PLAN_*: the switches of mhmr_vit_plan_request, in bit order; PLAN_DEFAULT = an empty environment
PLAN_SWITCHES = ("rowmap", "gemm128", "lnfold", "lo8", "anyorder", "qkv_merge", "fc1_rowmap", "cls_stats", "tiny_allrows", "lnfold_allrows", "vits_256")
PLAN = {n: 1 << i for i, n in enumerate(PLAN_SWITCHES)}
PLAN_DEFAULT = 0x3f5

_vp, _fp, _ip, _i, _f = C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float  # all device pointers are void*
_f32p = C.POINTER(C.c_float)        # a typed float*: the nullable outputs appended to a descriptor (set with f32p(tensor); NULL by default)


def f32p(t):
    """``float*`` of a torch tensor's data for a ``_f32p`` descriptor field (None -> NULL)."""
    return C.cast(C.c_void_p(None if t is None else t.data_ptr()), _f32p)


class MhmrError(RuntimeError):
    pass


#: No SLP vectoriser in any translation unit (csrc/mhmr_common.h has the reasons and refuses a build without -DMHMR_NO_SLP): its
#: op_sel-swizzled v_pk_*_f32 code returned wrong values in two kernels on gfx950, and the scalar build is 2 % faster.
#: Hidden visibility: the dynamic symbols of the library are the declarations of include/mhmr.h (which carry default visibility), not its
#: internal launchers and template helpers.
COMMON_FLAGS = ["-fno-slp-vectorize", "-DMHMR_NO_SLP", "-fvisibility=hidden"]
#: per-translation-unit extra flags.  render.hip: every step rounded on its own (the render contract's fp64 geometry and fp32 blend
#: are restated operation by operation in numpy by the tests; an FMA would change the last bit).  render_maps.hip: the same geometry
#: (csrc/render_shared.h), which must agree with render.hip's bit for bit.  scene.hip: the same fp64 geometry.
#: raster_grad.hip: the same geometry again: its depth is the key's high word bit for bit, its barycentrics are the oracle's.
#: silhouette.hip: the projection of mhmr_render_point_visibility and the face setup of mhmr_render_amodal: the same pixels, the same bits.
#: loss.hip: every element of the training loss is the reference's fp32 subtraction(s), rounded one by one (its sign is the gradient).
#: optim.hip: the Adam update is torch's sequence of fp32 operations, each rounded on its own.
#: attention_bf16.hip: the logit S = fl(QSCALE * acc) is rounded before exp2(S - lse) in all three kernels, as the contract states it.
#: encoder_pack.hip: the LayerNorm fold is one fp32 multiply and the low half one fp32 subtraction, as vit.pack_block rounds them.
#: fit.hip: its update kernel runs optim.hip's Adam element (csrc/adam_element.h) and must round it the same way.
#: track.hip: the association cost and the One-Euro recursion are rounded operation by operation (the tests restate them in numpy).
#: contact.hip is NOT here: its distances and winding sums are compared with fp64 by tolerance and gain from fused multiply-adds; the
#: one expression whose zero is part of its contract (the face normal) is formed under `#pragma clang fp contract(off)` in the source.
EXTRA_FLAGS = {"render.hip": ["-ffp-contract=off"], "render_maps.hip": ["-ffp-contract=off"], "scene.hip": ["-ffp-contract=off"], "loss.hip": ["-ffp-contract=off"],
               "optim.hip": ["-ffp-contract=off"], "encoder_pack.hip": ["-ffp-contract=off"], "attention_bf16.hip": ["-ffp-contract=off"], "fit.hip": ["-ffp-contract=off"],
               "track.hip": ["-ffp-contract=off"], "raster_grad.hip": ["-ffp-contract=off"], "silhouette.hip": ["-ffp-contract=off"]}


def source_hash() -> str:
    """sha256 prefix over the contents of every source / header of the library and the compile flags: the identity of a BUILD RECIPE,
    the same on every machine and in every checkout path (unlike the .so's own hash, which embeds path-derived symbol ids).  It is
    compiled into the library (``mhmr_source_hash()``), so a shipped ``libmhmr.so`` says which sources it was made from."""
    import hashlib
    h = hashlib.sha256()
    for name in sorted(SOURCES) + sorted(HEADERS):
        with open(os.path.normpath(os.path.join(CSRC, name)), "rb") as f:
            h.update(os.path.basename(name).encode() + b"\0" + f.read() + b"\0")
    h.update(repr((COMMON_FLAGS, sorted(EXTRA_FLAGS.items()))).encode())
    return h.hexdigest()[:16]


def built_source_hash(path: str | None = None) -> str | None:
    """The source hash compiled into an existing libmhmr.so (None: no library, or one from before the hash existed).  Read from the
    file's bytes (capi.hip plants the marker string), NOT through dlopen: a library loaded here would be the one the process keeps
    even after build() has replaced the file."""
    import re
    path = path or LIB_PATH
    if not os.path.isfile(path):
        return None
    with open(path, "rb") as f:
        m = re.search(rb"MHMR_SOURCE_HASH=([0-9a-f]{16})", f.read())
    return m.group(1).decode() if m else None


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP translation unit for gfx950 (hipcc cross-compiles without a GPU; one object per source, in parallel) and link
    csrc/libmhmr.so.  An existing library is kept only if the source hash compiled into it equals the hash of the sources beside it
    (file times say nothing about a library that travelled from another machine)."""
    from concurrent.futures import ThreadPoolExecutor
    want = source_hash()
    if not force and built_source_hash() == want:
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(CSRC, "build")
    os.makedirs(objdir, exist_ok=True)
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f'-DMHMR_SOURCE_HASH="{want}"'] + COMMON_FLAGS

    def compile_one(name):
        obj = os.path.join(objdir, name.replace(".hip", ".o"))
        cmd = base + EXTRA_FLAGS.get(name, []) + ["-c", os.path.join(CSRC, name), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise MhmrError(f"hipcc failed on {name}:\n" + res.stdout + res.stderr)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, len(SOURCES))) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise MhmrError("hipcc link failed:\n" + res.stdout + res.stderr)
    return LIB_PATH


class VitBlock(C.Structure):
    _fields_ = ([(n, _vp) for n in ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "ln2_w", "ln2_b",
                                    "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ls2", "v_w2", "proj_w2")] +
                [("flags", _i), ("qkv_colsum", _vp), ("fc1_colsum", _vp), ("v_w8", _vp), ("proj_w8", _vp), ("v_w8_scale", _i), ("proj_w8_scale", _i)])


class VitDesc(C.Structure):
    _fields_ = ([(n, _i) for n in ("dtype", "B", "S", "C", "H", "L", "G", "N", "T", "Tp", "Kp")] +
                [("patch_w", _vp), ("patch_b", _vp), ("cls_pos0", _vp), ("pos", _vp), ("blocks", C.POINTER(VitBlock)),
                 ("norm_w", _vp), ("norm_b", _vp)] +
                [(n, _vp) for n in ("a_patch", "resid", "xn", "qk", "vt", "att", "hid", "attn_flags", "pstats", "rowstats")] +
                [("lo8", _i), ("x3", _i), ("qkv32", _vp), ("hid32", _vp), ("splitk", _vp), ("splitk_bytes", C.c_longlong), ("cpad", _i), ("v16", _vp), ("cls_pstats", _vp),
                 ("tap", _vp), ("tap_first", _i)])


class VitPlanRequest(C.Structure):
    _fields_ = [(n, _i) for n in ("C", "H", "N", "B", "fold", "x3", "lo8", "cpad")] + [("switches", C.c_uint), ("ncu", _i)]


class VitPlan(C.Structure):
    _fields_ = ([(n, _i) for n in ("Tp", "row_map", "tiny_batch", "pitch", "need_pstats", "need_cls_pstats", "need_v16")] + [("splitk_bytes", C.c_longlong)] +
                [(n, _i) for n in ("attn_flags", "fold_eligible", "lo8_eligible")] + [("form_bits", C.c_uint)])


class HphLayer(C.Structure):
    _fields_ = [(n, _vp) for n in ("ln_sa_w", "ln_sa_b", "to_qkv", "sa_out_w", "sa_out_b", "ln_ca_w", "ln_ca_b", "to_kv16",
                                   "to_q", "ca_out_w", "ca_out_b", "ln_ff_w", "ln_ff_b", "ff1_w", "ff1_b", "ff2_w", "ff2_b")]


class HphDesc(C.Structure):
    _fields_ = ([(n, _i) for n in ("dtype", "C", "G", "N", "Kc", "dim", "heads", "mlp", "depth", "nb", "Ktok", "Ndec", "patch",
                                   "nearness")] + [("fn", _f)] +
                [(n, _vp) for n in ("off1_w", "off1_b", "off2_w", "off2_b", "cq_x", "cq_y", "cv_x", "cv_y", "init_tail",
                                    "tok_w", "tok_b")] + [("layers", C.POINTER(HphLayer))] +
                [(n, _vp) for n in ("dec_w", "dec_b", "zc", "token", "x", "xn", "t1", "t2", "kv", "dec", "det_row", "nvalid")] +
                [("cam_dim", _i)])


class HphLayerGrads(C.Structure):
    """include/mhmr.h mhmr_hph_layer_grads: one fp32 gradient buffer per field of HphLayer (to_kv fp32 [2 inner, Kc])."""
    FIELDS = ("ln_sa_w", "ln_sa_b", "to_qkv", "sa_out_w", "sa_out_b", "ln_ca_w", "ln_ca_b", "to_kv", "to_q", "ca_out_w", "ca_out_b",
              "ln_ff_w", "ln_ff_b", "ff1_w", "ff1_b", "ff2_w", "ff2_b")
    _fields_ = [(n, _vp) for n in FIELDS]


class XattnBackwardDesc(C.Structure):
    """include/mhmr.h mhmr_xattn_backward_desc."""
    _fields_ = ([("layers", C.POINTER(HphLayer)), ("grads", C.POINTER(HphLayerGrads))] +
                [(n, _i) for n in ("depth", "dim", "heads", "mlp", "Kc", "N", "B", "dtype", "P", "ngroups", "nmax", "nchunks", "ctx_valid")] +
                [(n, _vp) for n in ("x0", "ctx16", "gstart", "chunks", "g_x_out", "g_x0", "det_row", "g_ctx", "workspace")] + [("workspace_bytes", C.c_longlong)] +
                [("g_feat", _f32p), ("ld_feat", _i), ("feat_cols", _i)])


class HphBackwardDesc(C.Structure):
    """include/mhmr.h mhmr_hph_backward_desc."""
    GRADS = ("g_off1_w", "g_off1_b", "g_off2_w", "g_off2_b", "g_tok_w", "g_tok_b", "g_dec_w", "g_dec_b", "g_cq_x", "g_cq_y", "g_cv_x", "g_cv_y")
    _fields_ = ([("fwd", C.POINTER(HphDesc))] + [(n, _vp) for n in ("ctx16", "det_y", "det_x", "gstart", "chunks")] +
                [(n, _i) for n in ("ngroups", "nmax", "nchunks", "P", "B")] + [("g_readout", _vp), ("ldg", _i), ("g_offset", _vp)] +
                [(n, _vp) for n in GRADS] + [("layer_grads", C.POINTER(HphLayerGrads)), ("g_zc", _vp), ("g_token", _vp), ("workspace", _vp),
                                             ("workspace_bytes", C.c_longlong), ("g_feat", _f32p), ("ld_feat", _i)])


class LbsConsts(C.Structure):
    _fields_ = ([(n, _i) for n in ("V", "Vp", "Vl", "Kb", "nb", "Kinf", "center_joint")] +
                [(n, _vp) for n in ("basis16", "vtemp", "J0", "JS", "parents", "skin_idx", "skin_w", "skin16", "xbary", "pose_tasks")] +
                [("pose_levels", _i)])


class RenderDesc(C.Structure):
    _fields_ = ([(n, _i) for n in ("B", "H", "W", "P", "V", "F")] + [("verts", _vp), ("vstride", C.c_longlong)] +
                [(n, _vp) for n in ("faces", "adj_off", "adj", "image_index", "K", "Rt", "colors")] +
                [(n, _f) for n in ("alpha", "intensity", "ambient", "metallic", "roughness", "znear", "zfar")] +
                [("smooth", _i), ("cull_back", _i), ("img_in", _vp), ("img_out", _vp), ("workspace", _vp),
                 ("workspace_bytes", C.c_longlong), ("key_out", _vp), ("rgb_out", _vp)])


class RenderMapsDesc(C.Structure):
    """include/mhmr.h mhmr_render_maps_desc."""
    _fields_ = ([(n, _i) for n in ("B", "NV", "H", "W", "P", "F")] + [("keys", _vp), ("image_index", _vp), ("face_label", _vp), ("L", _i)] +
                [(n, _vp) for n in ("person", "face", "depth", "label", "visible_px", "bbox", "zmin", "label_px")])


class PointVisibilityDesc(C.Structure):
    """include/mhmr.h mhmr_point_visibility_desc."""
    _fields_ = ([(n, _i) for n in ("B", "NV", "H", "W", "P", "N")] + [("points", _vp), ("pstride", C.c_longlong)] +
                [(n, _vp) for n in ("image_index", "K", "view_Rt", "keys")] + [("znear", _f), ("tau", _f), ("out", _vp)])


class RasterDesc(C.Structure):
    """include/mhmr.h mhmr_raster_desc."""
    _fields_ = ([(n, _i) for n in ("B", "NV", "H", "W", "P", "V", "F", "C")] + [("verts", _vp), ("vstride", C.c_longlong)] +
                [(n, _vp) for n in ("faces", "adj_off", "adj", "image_index", "K", "view_Rt", "keys", "attr")] + [("astride", C.c_longlong)] +
                [("znear", _f), ("cull_back", _i)] +
                [(n, _vp) for n in ("depth", "bary", "out_attr", "g_depth", "g_bary", "g_out_attr", "g_verts", "g_attr", "workspace")] +
                [("workspace_bytes", C.c_longlong)])


RASTER_MAX_CHANNELS = 16            # include/mhmr.h mhmr_raster_desc: C in [0, 16]


class DistanceTransformDesc(C.Structure):
    """include/mhmr.h mhmr_distance_transform_desc."""
    _fields_ = [(n, _i) for n in ("N", "H", "W")] + [("src", _vp), ("max_dist", _i), ("dist2", _vp), ("nearest", _vp), ("workspace", _vp),
                                                     ("workspace_bytes", C.c_longlong)]


class SilhouetteDesc(C.Structure):
    """include/mhmr.h mhmr_silhouette_desc."""
    _fields_ = ([(n, _i) for n in ("B", "H", "W", "P", "V", "F")] + [("verts", _vp), ("vstride", C.c_longlong)] +
                [(n, _vp) for n in ("faces", "image_index", "K", "Rt")] + [("znear", _f), ("zfar", _f), ("cull_back", _i), ("mask", _vp), ("allowed", _vp),
                                                                          ("sigma", _f), ("robust", _i), ("max_dist", _i)] +
                [(n, _vp) for n in ("terms", "counts", "g_verts", "splat", "moments", "workspace")] + [("workspace_bytes", C.c_longlong)])


DISTANCE_MAX_SIDE, DISTANCE_MAX_R = 4096, 46340   # include/mhmr.h mhmr_distance_transform_desc: H, W and max_dist at most these


class ContactDesc(C.Structure):
    """include/mhmr.h mhmr_contact_desc."""
    _fields_ = ([(n, _i) for n in ("P", "V", "F")] + [("verts", _vp), ("vstride", C.c_longlong), ("image_index", _vp), ("faces", _vp),
                 ("max_dist", _f), ("tau", _f), ("workspace", _vp), ("workspace_bytes", C.c_longlong)] +
                [(n, _vp) for n in ("sdf", "nearest_person", "nearest_face", "closest", "penetration_depth", "inside_count", "contact_count",
                                    "pair_distance", "pair_inside", "aabb", "valid")])


#: faces per LDS tile of csrc/contact.hip (its TILE): the face counts at which the kernel's tiling changes
CONTACT_FACE_TILE = 512


class SceneDesc(C.Structure):
    """include/mhmr.h mhmr_scene_desc."""
    _fields_ = ([(n, _i) for n in ("P", "V", "F")] + [("verts", _vp), ("vstride", C.c_longlong)] +
                [(n, _vp) for n in ("faces", "adj_off", "adj", "transform", "out", "bounds")])


class BodyConsts(C.Structure):
    """include/mhmr.h mhmr_body_consts."""
    _fields_ = ([(n, _i) for n in ("V", "Vp", "J", "nc", "K", "E", "L")] +
                [(n, _vp) for n in ("vtemp", "basis", "J0", "JS", "parents", "weights", "extra_idx", "lmk_idx", "lmk_bary")])


class BodyBwdConsts(C.Structure):
    """include/mhmr.h mhmr_body_bwd_consts."""
    _fields_ = [("n", _i), ("inv_ptr", _vp), ("inv_joint", _vp), ("inv_w", _vp)]


class BodyBackwardDesc(C.Structure):
    """include/mhmr.h mhmr_body_backward_desc."""
    _fields_ = ([("c", C.POINTER(BodyConsts)), ("bc", C.POINTER(BodyBwdConsts)), ("G", _i)] +
                [(n, _vp) for n in ("pose", "coef", "transl", "K", "ws_F", "ws_A", "vertices", "joints", "g_vertices", "g_joints", "g_v2d",
                                    "g_j2d", "g_pose", "g_coef", "g_transl", "workspace")] + [("workspace_bytes", C.c_longlong)])


class HeadsDecodeDesc(C.Structure):
    """include/mhmr.h mhmr_heads_decode_desc."""
    _fields_ = ([(n, _i) for n in ("P", "nb", "ldr", "patch", "nearness")] + [("fn", _f)] +
                [(n, _vp) for n in ("readout", "offset", "K", "det_b", "det_y", "det_x", "loc", "rotmat", "rotvec", "shape", "expression",
                                    "dist_postprocessed", "dist")])


class HeadsPlaceDesc(C.Structure):
    """include/mhmr.h mhmr_heads_place_desc."""
    _fields_ = ([(n, _i) for n in ("P", "V", "NJ", "center_joint")] +
                [(n, _vp) for n in ("verts_u", "joints_u", "transl", "K", "det_b", "g_v3d", "g_j3d", "g_v2d", "g_j2d", "g_transl", "gx_v", "gx_j",
                                    "g_transl_total", "workspace")] + [("workspace_bytes", C.c_longlong)])


class HeadsDecodeBackwardDesc(C.Structure):
    """include/mhmr.h mhmr_heads_decode_backward_desc."""
    _fields_ = ([(n, _i) for n in ("P", "nb", "ldr", "patch", "nearness")] + [("fn", C.c_double)] +
                [(n, _vp) for n in ("readout", "offset", "K", "det_b", "det_y", "det_x", "g_rotmat", "g_rotvec", "g_shape", "g_expression", "g_dist",
                                    "g_dist_postprocessed", "g_transl", "g_loc", "g_offset_direct", "g_readout", "g_offset")])


FIT_L2, FIT_GMOF = 0, 1              # include/mhmr.h MHMR_FIT_*
FIT_ROBUST = {"l2": FIT_L2, "gmof": FIT_GMOF}


class FitDesc(C.Structure):
    """include/mhmr.h mhmr_fit_desc."""
    _fields_ = ([("c", C.POINTER(BodyConsts)), ("bc", C.POINTER(BodyBwdConsts))] +
                [(n, _i) for n in ("P", "nb", "ldr", "patch", "nearness", "center_joint")] + [("fn", C.c_double)] +
                [(n, _vp) for n in ("readout", "offset", "readout0", "offset0", "det_b", "det_y", "det_x", "K", "keypoints", "confidence")] +
                [("sigma", _f), ("robust", _i)] +
                [(n, _f) for n in ("lambda_pose", "lambda_shape", "lambda_depth", "lambda_expr", "lambda_loc")] + [("mask", _vp)] +
                [("steps", _i), ("step0", _i)] + [(n, C.c_double) for n in ("lr", "beta1", "beta2", "eps")] +
                [(n, _vp) for n in ("exp_avg", "exp_avg_sq", "objective", "grad", "workspace")] + [("workspace_bytes", C.c_longlong)])


EVAL_STATUS = ("a person's keypoint box has no width or no height", "a keypoint is NaN or infinite",
               "an image column is not ascending or leaves [0, B)")    # include/mhmr.h MHMR_EVAL_*: bit b of mhmr_eval_match's status
EVAL_MAX_PERSONS, EVAL_MAX_IMAGES = 8192, 65535                        # include/mhmr.h MHMR_EVAL_MAX_*

TRACK_GROUPS = ("pose", "shape", "depth", "expr", "loc")    # include/mhmr.h MHMR_TRACK_*: bit g of mhmr_track_desc.groups
TRACK_MAX_CAPACITY = 1024           # include/mhmr.h MHMR_TRACK_MAX_CAPACITY


class TrackDesc(C.Structure):
    """include/mhmr.h mhmr_track_desc."""
    _fields_ = ([(n, _i) for n in ("F", "P", "nb", "capacity")] + [(n, _vp) for n in ("img_id", "idx_y", "idx_x", "transl", "readout", "offset")] +
                [("fps", _f), ("max_dist", _f), ("max_age", _i), ("groups", _i), ("dcutoff", _f)] +
                [("mincutoff_" + g, _f) for g in TRACK_GROUPS] + [("beta_" + g, _f) for g in TRACK_GROUPS] +
                [("state", _vp), ("state_bytes", C.c_longlong), ("workspace", _vp), ("workspace_bytes", C.c_longlong)] +
                [(n, _vp) for n in ("track_id", "hits", "readout_s", "offset_s", "status")])


class PreImage(C.Structure):
    """include/mhmr.h mhmr_pre_image: one image of mhmr_preprocess_u8_batch (device pointers + the geometry of its plan)."""
    _fields_ = ([("img", _vp)] + [(n, _i) for n in ("H", "W", "ow", "oh", "y0", "rows", "pad_x", "pad_y", "ksh", "ksv")] +
                [(n, _vp) for n in ("kh", "bh", "kv", "bv", "tmp")])


class PreImageO(C.Structure):
    """include/mhmr.h mhmr_pre_image_o: one image of mhmr_preprocess_u8_batch_oriented (PreImage's fields; H, W = the stored buffer, the
    rest = the oriented image; ``orient`` = ORIENT_* bits)."""
    _fields_ = PreImage._fields_ + [("orient", _i)]


ORIENT_MIRROR, ORIENT_ROT90 = 1, 2  # include/mhmr.h MHMR_ORIENT_*


class LossDesc(C.Structure):
    """include/mhmr.h mhmr_loss_desc."""
    TENSORS = ("scores", "offset", "rotmat", "shape", "dist", "transl", "pelvis", "j3d", "v3d", "j2d", "v2d")
    _fields_ = ([(n + "_hat", _vp) for n in TENSORS] + [(n, _vp) for n in TENSORS] +
                [(n, _i) for n in ("B", "G", "P", "V", "J", "nrot", "nb_hat", "nb_gt")] + [("img_size", _f), ("use_2d", _i),
                                                                                          ("alpha", C.c_double * 10)])


class LossGrads(C.Structure):
    """include/mhmr.h mhmr_loss_grads."""
    _fields_ = [(n, _vp) for n in LossDesc.TENSORS]


LOSS_OUT_BYTES = 128                # include/mhmr.h MHMR_LOSS_OUT_BYTES


class AdamSegment(C.Structure):
    """include/mhmr.h mhmr_adam_segment."""
    _fields_ = ([(n, _vp) for n in ("param", "exp_avg", "exp_avg_sq", "grad", "param2", "exp_avg2", "exp_avg_sq2", "grad2", "packed", "addend")] +
                [("n", C.c_longlong)] + [(n, _i) for n in ("cols", "pitch", "packed_kind", "chunk0")] +
                [(n, _f) for n in ("step_size", "bc2_sqrt", "step_size2", "bc2_sqrt2")])


class VitBlockBackwardDesc(C.Structure):
    """include/mhmr.h mhmr_vit_block_backward_desc: the fp32 master tensors of one block (torch layout), the block input, the cotangent
    of its output, and one gradient buffer per tensor."""
    PARAMS = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ls2")
    _fields_ = ([(n, _i) for n in ("B", "T", "Tp", "C", "H")] + [(n, _vp) for n in PARAMS] + [(n, _vp) for n in ("x_in", "g_out", "g_in")] +
                [("g_" + n, _vp) for n in PARAMS] + [("workspace", _vp), ("workspace_bytes", C.c_longlong), ("linear_precision", _i)])


class VitTailBackwardDesc(C.Structure):
    """include/mhmr.h mhmr_vit_tail_backward_desc: final norm + the last n blocks, at the tapped streams."""
    _fields_ = ([(n, _i) for n in ("B", "N", "T", "Tp", "C", "H", "n")] + [("norm_w", _vp), ("norm_b", _vp),
                ("blocks", C.POINTER(VitBlockBackwardDesc))] + [(n, _vp) for n in ("tap", "resid", "g_feat", "g_norm_w", "g_norm_b", "g_stream",
                                                                                   "workspace")] + [("workspace_bytes", C.c_longlong),
                                                                                                     ("linear_precision", _i)])


BWD_F32, BWD_BF16 = 0, 1            # include/mhmr.h MHMR_BWD_*: linear_precision of the two descriptors above
BWD_PRECISIONS = {"f32": BWD_F32, "bf16": BWD_BF16}


def bwd_precision(name) -> int:
    """MHMR_BWD_* of a precision name of the backbone backward ("f32" or "bf16"); ``ValueError`` for anything else."""
    if name not in BWD_PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(BWD_PRECISIONS)}, not {name!r}")
    return BWD_PRECISIONS[name]


ATTN_F32, ATTN_BF16 = 0, 1          # include/mhmr.h MHMR_ATTN_*: attention_precision of the ..._a / ..._pa entries
ATTN_PRECISIONS = {"f32": ATTN_F32, "bf16": ATTN_BF16}


def attn_precision(name) -> int:
    """MHMR_ATTN_* of an attention precision name of the backbone backward ("f32" or "bf16"); ``ValueError`` for anything else."""
    if name not in ATTN_PRECISIONS:
        raise ValueError(f"attention must be one of {sorted(ATTN_PRECISIONS)}, not {name!r}")
    return ATTN_PRECISIONS[name]


class VitEmbedBackwardDesc(C.Structure):
    """include/mhmr.h mhmr_vit_embed_backward_desc: the image, the cotangent of the stream entering block 0, the resampling matrix and one
    gradient buffer for each of patch_embed.proj.weight / .bias, cls_token and pos_embed."""
    _fields_ = ([(n, _i) for n in ("B", "S", "G", "M", "Tp", "C")] +
                [(n, _vp) for n in ("x", "g_stream", "interp", "g_patch_w", "g_patch_b", "g_cls", "g_pos", "workspace")] +
                [("workspace_bytes", C.c_longlong)])


ADAM_CHUNK = 2048                   # include/mhmr.h MHMR_ADAM_CHUNK
ADAM_PACK_NONE, ADAM_PACK_F32, ADAM_PACK_F16, ADAM_PACK_BF16 = range(4)


class PackJob(C.Structure):
    """include/mhmr.h mhmr_pack_job."""
    _fields_ = ([(n, _vp) for n in ("w", "ln_w", "ln_b", "bias", "w16", "lo", "bias_out", "colsum", "pos_embed", "cls_token", "tap_w", "tap_i",
                                    "pos", "cls_pos0")] +
                [(n, _i) for n in ("kind", "dtype", "row0", "N", "K", "pitch16", "lo_form", "lo_row0", "lo_rows", "lo_section", "lo_pitch",
                                   "M", "G", "C")])


PACK_ROW, PACK_POS = 0, 1           # include/mhmr.h MHMR_PACK_*
PACK_LO_NONE, PACK_LO_PAIR, PACK_LO_TRIPLE = range(3)


_SIGS = {
    "mhmr_version": ([], _i),
    "mhmr_source_hash": ([], C.c_char_p),
    "mhmr_vit_forward": ([C.POINTER(VitDesc), _vp, _vp, _vp, _i, _vp], _i),
    "mhmr_vit_form_bits": ([C.POINTER(VitDesc), _vp, C.POINTER(C.c_uint)], _i),
    "mhmr_vit_plan": ([C.POINTER(VitPlanRequest), C.POINTER(VitPlan)], _i),
    "mhmr_gemm16": ([_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "mhmr_gemm16_ex": ([_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp], _i),
    "mhmr_gemm16_ln": ([_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "mhmr_gemm16_lo8": ([_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "mhmr_gemm16_masked": ([_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "mhmr_qkv16": ([_vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp], _i),
    "mhmr_splitk_workspace_bytes": ([_i, _i, _i], C.c_longlong),
    "mhmr_gemm16_splitk_resid": ([_vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _f, _vp, C.c_longlong, _i, _vp], _i),
    "mhmr_ln_stats": ([_vp, _vp, _vp, _i, _i, _i, _i, _f, _vp], _i),
    "mhmr_cls_linear16": ([_vp, C.c_longlong, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, C.c_longlong, _i, _i, _vp, _i, _i, _i, _i, _i, _vp], _i),
    "mhmr_attention16": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "mhmr_attention16_ex": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _vp, _vp], _i),
    "mhmr_attention_flag_count": ([_i, _i, _i], _i),
    "mhmr_attention16_pitch": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _vp], _i),
    "mhmr_layernorm16_pitch": ([_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp], _i),
    "mhmr_attention_f32": ([_vp, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "mhmr_layernorm16_pair": ([_vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp], _i),
    "mhmr_gelu16_pair": ([_vp, _vp, C.c_longlong, _i, _i, _vp], _i),
    "mhmr_layernorm16": ([_vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp], _i),
    "mhmr_detect_scores": ([_vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "mhmr_detect_count": ([_vp, _i, _i, _i, _f, _vp, _vp], _i),
    "mhmr_detect_write": ([_vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "mhmr_detect_write_cap": ([_vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _i, _vp], _i),
    "mhmr_person_groups": ([_vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp], _i),
    "mhmr_camera_embed": ([_vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "mhmr_hph_forward": ([C.POINTER(HphDesc), _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _vp, _i, _vp, _i,
                          _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "mhmr_xattn_layers_forward": ([C.POINTER(HphLayer)] + [_i] * 8 + [_vp] * 7 + [_i, _i, _vp, _i, _i, _vp], _i),
    "mhmr_linear_f32": ([_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp], _i),
    "mhmr_layernorm_f32": ([_vp, _vp, _vp, _vp, _i, _i, _f, _vp], _i),
    "mhmr_hph_self_attn": ([_vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "mhmr_hph_cross_attn": ([_vp, _vp, _vp, _i, _vp, _i, _i, _vp], _i),
    "mhmr_hph_decode": ([_vp, _i, _i, _vp, _vp, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp], _i),
    "mhmr_linear_f32_backward_input": ([_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp], _i),
    "mhmr_linear_f32_backward_weight": ([_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp], _i),
    "mhmr_layernorm_f32_backward_workspace_bytes": ([_i, _i], C.c_longlong),
    "mhmr_layernorm_f32_backward": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, C.c_longlong, _vp], _i),
    "mhmr_hph_self_attn_backward": ([_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "mhmr_hph_cross_attn_backward": ([_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "mhmr_grad_ctx_gemm_workspace_bytes": ([_i, _i, _i], C.c_longlong),
    "mhmr_grad_ctx_gemm": ([_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, C.c_longlong, _vp], _i),
    "mhmr_xattn_layers_backward_workspace_bytes": ([_i] * 8, C.c_longlong),
    "mhmr_xattn_layers_backward": ([C.POINTER(XattnBackwardDesc), _vp], _i),
    "mhmr_hph_backward_workspace_bytes": ([C.POINTER(HphDesc), _i, _i], C.c_longlong),
    "mhmr_hph_backward": ([C.POINTER(HphBackwardDesc), _vp], _i),
    "mhmr_detect_backward_workspace_bytes": ([_i, _i], C.c_longlong),
    "mhmr_detect_backward": ([_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, C.c_longlong, _vp], _i),
    "mhmr_rows_times_weight": ([_vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _vp], _i),
    "mhmr_detect_feature_grad_workspace_bytes": ([_i], C.c_longlong),
    "mhmr_detect_feature_grad": ([_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, C.c_longlong, _vp], _i),
    "mhmr_features_to_context": ([_vp, _vp, _vp, _i, _i, _i, _i, _vp], _i),
    "mhmr_lbs_forward": ([C.POINTER(LbsConsts)] + [_vp] * 7 + [_i] + [_vp] * 8 + [_vp], _i),
    "mhmr_preprocess_u8": ([_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _i] + [_i] * 7 + [_vp, _vp, _vp, _vp], _i),
    "mhmr_preprocess_u8_batch": ([C.POINTER(PreImage), _vp, _i, _i, _vp, _vp, _vp], _i),
    "mhmr_preprocess_u8_batch_oriented": ([C.POINTER(PreImageO), _vp, _i, _i, _vp, _vp, _vp], _i),
    "mhmr_eval_mesh_errors": ([_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp], _i),
    "mhmr_eval_match_workspace_bytes": ([_i, _i, _i], C.c_longlong),
    "mhmr_eval_match": ([_vp, C.c_longlong, _vp, _i, _vp, _vp, _i, _i, _i, _f, _vp, C.c_longlong, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i),
    "mhmr_eval_mesh_errors_indexed": ([_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp], _i),
    "mhmr_body_forward": ([C.POINTER(BodyConsts), _vp, _vp, _vp, _vp, _i] + [_vp] * 6 + [_vp], _i),
    "mhmr_body_backward_workspace_bytes": ([C.POINTER(BodyConsts), _i], C.c_longlong),
    "mhmr_body_backward": ([C.POINTER(BodyBackwardDesc), _vp], _i),
    "mhmr_heads_decode": ([C.POINTER(HeadsDecodeDesc), _vp], _i),
    "mhmr_heads_place_workspace_bytes": ([_i, _i, _i], C.c_longlong),
    "mhmr_heads_place_backward": ([C.POINTER(HeadsPlaceDesc), _vp], _i),
    "mhmr_heads_decode_backward": ([C.POINTER(HeadsDecodeBackwardDesc), _vp], _i),
    "mhmr_sparse_regress": ([_ip, _ip, _fp, _i, _i, _fp, _fp, _i, _fp, _vp], _i),
    "mhmr_gt_targets": ([_fp, _i, _i, _fp, _ip, _i, _i, _i, _i, _f, _i] + [_vp] * 7 + [_vp], _i),
    "mhmr_project_points": ([_fp, _fp, _i, _i, _fp, _vp], _i),
    "mhmr_rotvec_to_rotmat": ([_fp, _i, _fp, _vp], _i),
    "mhmr_anny_scores": ([_vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp], _i),
    "mhmr_anny_camera": ([_vp, _i, _i, _f, _vp, _vp, _vp], _i),
    "mhmr_anny_decode": ([_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i] + [_vp] * 6 + [_vp], _i),
    "mhmr_render_workspace_bytes": ([C.POINTER(RenderDesc)], C.c_longlong),
    "mhmr_render_meshes": ([C.POINTER(RenderDesc), _vp], _i),
    "mhmr_render_views_workspace_bytes": ([C.POINTER(RenderDesc), _i], C.c_longlong),
    "mhmr_render_views": ([C.POINTER(RenderDesc), _i, _vp, _vp], _i),
    "mhmr_render_maps": ([C.POINTER(RenderMapsDesc), _vp], _i),
    "mhmr_render_point_visibility": ([C.POINTER(PointVisibilityDesc), _vp], _i),
    "mhmr_render_amodal_workspace_bytes": ([C.POINTER(RenderDesc), _i, _i], C.c_longlong),
    "mhmr_render_amodal": ([C.POINTER(RenderDesc), _i, _vp, _vp, _vp], _i),
    "mhmr_raster_workspace_bytes": ([C.POINTER(RasterDesc), _i], C.c_longlong),
    "mhmr_raster_interpolate": ([C.POINTER(RasterDesc), _vp], _i),
    "mhmr_raster_backward": ([C.POINTER(RasterDesc), _vp], _i),
    "mhmr_distance_transform_workspace_bytes": ([C.POINTER(DistanceTransformDesc)], C.c_longlong),
    "mhmr_distance_transform": ([C.POINTER(DistanceTransformDesc), _vp], _i),
    "mhmr_silhouette_workspace_bytes": ([C.POINTER(SilhouetteDesc), _i], C.c_longlong),
    "mhmr_silhouette": ([C.POINTER(SilhouetteDesc), _vp], _i),
    "mhmr_contact_workspace_bytes": ([_i, _i], C.c_longlong),
    "mhmr_contact_check_faces": ([_vp, _i, _i], _i),
    "mhmr_contact": ([C.POINTER(ContactDesc), _vp], _i),
    "mhmr_scene_pack": ([C.POINTER(SceneDesc), _vp], _i),
    "mhmr_loss_workspace_bytes": ([], C.c_longlong),
    "mhmr_loss_forward": ([C.POINTER(LossDesc), _vp, C.c_longlong, _vp, _vp], _i),
    "mhmr_loss_backward": ([C.POINTER(LossDesc), _vp, _fp, C.POINTER(LossGrads), _vp], _i),
    "mhmr_adam_step": ([C.POINTER(AdamSegment), _vp, _i, C.c_double, C.c_double, C.c_double, C.c_double, _vp, C.c_longlong, _vp, _vp], _i),
    "mhmr_vit_repack": ([C.POINTER(PackJob), _vp, _i, _vp], _i),
    "mhmr_fit_keypoints_workspace_bytes": ([C.POINTER(BodyConsts), _i], C.c_longlong),
    "mhmr_fit_keypoints": ([C.POINTER(FitDesc), _vp], _i),
    "mhmr_track_state_bytes": ([_i, _i], C.c_longlong),
    "mhmr_track_workspace_bytes": ([_i, _i], C.c_longlong),
    "mhmr_track_update": ([C.POINTER(TrackDesc), _vp], _i),
    "mhmr_attention_f32_tape": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp], _i),
    "mhmr_attention_f32_backward_workspace_bytes": ([_i, _i, _i], C.c_longlong),
    "mhmr_attention_f32_backward": ([_vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, C.c_longlong, _vp], _i),
    "mhmr_vit_block_backward_workspace_bytes": ([_i, _i, _i], C.c_longlong),
    "mhmr_vit_block_backward_workspace_bytes_p": ([_i, _i, _i, _i], C.c_longlong),
    "mhmr_vit_block_backward": ([C.POINTER(VitBlockBackwardDesc), _vp], _i),
    "mhmr_vit_tail_backward_workspace_bytes": ([_i, _i, _i], C.c_longlong),
    "mhmr_vit_tail_backward_workspace_bytes_p": ([_i, _i, _i, _i], C.c_longlong),
    "mhmr_vit_tail_backward": ([C.POINTER(VitTailBackwardDesc), _vp], _i),
    "mhmr_linear_bf16_workspace_bytes": ([_i, _i, _i], C.c_longlong),
    "mhmr_linear_bf16": ([_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, C.c_longlong, _vp], _i),
    "mhmr_linear_bf16_backward_input": ([_vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, C.c_longlong, _vp], _i),
    "mhmr_linear_bf16_backward_weight": ([_vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, C.c_longlong, _vp], _i),
    "mhmr_attention_bf16_workspace_bytes": ([_i, _i, _i, _i], C.c_longlong),
    "mhmr_attention_bf16_tape": ([_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, C.c_longlong, _vp], _i),
    "mhmr_attention_bf16_backward": ([_vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, C.c_longlong, _vp], _i),
    "mhmr_vit_block_backward_workspace_bytes_pa": ([_i, _i, _i, _i, _i], C.c_longlong),
    "mhmr_vit_tail_backward_workspace_bytes_pa": ([_i, _i, _i, _i, _i], C.c_longlong),
    "mhmr_vit_block_backward_a": ([C.POINTER(VitBlockBackwardDesc), _i, _vp], _i),
    "mhmr_vit_tail_backward_a": ([C.POINTER(VitTailBackwardDesc), _i, _vp], _i),
    "mhmr_vit_embed_backward_workspace_bytes": ([_i, _i, _i, _i], C.c_longlong),
    "mhmr_vit_embed_backward": ([C.POINTER(VitEmbedBackwardDesc), _vp], _i),
    "mhmr_prof_enable": ([_i], _i),
    "mhmr_prof_collect": ([C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)], _i),
}

#: every symbol include/mhmr.h declares
EXPORTS = tuple(_SIGS.keys())

_lib = None


def lib() -> C.CDLL:
    """Load (once) the in-tree libmhmr.so; raise if it is absent -- there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise MhmrError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950). The Multi-HMR path has no CPU fallback.")
        l = C.CDLL(LIB_PATH)
        for name, (args, res) in _SIGS.items():
            fn = getattr(l, name)          # AttributeError if the symbol is not exported
            fn.argtypes, fn.restype = args, res
        if l.mhmr_version() != VERSION:
            raise MhmrError(f"{LIB_PATH} is version {l.mhmr_version()}, this package binds version {VERSION} (include/mhmr.h): rebuild")
        _lib = l
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        kind = {-1: "bad argument", -2: "bad shape"}.get(rc, f"hipError_t {rc}")
        raise MhmrError(f"{what} failed: {kind}")


def workspace_bytes(name: str, *args) -> int:
    """The byte count a ``mhmr_*_workspace_bytes`` entry answers for these arguments; its negative answers are error codes and raise."""
    n = int(getattr(lib(), name)(*args))
    if n < 0:
        check(n, name)
    return n


def ptr(t) -> int | None:
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()
