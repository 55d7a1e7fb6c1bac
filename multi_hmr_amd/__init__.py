"""MI355X-native Multi-HMR batched inference (drop-in for naver/multi-hmr ``model.Model`` / ``demo.forward_model``)."""
from .model import Model  # noqa: F401
from .demo import create_rotating_video, forward_model, get_camera_parameters, load_model, open_image, overlay_human_meshes  # noqa: F401
from .render import render_batch, render_meshes, render_views  # noqa: F401
from .maps import RenderMaps, part_labels, render_maps  # noqa: F401
from .contact import Contacts, contacts, penetration_loss  # noqa: F401
from .scene import create_scene, export_batch, get_bbox, pack_meshes, print_distance_on_image, read_glb  # noqa: F401

from .preprocess import Preprocessor  # noqa: F401
from .graphed import GraphedForward  # noqa: F401
from .pipeline import ImageResult, PipelineError, predict_images, predict_video  # noqa: F401
from .bodymodel import BodyModel, load_body_data  # noqa: F401
from .evaluate import Evaluator, SparseRegressor, evaluate_dataset, load_h36m_regressor, load_smplx2smpl  # noqa: F401
from .groundtruth import GroundTruth  # noqa: F401
from .loss import Loss, loss_and_grads  # noqa: F401
from . import heads  # noqa: F401
from . import fit  # noqa: F401
from .fit import COCO17, OPENPOSE_BODY25, FitResult, KeypointFitter, keypoints_by_name  # noqa: F401
from . import track  # noqa: F401
from .track import TrackResult, Tracker  # noqa: F401
from . import raster  # noqa: F401
from .raster import Raster, depth_loss, rasterize  # noqa: F401
from . import silhouette  # noqa: F401
from .silhouette import Silhouette, assign_instance_masks, distance_transform, silhouette_loss  # noqa: F401
from .optim import HeadsAdam, ModelAdam, encoder_segments  # noqa: F401
from .train import Trainer  # noqa: F401
from .data import BEDLAM, EHF, THREEDPW, AnnotatedImages, TrainLoader  # noqa: F401  (data.collate stays there: .collate is a module)

__all__ = ["BodyModel", "COCO17", "OPENPOSE_BODY25", "FitResult", "KeypointFitter", "fit", "keypoints_by_name", "Evaluator", "GroundTruth", "HeadsAdam", "ModelAdam", "encoder_segments", "Loss", "Model", "Trainer", "GraphedForward", "SparseRegressor", "evaluate_dataset", "load_body_data",
           "load_h36m_regressor", "load_smplx2smpl", "loss_and_grads", "ImageResult", "PipelineError", "Preprocessor", "create_rotating_video", "create_scene", "export_batch", "forward_model", "get_bbox",
           "get_camera_parameters", "heads", "load_model", "open_image", "overlay_human_meshes", "pack_meshes", "predict_images", "predict_video", "print_distance_on_image",
           "read_glb", "render_batch", "render_meshes", "render_views", "RenderMaps", "part_labels", "render_maps", "Contacts", "contacts", "penetration_loss", "Raster", "depth_loss", "rasterize",
           "Silhouette", "assign_instance_masks", "distance_transform", "silhouette", "silhouette_loss",
           "TrackResult", "Tracker", "track", "AnnotatedImages", "BEDLAM", "EHF", "THREEDPW", "TrainLoader"]
