"""Host-side mirror of the reference's `modules` package for the hot path only:
same import names as train.py:11-15 (`from modules.sampling import Sampling`, ...)."""
from .sampling import Sampling
from .loss import ChamferDistanceLoss, EarthMoverDistanceLoss, SilhouetteLoss, VPDiverseLoss, MeshRegularizationLoss, PointMeshDistanceLoss, OccupancyLoss
from .render import VertexRenderer, PhongRenderer
from .transform import (transform_points, rotate_points, translate_points, view_to_obj_points,
                        obj_to_view_points, rotate_points_forward_x_axis)
from .network import (pack_head_outputs, split_primitives, batch_norm_act, batch_norm_relu_pool, batch_norm_act_mean, conv3x3, conv2d, conv2d_bias_act, fold_batch_norm, GCNModel, GCNConv, FcHeads, ResNet18, VPNetOneRes, VPNetTwoRes,
                      SDNet)
from .meshing import Meshing, TriangleMesh, load_obj, merge_meshes
from .dataset import (parse_split_csv, parse_rendering_metadata, split_rgba, prepare_images, resized_size, MeshBatch,
                      sample_gt_points, gt_points, gt_normals, view_center_xforms, genre_xforms)
from . import augmentation
from .augmentation import (cut_mix_data, cut_mix_batch_points, adjust_point_num, mixup_points, point_mixup_data,
                           points_to_meshes_and_colors, points_to_mesh_batch, meshes_to_imgs, generate_point_mixup_data,
                           acd, augment, acd_mix_meshes, acd_mix_data)
from . import evaluation
from .evaluation import EvaluationMeter, SurfaceEvaluationMeter, VolumeEvaluationMeter
from . import visualize
from .visualize import Visualizer
from . import optim
from .optim import Adam
