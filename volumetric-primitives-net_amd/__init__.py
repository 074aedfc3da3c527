"""vpn_amd — MI355X-native volumetric-primitive hot path (sampler, Chamfer, soft raster).

Import as `vpn_amd` (repo-root alias module); the directory name is fixed by the project
layout.  Everything here runs on hand-written HIP kernels in libvpn_hip.so through the C
ABI of include/vpn_hip.h; there is no CPU fallback."""
from . import config
from .ops import (SPHERE, CUBOID, SampleFunction, TransformFunction, ChamferFunction, EmdFunction, HeadPackFunction, FcStackFunction, BatchNormActFunction, BatchNormPoolFunction, BatchNormMeanFunction, MeshFunction,
                  CameraTransformFunction, RasterFunction,
                  RasterLossFunction, RasterTotalFunction, HotPathLossFunction, TrainStepLossFunction, chamfer_nn, kinds_tensor,
                  emd_recovered_samples, emd_last_group, eval_step, surfeval_step, face_normals_at, ragged_face_normals,
                  primitive_occupancy, winding_number, ragged_winding_number, mesh_occupancy, grid_queries, voliou_state, voliou_step,
                  primitive_field, lattice, isosurface, IsoSurface, PaddedMeshArrays, mesh_signed_distance, vis_primitives, vis_mesh, phong_mesh,
                  cluster_points, support_hulls, hull_meshes, hull_augment, union_surface, acd_mix_points,
                  GcnFactoredInputFunction, gcn_factored_input,
                  GcnAggregate2Function, gcn_aggregate2, GcnProjectFunction, gcn_project, gcn_blocks,
                  MeshRegFunction, mesh_regularizers, mesh_topology,
                  PointMeshFunction, point_mesh_distance, point_mesh_nearest, mesh_incidence,
                  OccupancyLossFunction, primitive_occupancy_loss, primitive_soft_occupancy, occloss_plan)
from .primitives import PrimitivePack, pack_primitives, kinds_from_counts
from .modules import (Sampling, ChamferDistanceLoss, EarthMoverDistanceLoss, SilhouetteLoss, VPDiverseLoss, MeshRegularizationLoss, PointMeshDistanceLoss, OccupancyLoss, VertexRenderer, PhongRenderer,
                      transform_points, rotate_points, translate_points, view_to_obj_points,
                      obj_to_view_points, rotate_points_forward_x_axis, pack_head_outputs, split_primitives, Meshing, TriangleMesh, load_obj, merge_meshes,
                      cut_mix_data, cut_mix_batch_points, adjust_point_num, mixup_points, point_mixup_data,
                      points_to_meshes_and_colors, points_to_mesh_batch, meshes_to_imgs, generate_point_mixup_data, acd, augment,
                      acd_mix_meshes, acd_mix_data, EvaluationMeter, SurfaceEvaluationMeter, VolumeEvaluationMeter, prepare_images,
                      MeshBatch, sample_gt_points, gt_points, gt_normals, view_center_xforms, genre_xforms,
                      Visualizer, FcHeads, batch_norm_act, batch_norm_relu_pool, batch_norm_act_mean, conv3x3, conv2d, conv2d_bias_act, fold_batch_norm, ResNet18, VPNetOneRes, VPNetTwoRes, SDNet, Adam)
from . import modules
