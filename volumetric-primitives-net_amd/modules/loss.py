"""modules/loss of the reference (chamfer_distance.py, vp_diverse.py, silhouette.py, emd/emd_module.py)
on the HIP Chamfer, raster and auction kernels.  Same class names and forward signatures."""
import torch
import torch.nn as nn

from .. import config
from ..ops import ChamferFunction, EmdFunction, RasterTotalFunction, const_tensor, mesh_regularizers, point_mesh_distance, primitive_occupancy_loss
from ..primitives import PrimitivePack
from .render import VertexRenderer


class ChamferDistanceLoss(nn.Module):
    def __init__(self):
        super().__init__()

    def forward(self, points1: torch.Tensor, points2: torch.Tensor, each_batch=False,
                w1=config.CD_W1, w2=config.CD_W2) -> torch.Tensor:
        """chamfer_distance.py:10-30: w1*mean_i min_j|a_i-b_j| + w2*mean_j min_i|a_i-b_j|
        (non-squared), per sample if each_batch else the batch mean."""
        self.check_parameters(points1)
        self.check_parameters(points2)
        loss = ChamferFunction.apply(points1, points2, w1, w2)
        return loss if each_batch else loss.mean()

    @staticmethod
    def check_parameters(points: torch.Tensor):
        assert points.ndimension() == 3  # (B, N, 3)        chamfer_distance.py:32-35
        assert points.size(-1) == 3


class EarthMoverDistanceLoss(nn.Module):
    def __init__(self):
        super().__init__()

    def forward(self, input1: torch.Tensor, input2: torch.Tensor, eps, iters):
        """emd_module.py:77-78: (dist [B,n], assignment [B,n] int32); train.py:193 calls it with
        eps=0.005, iters=50 on point sets normalised to the unit cube."""
        return EmdFunction.apply(input1, input2, eps, iters)


class VPDiverseLoss(nn.Module):
    def __init__(self, vp_num=None):
        super().__init__()
        self.cd_loss_func = ChamferDistanceLoss()
        self.vp_num = vp_num             # the reference asserts len == config.VP_NUM (vp_diverse.py:23)

    def forward(self, translates: list, gt_points: torch.Tensor) -> torch.Tensor:
        """vp_diverse.py:12-18."""
        self.check_parameters(translates)
        vp_center_points = torch.cat([t[:, None, :] for t in translates], 1)
        return self.cd_loss_func(vp_center_points, gt_points, w1=0.5, w2=1.0)

    def check_parameters(self, translates):
        assert isinstance(translates, list)
        if self.vp_num is not None:
            assert len(translates) == self.vp_num


class SilhouetteLoss(nn.Module):
    def __init__(self, loss_func=config.SILHOUETTE_LOSS_FUNC):
        super().__init__()
        self.loss_func = nn.L1Loss() if loss_func == 'L1' else nn.MSELoss()     # silhouette.py:11
        self.is_mse = loss_func != 'L1'

    def forward(self, predict_meshes, gt_silhouettes: torch.Tensor,
                dists: torch.Tensor, elevs: torch.Tensor, azims: torch.Tensor) -> torch.Tensor:
        """silhouette.py:13-23.  `predict_meshes` is the reference's list of B composed meshes (train.py:146-149,
        made by Meshing: each carries its primitives), a list of per-sample packs, or one PrimitivePack for the
        batch; the B sequential
        renders of silhouette.py:16-18 become one launch at the GT silhouette's resolution."""
        H, W = gt_silhouettes.shape[-2:]
        try:
            predict_meshes = PrimitivePack.of(predict_meshes)
        except TypeError:
            # meshes without (valid) primitives, e.g. train_sphere.py:119-128 (a sphere mesh deformed in place): their
            # triangles are rendered, silhouette.py:16-22 as written (B renders -> cat -> L1Loss / MSELoss)
            alpha, _ = VertexRenderer.triangle_alpha(predict_meshes, dists, elevs, azims, H, W)
            return self.loss_func(alpha[:, None], gt_silhouettes.to(alpha.device).float().reshape(alpha.shape[0], 1, H, W))
        B = len(predict_meshes)
        dev = predict_meshes.params.device
        cam = torch.stack([dists.to(dev).float().reshape(-1).expand(B), elevs.to(dev).float().reshape(-1).expand(B),
                           azims.to(dev).float().reshape(-1).expand(B)], 1)
        # render + loss + gradient partials in one pass (silhouette.py:16-22 renders B times, concatenates and applies
        # L1Loss/MSELoss); with w_sil = 1, w_dep = 0 the differentiable total IS the silhouette loss
        losses = RasterTotalFunction.apply(predict_meshes.params, predict_meshes.kinds, cam, gt_silhouettes, None, H, W,
                                           VertexRenderer.sigma, VertexRenderer.gamma, VertexRenderer.z_far, self.is_mse,
                                           1.0, 0.0)
        return losses[2]


class MeshRegularizationLoss(nn.Module):
    """The surface priors a mesh-deformation stage trains with next to its point-set losses (Pixel2Mesh, Wang et al., ECCV
    2018, section 3.4; not part of the reference, whose train_gcn.py:131-134 has Chamfer and EMD alone):
    w_edge * edge + w_lap * lap + w_normal * normal of ops.mesh_regularizers over one face topology for the batch.  A
    weight of exactly 0 drops its term from the launch.  `.last` keeps the three parts of the latest call, detached and on
    the device (reading them is the caller's synchronisation, not this module's).  To regularise towards the primitives'
    shape rather than towards flatness pass the offsets, forward(predict_vertices - vertices, faces): the Laplacian is
    linear."""

    def __init__(self, w_edge=1.0, w_lap=1.0, w_normal=1.0, edge_target=0.0):
        super().__init__()
        self.weights = (float(w_edge), float(w_lap), float(w_normal))
        self.edge_target = float(edge_target)
        self.terms = tuple(t for t, w in zip(('edge', 'lap', 'normal'), self.weights) if w != 0.0)
        self.last = None

    def forward(self, vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
        parts = mesh_regularizers(vertices, faces, self.edge_target, self.terms)
        self.last = parts.detach()
        return (parts * const_tensor(self.weights, torch.float32, parts.device)).sum()


class PointMeshDistanceLoss(nn.Module):
    """The data term that sees the triangles (the point_mesh_face_distance of PyTorch3D; not part of the reference, whose
    train_gcn.py:131-134 compares the predicted VERTICES with the ground-truth points): w_point * (mean squared distance
    from every point to its nearest triangle) + w_face * (mean squared distance from every triangle to its nearest point)
    of ops.point_mesh_distance over one face topology for the batch.  Both parts come out of one scan, so a weight of 0
    only drops its part from the sum and from the gradient.  `.last` keeps the two parts of the latest call, detached and
    on the device (reading them is the caller's synchronisation, not this module's)."""

    def __init__(self, w_point=1.0, w_face=1.0):
        super().__init__()
        self.weights = (float(w_point), float(w_face))
        self.last = None

    def forward(self, points: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
        parts = point_mesh_distance(points, vertices, faces)
        self.last = parts.detach()
        return (parts * const_tensor(self.weights, torch.float32, parts.device)).sum()


class OccupancyLoss(nn.Module):
    """The volumetric term the point and pixel losses lack (the coverage / consistency pair of Tulsiani et al., the occupancy
    loss of Paschalidou et al., CvxNet and BSP-Net; not part of the reference): w_occ * (cross-entropy of the soft union of
    the primitives against occupancy labels at query points) + w_overlap * (mean of relu(sum_k sigmoid(z_k) - 1)^2, a point
    claimed by more than one primitive) of ops.primitive_occupancy_loss, at temperature tau.  Both parts come out of one
    scan, so a weight of 0 only drops its part from the sum and from the gradient.  `.last` keeps the two parts of the
    latest call and `.last_skipped` the number of queries left out (int32 [1]), detached and on the device (reading them is
    the caller's synchronisation, not this module's)."""

    def __init__(self, w_occ=1.0, w_overlap=0.0, tau=0.05):
        super().__init__()
        self.weights = (float(w_occ), float(w_overlap))
        self.tau = float(tau)
        self.last = None
        self.last_skipped = None

    def forward(self, params: torch.Tensor, kinds, queries: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        parts, skipped = primitive_occupancy_loss(params, kinds, queries, labels, self.tau, return_skipped=True)
        self.last, self.last_skipped = parts.detach(), skipped
        return (parts * const_tensor(self.weights, torch.float32, parts.device)).sum()
