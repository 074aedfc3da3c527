"""GCNModel of the reference (modules/network/gcn.py): the VPN + GCN refinement stage of train_gcn.py / test_gcn.py.

torch_geometric and kaolin are absent, so their two pieces are restated here: GCNConv (PyG's default: self loops,
symmetric normalisation, bias) and the unique mesh edges of `compute_adjacency_info`.  The dense GEMMs (x Theta and the
fc stack) stay torch.matmul / nn.Linear; everything around them runs on the HIP kernels of csrc/gcn.hip:
graph aggregation (+ bias, + ReLU), image bounds, positional encoding, perceptual feature pooling and their backward.

Degenerate clouds (zmax == zmin or ymax == ymin within a sample) divide by zero in the reference's grid; they do here
as well and are not supported."""
import math

import torch
import torch.nn as nn

from ..ops import (GcnAggregateFunction, GcnFactoredInputFunction, GcnInputFunction, gcn_aggregate2, gcn_blocks, gcn_bounds,
                   gcn_edges, gcn_edge_index, gcn_graph, gcn_project)


class GCNConv(nn.Module):
    """PyG's GCNConv(in_channels, out_channels) with its defaults (add_self_loops, normalize, bias, no cached edge
    weights): forward(x [B,N,in], graph) = A_hat (x Theta) + b, A_hat = D^-1/2 (A + I) D^-1/2 (ops.gcn_normalized_adjacency).
    Glorot-uniform Theta, zero bias, as PyG initialises them.

    Parameters: `weight` (in, out) and `bias` (out,), the PyG 1.x layout, which state_dict() saves.  load_state_dict also
    takes the PyG >= 2 layout, `lin.weight` (out, in) + `bias`, and transposes it."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.in_channels + self.out_channels))          # torch_geometric.nn.inits.glorot
        with torch.no_grad():
            self.weight.uniform_(-a, a)
            self.bias.zero_()

    def forward(self, x, graph, relu=False):
        """x [B,N,in] -> [B,N,out]; relu=True applies the ReLU that follows the layer in GCNModel (fused)."""
        return GcnAggregateFunction.apply(torch.matmul(x, self.weight), self.bias, graph.row_ptr, graph.col, graph.w, relu)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        lin = prefix + 'lin.weight'
        if lin in state_dict and prefix + 'weight' not in state_dict:
            state_dict[prefix + 'weight'] = state_dict.pop(lin).t().contiguous()
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    def extra_repr(self):
        return '%d, %d' % (self.in_channels, self.out_channels)


def to_pyg2_state_dict(state_dict):
    """A GCNModel / GCNConv state dict in the PyG >= 2 layout (`convK.lin.weight` (out, in)); the inverse of what
    load_state_dict does with such a dict."""
    out = {}
    for k, v in state_dict.items():
        if k.endswith('.weight') and k.split('.')[-2].startswith('conv') and v.dim() == 2:
            out[k[:-len('weight')] + 'lin.weight'] = v.t().contiguous()
        else:
            out[k] = v
    return out


class GCNModel(nn.Module):
    """gcn.py:7-58: same constructor, forward, layers (conv1..conv6, fc) and output
    predict_vertices [B,N,3] = vertices + 0.1 * fc(conv stack).  The graph of meshes[0]'s faces is built once per face
    topology (ops.gcn_graph) and the image bounds are computed on the device: a step makes no host synchronisation.

    factored_input=True computes conv1's product in factored form (ops.GcnFactoredInputFunction): the
    maps and the global features are projected by conv1.weight's row blocks and every vertex gathers from the projected
    maps, so conv1's [B,N,1511] input is never formed.  Parameters, state_dict and both checkpoint layouts are those of
    the plain model; the result differs from it by fp32 rounding.

    collapse_pairs=True computes every pair of layers without a ReLU between them (conv1 conv2, conv3 conv4, conv5 conv6)
    as one linear map: A_hat and Theta act on different axes, so conv_b(conv_a(x)) =
    A_hat(A_hat(x Theta_a Theta_b) + b_a Theta_b) + b_b.  The weight products are small dense GEMMs on the autograd tape,
    the two propagations one launch (ops.gcn_aggregate2), and conv5 conv6's 512 -> 3 product ops.gcn_project.  With
    factored_input the product Theta_1 Theta_2 takes conv1.weight's place in the factored op.  Parameters, state_dict and
    both checkpoint layouts are again those of the plain model; the result differs from it by fp32 rounding."""

    def __init__(self, n_dim=3, img_feature_dim=960 + 512, v_num=2048, use_position_encoding=True, factored_input=False,
                 collapse_pairs=False):
        super().__init__()
        conv = GCNConv
        self.use_position_encoding = use_position_encoding
        self.factored_input = bool(factored_input)
        self.collapse_pairs = bool(collapse_pairs)
        self.relu = nn.ReLU()
        n_dim = n_dim + n_dim * 12 if use_position_encoding else n_dim
        self.venc = n_dim
        self.conv1 = conv(n_dim + img_feature_dim, 512)
        self.conv2 = conv(512, 512)
        self.conv3 = conv(512, 512)
        self.conv4 = conv(512, 512)
        self.conv5 = conv(512, 64)
        self.conv6 = conv(64, 3)
        self.fc = nn.Sequential(
            nn.Linear(v_num * 3, 1024),
            nn.Linear(1024, 1024),
            nn.Linear(1024, v_num * 3),
            nn.Tanh()
        )

    def forward(self, meshes: list, rgbs: torch.Tensor, perceptual_features: list, global_features: torch.Tensor = None):
        batch_vertices = self.get_batch_vertices(meshes)                                  # (B, N, 3)
        graph = gcn_graph(meshes[0].faces, batch_vertices.size(1), batch_vertices.device)
        if self.venc not in (0, 3, 39):
            raise ValueError('GCNModel: the vertex encoding has %d channels; the kernels take 3 (n_dim = 3)' % self.venc)
        bounds = gcn_bounds(rgbs)
        if self.collapse_pairs:
            x = self._forward_collapsed(meshes[0].faces, batch_vertices, graph, bounds, perceptual_features, global_features)
        else:
            if self.factored_input:
                h = GcnFactoredInputFunction.apply(batch_vertices, bounds, global_features, self.conv1.weight, self.venc,
                                                   *perceptual_features)
                x = GcnAggregateFunction.apply(h, self.conv1.bias, graph.row_ptr, graph.col, graph.w, False)
            else:
                x = GcnInputFunction.apply(batch_vertices, bounds, global_features, self.venc, *perceptual_features)
                x = self.conv1(x, graph)
            x = self.conv2(x, graph, relu=True)
            x = self.conv3(x, graph)
            x = self.conv4(x, graph, relu=True)
            x = self.conv5(x, graph)
            x = self.conv6(x, graph, relu=True)
        x = x.reshape(x.size(0), -1)
        deformations = self.fc(x).view(x.size(0), -1, 3) * 0.1
        return batch_vertices + deformations

    @staticmethod
    def _pair(a, b):
        """(Theta_a Theta_b, b_a Theta_b) of two layers in a row: their one weight and the bias between the two hops."""
        return torch.matmul(a.weight, b.weight), torch.matmul(a.bias, b.weight)

    def _forward_collapsed(self, faces, verts, graph, bounds, maps, glob):
        blocks = gcn_blocks(faces, verts.size(1), verts.device)
        theta, u = self._pair(self.conv1, self.conv2)
        if self.factored_input:
            h = GcnFactoredInputFunction.apply(verts, bounds, glob, theta, self.venc, *maps)
        else:
            h = torch.matmul(GcnInputFunction.apply(verts, bounds, glob, self.venc, *maps), theta)
        x = gcn_aggregate2(h, u, self.conv2.bias, graph, blocks, relu=True)
        theta, u = self._pair(self.conv3, self.conv4)
        x = gcn_aggregate2(torch.matmul(x, theta), u, self.conv4.bias, graph, blocks, relu=True)
        theta, u = self._pair(self.conv5, self.conv6)
        return gcn_aggregate2(gcn_project(x, theta), u, self.conv6.bias, graph, blocks, relu=True)

    @staticmethod
    def get_edge_indices(mesh):
        """(2, 2E) int64 edge index of the unique undirected edges of mesh.faces, both directions, laid out as
        gcn.py:63-67 lays them out (column 2m = (a_m, b_m), 2m + 1 = (b_m, a_m), edges sorted by (a, b), a < b)."""
        return gcn_edge_index(gcn_edges(mesh.faces)).to(mesh.faces.device)

    @staticmethod
    def get_batch_vertices(meshes: list):
        return torch.cat([mesh.vertices[None] for mesh in meshes])

    @staticmethod
    def positional_encoding(x: torch.Tensor):
        """[x, sin(x), cos(x), sin(2x), cos(2x), ..., sin(32x), cos(32x)] along the last axis (gcn.py:73-82), x [..., 3]."""
        flat = x.reshape(1, -1, 3)
        return GcnInputFunction.apply(flat, None, None, 39).reshape(*x.shape[:-1], 39)

    @classmethod
    def get_local_features(cls, vertices: torch.Tensor, rgbs: torch.Tensor, perceptual_features: list):
        bounds = cls.get_bound_of_images(rgbs)
        return cls.perceptual_feature_pooling(perceptual_features, vertices, bounds)

    @staticmethod
    def get_bound_of_images(imgs: torch.Tensor):
        assert imgs.ndimension() == 4
        return gcn_bounds(imgs)

    @staticmethod
    def perceptual_feature_pooling(perceptual_features: list, points: torch.Tensor, bounds: torch.Tensor):
        """(B, N, sum C_l): bilinear samples (align_corners=True, zero padding) of the maps at the grid of gcn.py:141-153."""
        assert points.ndimension() == 3 and bounds.ndimension() == 2
        return GcnInputFunction.apply(points, bounds, None, 0, *perceptual_features)
