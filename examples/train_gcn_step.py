"""The refinement step of the reference's train_gcn.py (:119-138) on the drop-in surface, with synthetic inputs.

    python examples/train_gcn_step.py [--steps 5] [--batch 8] [--net standin|vpnet_oneres] [--vpn CKPT] [--gcn-input plain|factored] [--gcn-collapse] [--vpn-fold] [--mesh-reg WE,WL,WN] [--surface-loss WP,WF]

--net vpnet_oneres runs the reference's frozen VPNetOneRes (modules/network.py; --vpn CKPT loads a reference checkpoint
into it as train_gcn.py:100-102 does, otherwise it is randomly initialised).  By default a stand-in
produces what train_gcn.py:126 takes from it: 16 sphere primitives (volumes, rotates, translates) and the ResNet-18
feature maps of a 128 x 128 image (64@32², 128@16², 256@8², 512@4²) plus a 512-wide global feature.  The rest is the
reference's step:

    get_vp_meshes / compose_vp_meshes  train_gcn.py:68-88   Meshing.sphere_meshing, Meshing.compose_meshes  (16 x 128 = 2048)
    gcn(predict_meshes, rgbs, ...)     train_gcn.py:129-130 GCNModel                                        (vpn_gcn_*)
    cd_loss + emd_loss                 train_gcn.py:132-135 ChamferDistanceLoss + sqrt(EMD dist).mean()
    Adam(lr, betas=(0.9, 0.99), weight_decay)               train_gcn.py:100-101

--mesh-reg WE,WL,WN (off by default; not in the reference) adds vpn_amd.MeshRegularizationLoss(WE, WL, WN) of predict_vertices
over the composed mesh's faces to the two point-set losses: edge length, uniform Laplacian, normal consistency
(csrc/meshreg.hip).  Chamfer and EMD never look at the triangles; these three keep them from folding.

--surface-loss WP,WF (off by default; not in the reference) adds vpn_amd.PointMeshDistanceLoss(WP, WF) of `points` against
the surface of predict_vertices over the composed mesh's faces: the squared distance from every point to its nearest
triangle and from every triangle to its nearest point (csrc/pointmesh.hip), the data term that sees the triangles.
"""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402
from vpn_amd.modules.network import GCNModel  # noqa: E402

VP_NUM = 16


class StandInVPN(nn.Module):
    """rgbs [B,3,128,128] -> (volumes, rotates, translates) as K lists of (B,3|4|3), perceptual maps, global [B,512]."""

    def __init__(self):
        super().__init__()
        self.levels = nn.ModuleList([nn.Conv2d(3, c, 1) for c in (64, 128, 256, 512)])
        self.head = nn.Linear(512, VP_NUM * 10)

    def forward(self, rgbs):
        maps = [conv(nn.functional.adaptive_avg_pool2d(rgbs, s)) for conv, s in zip(self.levels, (32, 16, 8, 4))]
        g = maps[-1].mean((2, 3))
        p = torch.sigmoid(self.head(g)).view(-1, VP_NUM, 10)
        volumes = [p[:, k, 0:3] * 0.2 + 0.05 for k in range(VP_NUM)]
        rotates = [p[:, k, 3:7] for k in range(VP_NUM)]
        translates = [(p[:, k, 7:10] - 0.5) * 0.8 for k in range(VP_NUM)]
        return volumes, rotates, translates, maps, g


def get_vp_meshes(volumes, rotates, translates):
    batch_vp_meshes = [[] for _ in range(volumes[0].size(0))]
    for i in range(VP_NUM):
        meshes = vpn_amd.Meshing.sphere_meshing(volumes[i], rotates[i], translates[i])
        for b in range(volumes[0].size(0)):
            batch_vp_meshes[b].append(meshes[b])
    return batch_vp_meshes


def compose_vp_meshes(batch_vp_meshes):
    return [vpn_amd.Meshing.compose_meshes(m) for m in batch_vp_meshes]


def calculate_emd_loss(predict_points, gt_points):
    dist, _assignment = vpn_amd.EarthMoverDistanceLoss()(predict_points, gt_points, 0.005, 50)
    return torch.sqrt(dist).mean()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--lr', type=float, default=1e-5)
    ap.add_argument('--net', default='standin', choices=('standin', 'vpnet_oneres'))
    ap.add_argument('--vpn', default=None, help='a VPNetOneRes state_dict saved by the reference (implies --net vpnet_oneres)')
    ap.add_argument('--optimizer', default='torch', choices=('torch', 'hip'),
                    help='hip: vpn_amd.Adam (one launch per step, csrc/optim.hip) with the reference\'s betas (0.9, 0.99)')
    ap.add_argument('--trunk-norm', default='torch', choices=('torch', 'hip', 'hip+pool'),
                    help='hip: the ResNet-18 trunk runs each batch norm with its residual add and ReLU as one op (csrc/trunknorm.hip); '
                         'hip+pool: the stem\'s norm, ReLU and max pool as one op as well')
    ap.add_argument('--trunk-tail', default='torch', choices=('torch', 'hip'),
                    help='hip: the last norm site of the ResNet-18 trunk and the global average pool run as one op (csrc/trunknorm.hip)')
    ap.add_argument('--trunk-conv', default='torch', choices=('torch', 'hip', 'all'),
                    help='hip: the 13 stride-1 3x3 convolutions of the ResNet-18 trunk run on the f32-input MFMA (csrc/trunkconv.hip); '
                         'all: the seven stride-2 ones as well (csrc/trunkstride.hip): no library convolution is left in the trunk')
    ap.add_argument('--gcn-input', default='plain', choices=('plain', 'factored'),
                    help='factored: conv1 projects the maps and the global features and every vertex gathers from the '
                         'projected maps (GCNModel(factored_input=True), csrc/gcn.hip); its [B,N,1511] input is never formed')
    ap.add_argument('--gcn-collapse', action='store_true',
                    help='every pair of layers without a ReLU between them as one linear map: one long product a pair, both '
                         'propagations in one launch (GCNModel(collapse_pairs=True), csrc/gcnpair.hip)')
    ap.add_argument('--vpn-fold', action='store_true',
                    help='the frozen VPNetOneRes runs its trunk in the inference form: every batch norm folded into the convolution '
                         'before it, bias, residual add and ReLU in the convolution\'s epilogue (ResNet18.fold(), csrc/trunkfold.hip); '
                         'needs --net vpnet_oneres; the --trunk-* choices select nothing then')
    ap.add_argument('--mesh-reg', default=None, metavar='WE,WL,WN',
                    help='add the mesh regularisers on predict_vertices with these weights: edge length, uniform Laplacian, normal '
                         'consistency (vpn_amd.MeshRegularizationLoss, csrc/meshreg.hip); a weight of 0 drops its term')
    ap.add_argument('--surface-loss', default=None, metavar='WP,WF',
                    help='add the point-to-surface distance between the ground-truth points and the triangles of predict_vertices '
                         'with these weights: points to faces, faces to points (vpn_amd.PointMeshDistanceLoss, csrc/pointmesh.hip)')
    args = ap.parse_args(argv)
    surface_loss = None
    if args.surface_loss is not None:
        try:
            weights = [float(w) for w in args.surface_loss.split(',')]
        except ValueError:
            weights = []
        if len(weights) != 2:
            ap.error('--surface-loss takes two numbers WP,WF')
        surface_loss = vpn_amd.PointMeshDistanceLoss(*weights)
    mesh_reg = None
    if args.mesh_reg is not None:
        try:
            weights = [float(w) for w in args.mesh_reg.split(',')]
        except ValueError:
            weights = []
        if len(weights) != 3:
            ap.error('--mesh-reg takes three numbers WE,WL,WN')
        mesh_reg = vpn_amd.MeshRegularizationLoss(*weights)
    if args.vpn_fold and not (args.vpn or args.net == 'vpnet_oneres'):
        ap.error('--vpn-fold needs --net vpnet_oneres (or --vpn CKPT): the stand-in has no trunk to fold')
    dev = torch.device('cuda')
    torch.manual_seed(1234)
    if args.vpn or args.net == 'vpnet_oneres':
        vpn = vpn_amd.VPNetOneRes(vp_num=VP_NUM, trunk=vpn_amd.ResNet18(fused_norm=args.trunk_norm != 'torch', fused_pool=args.trunk_norm == 'hip+pool', hip_conv=args.trunk_conv in ('hip', 'all'), hip_conv_strided=args.trunk_conv == 'all', fused_tail=args.trunk_tail == 'hip') if (args.trunk_norm, args.trunk_conv, args.trunk_tail) != ('torch', 'torch', 'torch') else None)
        if args.vpn:
            vpn.load_state_dict(torch.load(args.vpn, map_location='cpu'))
        vpn = vpn.to(dev).eval()
        if args.vpn_fold:
            vpn.resnet.fold()
    else:
        vpn = StandInVPN().to(dev).eval()
    gcn = GCNModel(factored_input=args.gcn_input == 'factored', collapse_pairs=args.gcn_collapse).to(dev)
    adam = vpn_amd.Adam if args.optimizer == 'hip' else torch.optim.Adam
    optimizer = adam(params=gcn.parameters(), lr=args.lr, betas=(0.9, 0.99), weight_decay=1e-6)      # train_gcn.py:105
    cd_loss_func = vpn_amd.ChamferDistanceLoss()
    B = args.batch
    losses = []
    for step in range(args.steps):
        rgbs = torch.zeros(B, 3, 128, 128, device=dev)
        rgbs[:, :, 24:104, 16:112] = torch.rand(B, 3, 80, 96, device=dev)
        points = (torch.rand(B, VP_NUM * 128, 3, device=dev) - 0.5) * 0.8
        with torch.no_grad():
            volumes, rotates, translates, perceptual_features, global_features = vpn(rgbs)
        predict_meshes = compose_vp_meshes(get_vp_meshes(volumes, rotates, translates))
        predict_vertices = gcn(predict_meshes, rgbs, perceptual_features, global_features)
        cd_loss = cd_loss_func(predict_vertices, points)
        emd_loss = calculate_emd_loss(predict_vertices, points)
        total_loss = cd_loss + emd_loss
        if mesh_reg is not None:
            reg_loss = mesh_reg(predict_vertices, predict_meshes[0].faces)
            total_loss = total_loss + reg_loss
        if surface_loss is not None:
            surf_loss = surface_loss(points, predict_vertices, predict_meshes[0].faces)
            total_loss = total_loss + surf_loss
        optimizer.zero_grad()
        total_loss.backward()
        optimizer.step()
        losses.append((float(cd_loss), float(emd_loss)))
        print('step %d  CD Loss = %.6f, EMD Loss = %.6f' % (step, losses[-1][0], losses[-1][1])
              + ('' if mesh_reg is None else ', Mesh Reg = %.6f (edge %.6f, lap %.6f, normal %.6f)' % ((float(reg_loss),) + tuple(mesh_reg.last.tolist())))
              + ('' if surface_loss is None else ', Surface Loss = %.6f (point %.6f, face %.6f)' % ((float(surf_loss),) + tuple(surface_loss.last.tolist()))),
              flush=True)
    return losses


if __name__ == '__main__':
    main()
