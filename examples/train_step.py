"""A training step of the reference (train.py:221-268) on the drop-in surface, with a stand-in network.

    python examples/train_step.py [--steps 20] [--net standin|vpnet_oneres|vpnet_twores] [--optimizer torch|hip] [--trunk-norm torch|hip|hip+pool] [--trunk-conv torch|hip|all] [--trunk-tail torch|hip] [--occupancy-loss W_OCC,W_OV[,TAU]]

By default a two-layer MLP on a random feature vector produces the three head outputs (volumes [B,3K], rotates [B,4K],
translates [B,3K]); --net vpnet_oneres / vpnet_twores trains the reference's network instead (modules/network.py: a
ResNet-18 trunk, randomly initialised here, and the FC heads of csrc/fcstack.hip) on the ground-truth
silhouette repeated over three channels as the image.  Everything after that is the
code path of the reference, through vpn_amd's mirror of its modules:

    head post-processing     vpnet_one_resnet.py:34-41   pack_head_outputs
    predicted points         train.py:105-120            Sampling.sample_primitives
    view-centred Chamfer     train.py:160                ChamferDistanceLoss
    object-centred Chamfer   train.py:158-161            view_to_obj_points + ChamferDistanceLoss
    silhouette loss          train.py:176                SilhouetteLoss
    VP diversity loss        train.py:185                VPDiverseLoss
    EMD loss                 train.py:193                EarthMoverDistanceLoss

--occupancy-loss W_OCC,W_OV[,TAU] (off by default; not in the reference; the non-fused path only) adds
vpn_amd.OccupancyLoss(W_OCC, W_OV, TAU): the cross-entropy of the soft union of the predicted primitives against the
occupancy of the target assembly, and the overlap penalty, at the cell centres of a 16^3 grid plus the ground-truth points
jittered by a fixed-seed normal.
"""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402


class Heads(nn.Module):
    """Stand-in for VPNetOneRes: features -> (volumes, rotates, translates) raw head outputs."""

    def __init__(self, feat, K):
        super().__init__()
        self.trunk = nn.Sequential(nn.Linear(feat, 256), nn.ReLU())
        self.volume_fc, self.rotate_fc, self.translate_fc = nn.Linear(256, 3 * K), nn.Linear(256, 4 * K), nn.Linear(256, 3 * K)

    def forward(self, x):
        h = self.trunk(x)
        return self.volume_fc(h), self.rotate_fc(h), self.translate_fc(h)


def head_params(net, feats, gt_sil):
    """[B,K,10] from the stand-in (features) or from the reference's network (images)."""
    if isinstance(net, Heads):
        return vpn_amd.pack_head_outputs(*net(feats))
    out = net.forward_packed(gt_sil.expand(-1, 3, -1, -1).contiguous())
    return out[0] if isinstance(out, tuple) else out


def training_losses(net, feats, gt_points, gt_sil, dists, elevs, azims, angles, kinds, sample_num, weights, seed, occupancy=None):
    """total loss of train.py:243-262 (w = (L_VIEW_CD, L_CAN_CD, L_SIL, L_VP_DIV, L_EMD)) and its parts.  occupancy: None, or
    (vpn_amd.OccupancyLoss, queries, labels), whose weighted sum is added as the part 'occ'."""
    K = len(kinds)
    params = head_params(net, feats, gt_sil)                                      # [B,K,10]
    volumes, rotates, translates = vpn_amd.split_primitives(params)
    pred = vpn_amd.Sampling.sample_primitives(params, kinds, sample_num, seed=seed)   # [B, K*n, 3], view-centred
    cd = vpn_amd.ChamferDistanceLoss()
    view_cd = cd(pred, gt_points)
    obj_cd = cd(vpn_amd.view_to_obj_points(pred, dists, elevs, azims, angles),
                vpn_amd.view_to_obj_points(gt_points, dists, elevs, azims, angles))
    sil = vpn_amd.SilhouetteLoss()(vpn_amd.PrimitivePack(params, kinds), gt_sil, dists, elevs, azims)
    div = vpn_amd.VPDiverseLoss(vp_num=K)(translates, gt_points)
    dist, _ = vpn_amd.EarthMoverDistanceLoss()(pred, gt_points, 0.005, 50)         # needs K*n == M (emd_module.py:36)
    emd = torch.sqrt(dist).mean()
    w = weights
    total = w[0] * view_cd + w[1] * obj_cd + w[2] * sil + w[3] * div + w[4] * emd
    parts = {'view_cd': view_cd, 'obj_cd': obj_cd, 'sil': sil, 'vp_div': div, 'emd': emd}
    if occupancy is not None:
        occ_loss, queries, labels = occupancy
        parts['occ'] = occ_loss(params, kinds, queries, labels)
        total = total + parts['occ']
    return total, parts


def training_losses_fused(net, feats, gt_points, gt_sil, dists, elevs, azims, angles, kinds, sample_num, weights, seed):
    """The same loss as ONE autograd node (vpn_amd.TrainStepLossFunction: 9 launches forward with the auction on a second
    stream, 1 backward).  Needs K * sample_num >= 512 sampled points against as many GT points."""
    params = head_params(net, feats, gt_sil)                                      # [B,K,10]
    size = gt_sil.shape[-1]
    gt_canon = vpn_amd.view_to_obj_points(gt_points, dists, elevs, azims, angles)
    view_cd, obj_cd, sil, div, emd, total = vpn_amd.TrainStepLossFunction.apply(
        params, kinds, gt_points, gt_canon, gt_sil, dists, elevs, azims, angles, sample_num, seed, 0, size, size, weights)
    return total, {'view_cd': view_cd, 'obj_cd': obj_cd, 'sil': sil, 'vp_div': div, 'emd': emd}   # the WEIGHTED terms


def draw_inputs(B, K, seed=0):
    """The random inputs of a batch, on the host: (feats [B,64], target [B,K,10]), the target K random ellipsoids.  The one place
    these draws are made: make_batch and target_assembly both come here."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, 64, generator=g)
    v = (torch.rand(B, K, 3, generator=g) + 0.1) / torch.tensor([8.0, 10.0, 10.0])
    target = torch.cat([v, torch.rand(B, K, 4, generator=g), 0.3 * (torch.rand(B, K, 3, generator=g) * 2 - 1)], 2)
    return feats, target


def make_batch(B, K, sample_num, size, dev, seed=0):
    # a target made of K random ellipsoids: its surface points and its silhouette
    feats, target = (t.to(dev) for t in draw_inputs(B, K, seed))
    kinds = [vpn_amd.SPHERE] * K
    with torch.no_grad():
        gt_points = vpn_amd.Sampling.sample_primitives(target, kinds, sample_num, seed=99)
        dists = torch.ones(B, device=dev)
        elevs = torch.zeros(B, device=dev)
        azims = torch.zeros(B, device=dev)
        _, alpha, _ = vpn_amd.VertexRenderer.render(vpn_amd.PrimitivePack(target, kinds), dists, elevs, azims,
                                                    image_size=(size, size))
        gt_sil = (alpha.reshape(B, 1, size, size) > 0.5).float()
    return feats, gt_points, gt_sil, dists, elevs, azims, torch.zeros(B, device=dev), kinds


def target_assembly(B, K, dev, seed=0):
    """The target of make_batch(B, K, ..., seed): params [B,K,10] of its K random ellipsoids."""
    return draw_inputs(B, K, seed)[1].to(dev)


def occupancy_queries(gt_points, target, kinds, jitter=0.02, seed=77):
    """(queries [B, 16^3 + M, 3], labels uint8 [B, 16^3 + M]): the cell centres of a 16^3 grid over the unit cube and the
    ground-truth points moved by a fixed-seed normal of scale `jitter`, labelled by the occupancy of the target assembly."""
    B, dev = gt_points.shape[0], gt_points.device
    noise = torch.randn(gt_points.shape, generator=torch.Generator().manual_seed(seed)).to(dev)
    grid = vpn_amd.grid_queries(16, device=dev)
    queries = torch.cat([grid[None].expand(B, -1, -1), gt_points + jitter * noise], 1).contiguous()
    return queries, vpn_amd.primitive_occupancy(target, kinds, queries)


def augment_batch(batch, which, it):
    """train.py:232-237 on the HIP augmentation stage, in the reference's order.  The stand-in network reads features, not
    pixels, so the mixed rgbs (here: the silhouette repeated over three channels) have no consumer.  `mixup` moves the
    points only; `pointmixup` is the whole point_mixup_data: mixed clouds, a mesh of convex parts from each, its render as
    the new silhouette and its surface samples as the new points.  `acdmix` is the data of train.py -a_mix
    made on the fly (generate.py:108-173): every sample's cloud is mixed with its successor's as two objects,
    and one random view of the mix gives the silhouette, the points and the camera."""
    feats, gt_points, gt_sil, dists, elevs, azims, angles, kinds = batch
    if 'acdmix' in which:
        torch.manual_seed(4000 + it)
        rgba, _verts, gt, d, e, a = vpn_amd.acd_mix_data(gt_points, gt_points.roll(1, 0), views=1, img_size=gt_sil.shape[-1],
                                                         num_points=gt_points.shape[1])
        gt_points, gt_sil = gt[:, 0].contiguous(), (rgba[:, 0, 3:4] > 0.5).float()
        dists, elevs, azims = d[:, 0].contiguous(), e[:, 0].contiguous(), a[:, 0].contiguous()
    if 'rotate' in which:
        # AUGMENT_3D['rotate'] (dataset.py:120-121, train.py): the image and the points turn by the SAME angle.  The stand-in
        # image is the silhouette as an opaque-white RGBA rendering; prepare_images draws the angles, rotates the image
        # (PIL's nearest-neighbour rotation) and returns them for the points.
        S = gt_sil.shape[-1]
        a = (gt_sil[:, 0] * 255).to(torch.uint8)
        rgba = torch.stack([a, a, a, a], -1).contiguous()
        _, gt_sil, angles = vpn_amd.prepare_images(rgba, size=S, jitter=False, rotate=True, seed=5000 + it)
        gt_points = vpn_amd.rotate_points_forward_x_axis(gt_points, angles)
    if 'cutmix' in which:
        _, gt_sil, gt_points = vpn_amd.cut_mix_data(gt_sil.expand(-1, 3, -1, -1), gt_sil, gt_points, seed=2000 + it)
    if 'mixup' in which:
        gt_points = vpn_amd.mixup_points(gt_points)
    if 'pointmixup' in which:
        _, sil, gt_points = vpn_amd.point_mixup_data(gt_points, img_size=gt_sil.shape[-1], num_points=gt_points.shape[1],
                                                     seed=3000 + it)
        gt_sil = (sil > 0.5).float()
    return feats, gt_points, gt_sil, dists, elevs, azims, angles, kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=8)          # config.py:9
    ap.add_argument('--prims', type=int, default=16)         # config.py:34
    ap.add_argument('--sample-num', type=int, default=128)   # config.py:8
    ap.add_argument('--size', type=int, default=128)         # config.py:49
    ap.add_argument('--net', default='standin', choices=('standin', 'vpnet_oneres', 'vpnet_twores'))
    ap.add_argument('--fused', action='store_true', help='the whole loss as one autograd node (TrainStepLossFunction)')
    ap.add_argument('--augment', default='', help='comma-separated subset of rotate,cutmix,mixup,pointmixup,acdmix (config.py AUGMENT_3D; default: none)')
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
    ap.add_argument('--occupancy-loss', default=None, metavar='W_OCC,W_OV[,TAU]',
                    help='add vpn_amd.OccupancyLoss(W_OCC, W_OV, TAU): the soft union of the predicted primitives against the occupancy '
                         'of the target assembly, and the overlap penalty (not in the reference; the non-fused path, no augmentation)')
    args = ap.parse_args()
    augment = [a for a in args.augment.split(',') if a]
    assert set(augment) <= {'rotate', 'cutmix', 'mixup', 'pointmixup', 'acdmix'}, augment
    occ_args = None
    if args.occupancy_loss is not None:
        try:
            occ_args = [float(w) for w in args.occupancy_loss.split(',')]
            assert len(occ_args) in (2, 3)
        except (ValueError, AssertionError):
            ap.error('--occupancy-loss takes two or three numbers W_OCC,W_OV[,TAU]')
        if args.fused or augment:
            ap.error('--occupancy-loss belongs to the non-fused path without --augment: its labels are those of the target assembly')
    losses = training_losses_fused if args.fused else training_losses
    dev = torch.device('cuda')
    torch.manual_seed(1234)
    batch = make_batch(args.batch, args.prims, args.sample_num, args.size, dev)

    own_trunk = (args.trunk_norm, args.trunk_conv, args.trunk_tail) != ('torch', 'torch', 'torch')

    def trunk():           # None: the model builds its own plain trunk, as it always did
        return vpn_amd.ResNet18(fused_norm=args.trunk_norm != 'torch', fused_pool=args.trunk_norm == 'hip+pool', hip_conv=args.trunk_conv in ('hip', 'all'), hip_conv_strided=args.trunk_conv == 'all', fused_tail=args.trunk_tail == 'hip') if own_trunk else None
    net = {'standin': lambda: Heads(64, args.prims), 'vpnet_oneres': lambda: vpn_amd.VPNetOneRes(vp_num=args.prims, trunk=trunk()),
           'vpnet_twores': lambda: vpn_amd.VPNetTwoRes(vp_num=args.prims, trunk=(trunk(), trunk()) if own_trunk else None)}[args.net]().to(dev)
    if args.optimizer == 'hip':
        opt = vpn_amd.Adam(net.parameters(), lr=1e-3, betas=(0.9, 0.99))                # train.py:83
    else:
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    weights = (1.0, 1.0, 1.0, 0.1, 1.0)
    extra, occ_loss = {}, None
    if occ_args is not None:
        occ_loss = vpn_amd.OccupancyLoss(*occ_args)
        extra['occupancy'] = (occ_loss,) + occupancy_queries(batch[1], target_assembly(args.batch, args.prims, dev), batch[7])
    for it in range(args.steps):
        opt.zero_grad()
        total, parts = losses(net, *(augment_batch(batch, augment, it) if augment else batch), args.sample_num, weights,
                              seed=1000 + it, **extra)
        total.backward()
        opt.step()
        print('step %3d  total %.5f  ' % (it, float(total.detach())) + '  '.join('%s %.5f' % (k, float(v.detach())) for k, v in parts.items())
              + ('' if occ_loss is None else ' (occupancy %.5f, overlap %.5f)' % tuple(occ_loss.last.tolist())), flush=True)


if __name__ == '__main__':
    main()
