"""The evaluation loops of the reference on the drop-in surface, with stand-in networks and synthetic data.

    python examples/eval_step.py [--batches 6] [--batch 8]          # test.py:68-135: Chamfer only
    python examples/eval_step.py --gcn [--gcn-input factored] [--gcn-collapse]     # test_gcn.py:115-178: Chamfer + EMD on refined vertices

    python examples/eval_step.py --dump DIR [--three-elev] [--gcn]  # also write the visual dump of sample 0 every third batch
    python examples/eval_step.py --surface [--thresholds 0.01,0.02] [--gcn]        # also the surface metrics
    python examples/eval_step.py --volume [--resolution 32] [--gcn]                # also volumetric IoU
    python examples/eval_step.py --surface --outer [--outer-resolution 64] [--gcn] # the surface metrics on the OUTER surface (4.30)

The trained networks and the dataset are out of scope; what the loops do with a batch is
the reference's, under torch.no_grad():

    test.py       head -> Sampling (16 x 128 points) -> ChamferDistanceLoss(each_batch=True) * L_VIEW_CD   test.py:93-102
    test_gcn.py   VPN -> sphere meshes -> GCNModel (2048 vertices) -> Chamfer + sqrt(EMD dist).mean(1)     test_gcn.py:136-143
    bookkeeping   batch means, per-class sums and counts, the table at the end                             EvaluationMeter
    dumps         Visualizer.render_vp_meshes (test.py:110-124) / render_refine_vp_meshes (test_gcn.py:154-161)
    --surface     SurfaceEvaluationMeter beside the meter above: F-score at the thresholds, Chamfer-L1 and -L2; with --gcn on
                  points sampled from the refined SURFACE with normal consistency (the stand-in ground-truth normals point away
                  from the origin), without it on the sampled primitive points, which carry no normals
    --outer       with --surface: the points are drawn from the boundary of the UNION instead: without --gcn
                  SurfaceEvaluationMeter.update_primitives (the primitive field's zero level on an outer-resolution^3 lattice), with
                  it the zero level of the refined mesh's signed distance (ops.mesh_signed_distance -> ops.isosurface ->
                  update_surface); no point lies on a wall inside another primitive.  With --dump sample 0's union mesh is saved
                  as an OBJ file
    --volume      VolumeEvaluationMeter beside them: IoU, precision and recall of the occupied volume on a resolution^3 grid; the
                  prediction is the primitive assembly's closed-form occupancy (with --gcn the refined mesh's winding number), the
                  stand-in ground truth a packed batch of ellipsoid meshes

The class indices cycle over the reference's 13 ShapeNet classes; the last batch is short."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402
from examples.train_gcn_step import StandInVPN, compose_vp_meshes, get_vp_meshes  # noqa: E402
from examples.train_step import Heads  # noqa: E402
from vpn_amd.modules.network import GCNModel  # noqa: E402

CLASS_NAMES = ['airplane', 'rifle', 'display', 'table', 'telephone', 'car', 'chair', 'bench', 'lamp', 'cabinet', 'loudspeaker',
               'sofa', 'watercraft']
L_VIEW_CD = 1.0
VP_NUM, SAMPLE_NUM = 16, 128


def batches(n, B):
    """(batch size, class indices as a DataLoader yields them) of n batches, the last one short."""
    seen = 0
    for k in range(n):
        b = B if k < n - 1 or B < 3 else B - 3
        yield b, torch.arange(seen, seen + b) % len(CLASS_NAMES)
        seen += b


def gt_meshes(b, it, dev):
    """The stand-in ground truth of --volume: b ellipsoid meshes (semi-axes 0.15 .. 0.35) as one MeshBatch; its own generator,
    so the other draws of the loop are what they are without the flag."""
    from vpn_amd.modules.meshing import uv_sphere
    g = torch.Generator().manual_seed(300 + it)
    sv, sf = uv_sphere()
    sv, sf = sv.cpu(), sf.cpu().flip(1)          # the template is wound clockwise seen from outside: flipped, w = +1 inside
    return vpn_amd.MeshBatch.pack([(sv * (0.15 + 0.2 * torch.rand(3, generator=g)), sf) for _ in range(b)], dev)


@torch.no_grad()
def test(args, dev):
    model = Heads(64, VP_NUM).to(dev).eval()
    kinds = [vpn_amd.SPHERE] * VP_NUM
    meter = vpn_amd.EvaluationMeter(CLASS_NAMES, dev, emd=False, cd_scale=L_VIEW_CD)
    surface = vpn_amd.SurfaceEvaluationMeter(CLASS_NAMES, dev, thresholds=args.thresholds) if args.surface else None
    volume = vpn_amd.VolumeEvaluationMeter(CLASS_NAMES, dev, resolution=args.resolution) if args.volume else None
    for it, (b, class_indices) in enumerate(batches(args.batches, args.batch)):
        feats = torch.randn(b, 64, device=dev)
        view_points = (torch.rand(b, VP_NUM * SAMPLE_NUM, 3, device=dev) - 0.5) * 0.8
        params = vpn_amd.pack_head_outputs(*model(feats))
        predict_points = vpn_amd.Sampling.sample_primitives(params, kinds, SAMPLE_NUM, seed=100 + it)
        meter.update(predict_points, view_points, class_indices)
        if surface is not None and args.outer:
            surface.update_primitives(params, kinds, view_points, class_indices, resolution=args.outer_resolution,
                                      n=VP_NUM * SAMPLE_NUM, seed=100 + it)
            if args.dump and it % 3 == 0:
                union = vpn_amd.Meshing.union_meshes(params[:1], kinds, resolution=args.outer_resolution)
                union.meshes()[0].save_mesh(os.path.join(args.dump, 'union_%03d.obj' % it))
        elif surface is not None:
            surface.update(predict_points, view_points, class_indices)
        if volume is not None:
            volume.update_primitives(params, kinds, gt_meshes(b, it, dev), class_indices)
        if args.dump and it % 3 == 0:                                    # test.py:110-124: the K meshes of sample 0
            volumes, rotates, translates = vpn_amd.split_primitives(params)
            vp_meshes = [vpn_amd.Meshing.sphere_meshing(volumes[k][:1], rotates[k][:1], translates[k][:1])[0] for k in range(VP_NUM)]
            vpn_amd.Visualizer.render_vp_meshes(torch.rand(3, 128, 128, device=dev), vp_meshes,
                                                os.path.join(args.dump, 'vp_%03d.gif' % it), is_three_elev=args.three_elev)
    res = meter.report(args.epoch)
    if surface is not None:
        surface.report()
    if volume is not None:
        volume.report()
    return res


@torch.no_grad()
def test_gcn(args, dev):
    vpn = StandInVPN().to(dev).eval()
    gcn = GCNModel(factored_input=args.gcn_input == 'factored', collapse_pairs=args.gcn_collapse).to(dev).eval()
    meter = vpn_amd.EvaluationMeter(CLASS_NAMES, dev, emd=True)
    surface = vpn_amd.SurfaceEvaluationMeter(CLASS_NAMES, dev, thresholds=args.thresholds) if args.surface else None
    volume = vpn_amd.VolumeEvaluationMeter(CLASS_NAMES, dev, resolution=args.resolution) if args.volume else None
    for it, (b, class_indices) in enumerate(batches(args.batches, args.batch)):
        rgbs = torch.zeros(b, 3, 128, 128, device=dev)
        rgbs[:, :, 24:104, 16:112] = torch.rand(b, 3, 80, 96, device=dev)
        gt_points = (torch.rand(b, VP_NUM * 128, 3, device=dev) - 0.5) * 0.8
        volumes, rotates, translates, perceptual_features, global_features = vpn(rgbs)
        vp_meshes = get_vp_meshes(volumes, rotates, translates)
        predict_meshes = compose_vp_meshes(vp_meshes)
        predict_vertices = gcn(predict_meshes, rgbs, perceptual_features, global_features)
        meter.update(predict_vertices, gt_points, class_indices)
        if surface is not None and args.outer:
            # the refined mesh re-meshed without its interior faces; the composed template is wound clockwise seen from outside
            cx, cy, cz, nodes = vpn_amd.lattice(args.outer_resolution, -0.5, 0.5, dev)
            distance = vpn_amd.mesh_signed_distance(predict_vertices, predict_meshes[0].faces.flip(1), nodes)
            union = vpn_amd.isosurface(distance.view(b, cz.numel(), cy.numel(), cx.numel()), (cx, cy, cz))
            surface.update_surface(union, gt_points, class_indices, n=gt_points.size(1), seed=200 + it,
                                   gt_normals=torch.nn.functional.normalize(gt_points, dim=-1))
            if args.dump and it % 3 == 0:
                union.meshes()[0].save_mesh(os.path.join(args.dump, 'union_%03d.obj' % it))
        elif surface is not None:                                        # one face list for the batch: the composed topology
            gt_normals = torch.nn.functional.normalize(gt_points, dim=-1)
            surface.update_mesh(predict_vertices, predict_meshes[0].faces, gt_points, class_indices, n=gt_points.size(1),
                                seed=200 + it, gt_normals=gt_normals)
        if volume is not None:
            # the composed sphere template is wound clockwise seen from outside; occupancy wants w = +1 inside
            volume.update_mesh(predict_vertices, predict_meshes[0].faces.flip(1), gt_meshes(b, it, dev), class_indices)
        if args.dump and it % 3 == 0:                                    # test_gcn.py:154-161
            vpn_amd.Visualizer.render_refine_vp_meshes(rgbs[0], vp_meshes[0], predict_vertices[0],
                                                       os.path.join(args.dump, 'refine_%03d.gif' % it))
    res = meter.report(args.epoch)
    if surface is not None:
        surface.report()
    if volume is not None:
        volume.report()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gcn', action='store_true', help='the test_gcn.py loop (Chamfer + EMD on the refined vertices)')
    ap.add_argument('--gcn-input', default='plain', choices=('plain', 'factored'),
                    help='with --gcn: conv1 of the GCN in factored form (GCNModel(factored_input=True))')
    ap.add_argument('--gcn-collapse', action='store_true',
                    help='with --gcn: every pair of GCN layers as one linear map (GCNModel(collapse_pairs=True))')
    ap.add_argument('--batches', type=int, default=6)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--epoch', type=int, default=0)
    ap.add_argument('--dump', default='', metavar='DIR', help='write the visual dump of sample 0 every third batch into DIR')
    ap.add_argument('--three-elev', action='store_true', help='three elevations per frame (is_three_elev of render_vp_meshes)')
    ap.add_argument('--surface', action='store_true',
                    help='also run SurfaceEvaluationMeter: F-score, Chamfer-L1 / -L2 and (with --gcn) normal consistency')
    ap.add_argument('--thresholds', default=(0.01, 0.02), type=lambda s: tuple(float(t) for t in s.split(',')),
                    help='with --surface: the distance thresholds of the F-score, comma separated (default 0.01,0.02)')
    ap.add_argument('--outer', action='store_true',
                    help='with --surface: score points drawn from the outer surface of the union (surface nets, DESIGN.md 4.30)')
    ap.add_argument('--outer-resolution', type=int, default=64, help='with --outer: the lattice has outer-resolution^3 nodes')
    ap.add_argument('--volume', action='store_true',
                    help='also run VolumeEvaluationMeter: volumetric IoU, precision and recall against stand-in ground-truth meshes')
    ap.add_argument('--resolution', type=int, default=32, help='with --volume: the query grid has resolution^3 cell centres')
    args = ap.parse_args(argv)
    if args.outer and not args.surface:
        ap.error('--outer chooses where --surface draws its points: give --surface too')
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    torch.manual_seed(1234)
    dev = torch.device('cuda')
    return (test_gcn if args.gcn else test)(args, dev)


if __name__ == '__main__':
    main()
