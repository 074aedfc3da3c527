"""Time the point-to-surface distance (vpn_amd.point_mesh_distance, csrc/pointmesh.hip) on one MI355X at the
reference shape: B = 8, P = 2048, V = 16 x 128 = 2048, F = 4032.  Writes profiles/pointmesh_time.txt.

    python tools/time_pointmesh.py [--replays 50] [--out profiles/pointmesh_time.txt]

  (a) the op, forward alone and forward + backward to the points and the vertices with an upstream gradient [2], next to
      ChamferDistanceLoss(predict_vertices, points) at the same shape, the term it stands beside in the step; the pair tests
      per second of the op's forward (B P F pairs).  No composition of this op from ATen ops fits in memory (a [B,P,F]
      closest-point table with its temporaries is several GB), so there is nothing of that kind to race;
  (b) the model step of examples/train_gcn_step.py (GCNModel forward, Chamfer + EMD, backward to the parameters) without
      and with --surface-loss 1,1.

Each variant is captured into a graph once; the graphs of a row are replayed in turn in the same process, every replay
between two device events; reported is the median (10th .. 90th percentile) of `replays` replays after 20 warm-up replays.
There is no speed bar: the numbers are reported, not asserted.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402
from vpn_amd.modules.gcn import GCNModel  # noqa: E402
from vpn_amd.modules.meshing import TriangleMesh  # noqa: E402
from time_gcn_factored import inputs  # noqa: E402
from time_trunknorm import capture, measure  # noqa: E402


def cloud(verts, dev):
    """Ground-truth points as the example draws them: uniform in a box of side 0.8."""
    gen = torch.Generator().manual_seed(27)
    return ((torch.rand(verts.shape[0], 2048, 3, generator=gen) - 0.5) * 0.8).to(dev)


def op_steps(dev, backward):
    verts, faces, _maps, _glob, _rgbs = inputs(dev)
    points = cloud(verts, dev)
    cd = vpn_amd.ChamferDistanceLoss()
    if not backward:
        return {'ChamferDistanceLoss': lambda: cd(verts, points), 'point_mesh_distance': lambda: vpn_amd.point_mesh_distance(points, verts, faces)}
    v, p = verts.clone().requires_grad_(True), points.clone().requires_grad_(True)
    up = torch.tensor([0.3, -2.0], device=dev)
    return {'ChamferDistanceLoss': lambda: torch.autograd.grad(cd(v, p), [v, p]),
            'point_mesh_distance': lambda: torch.autograd.grad((vpn_amd.point_mesh_distance(p, v, faces) * up).sum(), [p, v])}


def model_steps(dev):
    verts, faces, maps, glob, rgbs = inputs(dev)
    torch.manual_seed(1)
    model = GCNModel().to(dev)
    points = cloud(verts, dev)
    cd, emd, surf = vpn_amd.ChamferDistanceLoss(), vpn_amd.EarthMoverDistanceLoss(), vpn_amd.PointMeshDistanceLoss(1.0, 1.0)
    leaves = list(model.parameters())

    def make(with_surface):
        def step():
            meshes = [TriangleMesh(verts[b], faces) for b in range(verts.shape[0])]
            pred = model(meshes, rgbs, maps, glob)
            loss = cd(pred, points) + torch.sqrt(emd(pred, points, 0.005, 50)[0]).mean()
            if with_surface:
                loss = loss + surf(points, pred, faces)
            return torch.autograd.grad(loss, leaves)
        return step
    return {'Chamfer + EMD': make(False), '+ --surface-loss': make(True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replays', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'pointmesh_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_pointmesh.py needs a GPU: nothing is measured on a CPU')
    if args.replays < 50:
        raise SystemExit('at least 50 replays per variant')
    dev = torch.device('cuda:0')
    B, P, F = 8, 2048, 4032
    lines = ['tools/time_pointmesh.py --replays %d on one MI355X (torch %s): B = 8, P = 2048, V = 2048 = 16 spheres of 128, F = 4032, '
             '%.1f M point-triangle pairs; us, median [10th .. 90th percentile] of %d graph replays, each between two device '
             'events, after 20 warm-up replays; the variants of a row alternate' % (args.replays, torch.__version__, B * P * F / 1e6, args.replays)]
    rows = [('(a) forward', lambda: op_steps(dev, False)), ('(a) forward + backward to the points and the vertices', lambda: op_steps(dev, True)),
            ('(b) model step of examples/train_gcn_step.py: GCNModel forward, losses, backward to the parameters', lambda: model_steps(dev))]
    for label, steps in rows:
        steps = steps()
        graphs = {k: capture(v) for k, v in steps.items()}
        t = {k: torch.tensor(v, dtype=torch.float64) * 1e3 for k, v in measure(graphs, args.replays).items()}
        q = {k: [float(torch.quantile(v, p)) for p in (0.5, 0.1, 0.9)] for k, v in t.items()}
        first = len(lines)
        lines.append(label)
        base = q[next(iter(graphs))][0]
        for k in graphs:
            lines.append('    %-20s %8.1f us [%8.1f .. %8.1f]   %5.2f x the first variant' % (k, *q[k], q[k][0] / base))
        if label == '(a) forward':
            lines.append('    point_mesh_distance forward: %.1f G pair tests per second' % (B * P * F / q['point_mesh_distance'][0] / 1e3))
        print('\n'.join(lines[first:]), flush=True)
        del graphs, steps
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
