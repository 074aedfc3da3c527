"""Time the mesh regularisers (vpn_amd.mesh_regularizers, csrc/meshreg.hip) on one MI355X at the reference
shape: B = 8, V = 16 x 128 = 2048, F = 4032, E = 6048.  Writes profiles/meshreg_time.txt.

    python tools/time_meshreg.py [--replays 50] [--out profiles/meshreg_time.txt]

  (a) the op, forward + backward to the vertices with an upstream gradient [3], against the same three losses composed from
      ATen ops in fp32 on the GPU (index_select, index_add_, cross, ...: what a user writes without the op; its scatter-adds
      are atomic, so its gradient is not bit-equal from run to run), all terms and each alone;
  (b) the model step of examples/train_gcn_step.py (GCNModel forward, Chamfer + EMD, backward to the parameters) without
      and with --mesh-reg 0.1,0.5,0.01.

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
from vpn_amd import ops  # noqa: E402
from vpn_amd.modules.gcn import GCNModel  # noqa: E402
from vpn_amd.modules.meshing import TriangleMesh  # noqa: E402
from time_gcn_factored import inputs  # noqa: E402
from time_trunknorm import capture, measure  # noqa: E402

TERMS = ('edge', 'lap', 'normal')


def aten_tables(topo, dev):
    """The index tensors of the composition, made once (a user would cache them too): int64 on the device."""
    e, f, p = topo.host['edges'].long().to(dev), topo.host['faces'].long().to(dev), topo.pairs.to(dev)
    rows, cols = torch.cat([e[:, 0], e[:, 1]]), torch.cat([e[:, 1], e[:, 0]])
    deg = torch.zeros(topo.n, device=dev).index_add_(0, rows, torch.ones(rows.numel(), device=dev))
    return dict(e0=e[:, 0].contiguous(), e1=e[:, 1].contiguous(), rows=rows, cols=cols, has=(deg > 0)[None, :, None],
                inv_deg=(1.0 / deg.clamp_min(1))[None, :, None], f0=f[:, 0].contiguous(), f1=f[:, 1].contiguous(),
                f2=f[:, 2].contiguous(), p0=p[:, 0].contiguous(), p1=p[:, 1].contiguous(), s=p[:, 2].float())


def aten_regularizers(verts, t, terms):
    """The three terms from ATen ops over the same topology (l0 = 0): the composition the op replaces."""
    out = [verts.new_zeros(())] * 3
    if 'edge' in terms:
        d = verts.index_select(1, t['e0']) - verts.index_select(1, t['e1'])
        out[0] = (d * d).sum(-1).mean()
    if 'lap' in terms:
        s = torch.zeros_like(verts).index_add_(1, t['rows'], verts.index_select(1, t['cols']))
        delta = torch.where(t['has'], s * t['inv_deg'] - verts, torch.zeros_like(verts))
        out[1] = (delta * delta).sum(-1).mean()
    if 'normal' in terms:
        v0 = verts.index_select(1, t['f0'])
        n = torch.cross(verts.index_select(1, t['f1']) - v0, verts.index_select(1, t['f2']) - v0, dim=-1)
        norm = n.norm(dim=-1).clamp_min(1e-8)
        cos = t['s'] * (n.index_select(1, t['p0']) * n.index_select(1, t['p1'])).sum(-1) / (
            norm.index_select(1, t['p0']) * norm.index_select(1, t['p1']))
        out[2] = (1 - cos).mean()
    return torch.stack(out)


def op_steps(dev, terms):
    verts, faces, _maps, _glob, _rgbs = inputs(dev)
    topo = ops.mesh_topology(faces, verts.shape[1], dev)
    tables = aten_tables(topo, dev)
    v = verts.clone().requires_grad_(True)
    up = torch.tensor([0.3, -2.0, 5.0], device=dev)
    a = vpn_amd.mesh_regularizers(v, faces, 0.0, terms).detach()
    b = aten_regularizers(v, tables, terms).detach()
    assert torch.allclose(a, b, rtol=1e-4, atol=0), (a, b)                   # the two variants compute the same thing
    return {'ATen composition': lambda: torch.autograd.grad((aten_regularizers(v, tables, terms) * up).sum(), [v]),
            'mesh_regularizers': lambda: torch.autograd.grad((vpn_amd.mesh_regularizers(v, faces, 0.0, terms) * up).sum(), [v])}


def model_steps(dev):
    verts, faces, maps, glob, rgbs = inputs(dev)
    torch.manual_seed(1)
    model = GCNModel().to(dev)
    points = (torch.rand(verts.shape[0], verts.shape[1], 3, device=dev) - 0.5) * 0.8
    cd, emd, reg = vpn_amd.ChamferDistanceLoss(), vpn_amd.EarthMoverDistanceLoss(), vpn_amd.MeshRegularizationLoss(0.1, 0.5, 0.01)
    leaves = list(model.parameters())

    def make(with_reg):
        def step():
            meshes = [TriangleMesh(verts[b], faces) for b in range(verts.shape[0])]
            pred = model(meshes, rgbs, maps, glob)
            loss = cd(pred, points) + torch.sqrt(emd(pred, points, 0.005, 50)[0]).mean()
            if with_reg:
                loss = loss + reg(pred, faces)
            return torch.autograd.grad(loss, leaves)
        return step
    return {'Chamfer + EMD': make(False), '+ --mesh-reg': make(True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replays', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'meshreg_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_meshreg.py needs a GPU: nothing is measured on a CPU')
    if args.replays < 50:
        raise SystemExit('at least 50 replays per variant')
    dev = torch.device('cuda:0')
    lines = ['tools/time_meshreg.py --replays %d on one MI355X (torch %s): B = 8, V = 2048 = 16 spheres of 128, F = 4032, E = 6048, '
             '6048 pairs; us, median [10th .. 90th percentile] of %d graph replays, each between two device events, after 20 '
             'warm-up replays; the variants of a row alternate' % (args.replays, torch.__version__, args.replays)]
    rows = [('(a) forward + backward to the vertices, %s' % ('all three terms' if len(t) == 3 else t[0] + ' alone'),
             lambda t=t: op_steps(dev, t)) for t in (TERMS,) + tuple((t,) for t in TERMS)]
    rows.append(('(b) model step of examples/train_gcn_step.py: GCNModel forward, losses, backward to the parameters',
                 lambda: model_steps(dev)))
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
        print('\n'.join(lines[first:]), flush=True)
        del graphs, steps
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
