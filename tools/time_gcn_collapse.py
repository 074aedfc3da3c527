"""Time the GCN's collapsed layer pairs (GCNModel(collapse_pairs=True), ops.gcn_aggregate2, ops.gcn_project, csrc/gcnpair.hip;
DESIGN.md 4.24) against what they replace on one MI355X, at the reference shape: B = 8, N = 16 x 128 (a block a sphere).
Writes profiles/gcn_collapse_time.txt.

    python tools/time_gcn_collapse.py [--replays 50] [--out profiles/gcn_collapse_time.txt]

  (a) gcn_aggregate2 against two launches of the one-hop op (GcnAggregateFunction twice) at C = 512 and C = 3, with u, bias
      and the ReLU, forward alone and forward + backward (h, u and bias needing their gradients);
  (b) gcn_project against torch.matmul at [16384, 512] x [512, 3], forward alone and forward + backward;
  (c) the whole GCNModel forward + backward for {plain, factored input} x {pairs in a row, collapsed}, with gradients to the
      parameters alone (train_gcn.py: the VPN is frozen) and to every input.

Each variant is captured into a graph once; the graphs of a row are replayed in turn in the same process, every replay
between two device events; reported is the median (10th .. 90th percentile) of `replays` replays after 20 warm-up replays.
There is no speed bar: the numbers are reported, not asserted.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402, F401
from vpn_amd import ops  # noqa: E402
from vpn_amd.modules.gcn import GCNModel  # noqa: E402
from vpn_amd.modules.meshing import TriangleMesh  # noqa: E402
from time_gcn_factored import inputs  # noqa: E402
from time_trunknorm import capture, measure  # noqa: E402


def _fwd(f):
    def step():
        with torch.no_grad():
            return f()
    return step


def aggregate_steps(dev, C):
    verts, faces, _maps, _glob, _rgbs = inputs(dev)
    B, N = verts.shape[:2]
    graph, blocks = ops.gcn_graph(faces, N, dev), ops.gcn_blocks(faces, N, dev)
    assert blocks is not None and blocks.numel() == 17
    gen = torch.Generator().manual_seed(C)
    h = torch.randn(B, N, C, generator=gen).to(dev).requires_grad_(True)
    u = torch.randn(C, generator=gen).to(dev).requires_grad_(True)
    b = torch.randn(C, generator=gen).to(dev).requires_grad_(True)
    dy = torch.randn(B, N, C, generator=gen).to(dev)

    def one_hop_twice():
        t = ops.GcnAggregateFunction.apply(h, u, graph.row_ptr, graph.col, graph.w, False)
        return ops.GcnAggregateFunction.apply(t, b, graph.row_ptr, graph.col, graph.w, True)

    def two_hop():
        return ops.gcn_aggregate2(h, u, b, graph, blocks, relu=True)

    forms = {'one-hop x 2': one_hop_twice, 'aggregate2': two_hop}
    return ({k: _fwd(f) for k, f in forms.items()},
            {k: (lambda f=f: torch.autograd.grad(f(), [h, u, b], dy)) for k, f in forms.items()})


def project_steps(dev, R=16384, Ci=512, Co=3):
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(R, Ci, generator=gen).to(dev).requires_grad_(True)
    th = (torch.randn(Ci, Co, generator=gen) * 0.05).to(dev).requires_grad_(True)
    g = torch.randn(R, Co, generator=gen).to(dev)
    forms = {'torch.matmul': lambda: torch.matmul(x, th), 'gcn_project': lambda: ops.gcn_project(x, th)}
    return ({k: _fwd(f) for k, f in forms.items()},
            {k: (lambda f=f: torch.autograd.grad(f(), [x, th], g)) for k, f in forms.items()})


def model_steps(dev, frozen):
    verts, faces, maps, glob, rgbs = inputs(dev)
    torch.manual_seed(1)
    models = {}
    for factored in (False, True):
        for collapse in (False, True):
            name = ('factored' if factored else 'plain') + (', collapsed' if collapse else '')
            models[name] = GCNModel(factored_input=factored, collapse_pairs=collapse).to(dev)
            models[name].load_state_dict(models['plain'].state_dict())
    v = verts.clone().requires_grad_(not frozen)
    g = glob.clone().requires_grad_(not frozen)
    mp = [m.clone().requires_grad_(not frozen) for m in maps]

    def make(model):
        leaves = list(model.parameters()) + ([] if frozen else [v, g] + mp)

        def step():                                  # the meshes are views of v: made in the step, so that no autograd graph outlives it
            meshes = [TriangleMesh(v[b], faces) for b in range(v.shape[0])]
            return torch.autograd.grad(model(meshes, rgbs, mp, g).square().mean(), leaves)
        return step
    return {k: make(m) for k, m in models.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replays', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'gcn_collapse_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_gcn_collapse.py needs a GPU: nothing is measured on a CPU')
    if args.replays < 50:
        raise SystemExit('at least 50 replays per variant')
    dev = torch.device('cuda:0')
    lines = ['tools/time_gcn_collapse.py --replays %d on one MI355X (torch %s): B = 8, N = 2048 = 16 blocks of 128, maps 64@32^2 '
             '128@16^2 256@8^2 512@4^2, G = 512; us, median [10th .. 90th percentile] of %d graph replays, each between two '
             'device events, after 20 warm-up replays; the variants of a row alternate'
             % (args.replays, torch.__version__, args.replays)]
    rows = []
    for C in (512, 3):
        f, fb = aggregate_steps(dev, C)
        rows.append(('(a) A(A h + u) + b, ReLU, C = %d, forward' % C, f))
        rows.append(('(a) A(A h + u) + b, ReLU, C = %d, forward + backward (h, u, b)' % C, fb))
    f, fb = project_steps(dev)
    rows.append(('(b) [16384, 512] x [512, 3], forward', f))
    rows.append(('(b) [16384, 512] x [512, 3], forward + backward (x, theta)', fb))
    rows.append(('(c) GCNModel forward + backward, parameters only (frozen VPN)', lambda: model_steps(dev, True)))
    rows.append(('(c) GCNModel forward + backward, every input needs its gradient', lambda: model_steps(dev, False)))
    for label, steps in rows:
        if callable(steps):
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
