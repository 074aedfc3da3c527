"""Time conv1 of the GCN in factored form (GCNModel(factored_input=True), ops.GcnFactoredInputFunction, the gcn_factored_
kernels of csrc/gcn.hip) against the plain path on one MI355X, at the reference shape: B = 8, N = 16 x 128,
maps 64@32^2, 128@16^2, 256@8^2, 512@4^2, G = 512, conv1.weight [1511, 512].  Writes profiles/gcn_factored_time.txt.

    python tools/time_gcn_factored.py [--replays 50] [--out profiles/gcn_factored_time.txt]

  (a) conv1's input and x Theta: GcnInputFunction + torch.matmul against GcnFactoredInputFunction, forward alone and forward
      + backward with every input needing its gradient;
  (b) the same with the maps and the global features needing none (train_gcn.py: the VPN is frozen);
  (c) the whole GCNModel forward + backward, plain against factored, with every input needing its gradient and with the
      parameters alone.

Each variant is captured into a graph once; the graphs of a row are replayed in turn in the same process, every replay
between two device events; reported is the median (10th .. 90th percentile) of `replays` replays after 20 warm-up replays.
Then the library's own per-launch events over eager forward + backward runs of either form give the time of every kernel
it launches.  There is no speed bar: the numbers are reported, not asserted.  No GPU: the script fails, it measures nothing
on a CPU."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402
from vpn_amd import ops, _lib  # noqa: E402
from vpn_amd.modules.gcn import GCNModel  # noqa: E402
from vpn_amd.modules.meshing import TriangleMesh, uv_sphere  # noqa: E402
from time_trunknorm import capture, measure  # noqa: E402

MAPS = [(64, 32), (128, 16), (256, 8), (512, 4)]


def inputs(dev, B=8, K=16, G=512):
    torch.manual_seed(0)
    sv, sf = uv_sphere()
    verts = torch.cat([sv[None] * (torch.rand(B, 1, 3) * 0.2 + 0.1) + (torch.rand(B, 1, 3) - 0.5) * 0.6 for _ in range(K)], 1).to(dev)
    faces = torch.cat([sf + sv.shape[0] * k for k in range(K)]).to(dev)
    maps = [torch.randn(B, c, s, s, device=dev) for c, s in MAPS]
    glob = torch.randn(B, G, device=dev)
    rgbs = torch.zeros(B, 3, 128, 128, device=dev)
    rgbs[:, :, 20:100, 12:116] = torch.rand(B, 3, 80, 104, device=dev)
    return verts, faces, maps, glob, rgbs


def op_steps(dev, frozen):
    """{'plain' | 'factored'} x {forward, forward + backward}: frozen -> the maps and the global features need no gradient."""
    verts, _faces, maps, glob, rgbs = inputs(dev)
    bounds = ops.gcn_bounds(rgbs)
    ctot = 39 + sum(c for c, _ in MAPS) + glob.shape[1]
    weight = ((torch.rand(ctot, 512, device=dev) * 2 - 1) * (6.0 / (ctot + 512)) ** 0.5).requires_grad_(True)
    dh = torch.randn(verts.shape[0], verts.shape[1], 512, device=dev)
    v = verts.clone().requires_grad_(True)
    g = glob.clone().requires_grad_(not frozen)
    mp = [m.clone().requires_grad_(not frozen) for m in maps]
    leaves = [v, weight] + ([] if frozen else [g] + mp)

    def plain():
        return torch.matmul(ops.GcnInputFunction.apply(v, bounds, g, 39, *mp), weight)

    def factored():
        return ops.GcnFactoredInputFunction.apply(v, bounds, g, weight, 39, *mp)

    def fwd(f):
        def step():
            with torch.no_grad():
                return f()
        return step

    def fwd_bwd(f):
        return lambda: torch.autograd.grad(f(), leaves, dh)
    return {'plain': fwd(plain), 'factored': fwd(factored)}, {'plain': fwd_bwd(plain), 'factored': fwd_bwd(factored)}


def model_steps(dev, frozen):
    verts, faces, maps, glob, rgbs = inputs(dev)
    torch.manual_seed(1)
    plain = GCNModel().to(dev)
    fact = GCNModel(factored_input=True).to(dev)
    fact.load_state_dict(plain.state_dict())
    v = verts.clone().requires_grad_(not frozen)
    g = glob.clone().requires_grad_(not frozen)
    mp = [m.clone().requires_grad_(not frozen) for m in maps]

    def make(model):
        leaves = list(model.parameters()) + ([] if frozen else [v, g] + mp)

        def step():                                  # the meshes are views of v: made in the step, so that no autograd graph outlives it
            meshes = [TriangleMesh(v[b], faces) for b in range(v.shape[0])]
            return torch.autograd.grad(model(meshes, rgbs, mp, g).square().mean(), leaves)
        return step
    return {'plain': make(plain), 'factored': make(fact)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replays', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'gcn_factored_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_gcn_factored.py needs a GPU: nothing is measured on a CPU')
    if args.replays < 50:
        raise SystemExit('at least 50 replays per variant')
    dev = torch.device('cuda:0')
    lines = ['tools/time_gcn_factored.py --replays %d on one MI355X (torch %s): B = 8, N = 2048, maps 64@32^2 128@16^2 256@8^2 '
             '512@4^2, G = 512, conv1.weight [1511, 512]; us, median [10th .. 90th percentile] of %d graph replays, each between '
             'two device events, after 20 warm-up replays; the two variants of a row alternate'
             % (args.replays, torch.__version__, args.replays)]
    rows = []
    profiled = None
    for frozen, tag in ((False, 'every input needs its gradient'), (True, 'maps and global features need none (frozen VPN)')):
        f, fb = op_steps(dev, frozen)
        if not frozen:
            rows.append(('(a) conv1 input + x Theta, forward', f))
            profiled = fb
        rows.append(('(%s) conv1 input + x Theta, forward + backward, %s' % ('b' if frozen else 'a', tag), fb))
    rows.append(('(c) GCNModel forward + backward, every input needs its gradient', model_steps(dev, False)))
    rows.append(('(c) GCNModel forward + backward, parameters only (frozen VPN)', model_steps(dev, True)))
    for label, steps in rows:
        graphs = {k: capture(v) for k, v in steps.items()}
        t = {k: torch.tensor(v, dtype=torch.float64) * 1e3 for k, v in measure(graphs, args.replays).items()}
        q = {k: [float(torch.quantile(v, p)) for p in (0.5, 0.1, 0.9)] for k, v in t.items()}
        lines.append(label)
        for k in graphs:
            lines.append('    %-10s %8.1f us [%8.1f .. %8.1f]' % (k, *q[k]))
        lines.append('    plain / factored %5.2f' % (q['plain'][0] / q['factored'][0]))
        print('\n'.join(lines[-4:]), flush=True)
        del graphs
    # ---- the library's kernels in one forward + backward of either form, eager, every input needing its gradient
    for name, step in profiled.items():
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        with _lib.KernelProfile() as kp:
            for _ in range(args.replays):
                step()
            torch.cuda.synchronize()
        first = len(lines)
        lines.append('kernels of one %s forward + backward (the library\'s per-launch events, mean of %d eager runs; the dense '
                     'products of torch.matmul are not listed)' % (name, args.replays))
        total = 0.0
        for k, (c, ms) in sorted(kp.summary().items()):
            lines.append('    %-34s %3d launches a run  %8.1f us each' % (k, c // args.replays, ms * 1e3))
            total += c * ms * 1e3 / args.replays
        lines.append('    sum %8.1f us a run' % total)
        print('\n'.join(lines[first:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
