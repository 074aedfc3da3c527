"""Time the occupancy loss (ops.primitive_occupancy_loss, csrc/occloss.hip) on one MI355X: B = 8 and B = 64
samples, K = 16 primitives of alternating kinds, Q = 32^3 grid queries and Q = 4096 drawn ones, uint8 labels, tau = 0.05.
Writes profiles/occloss_time.txt.

    python tools/time_occloss.py [--rounds 50] [--out profiles/occloss_time.txt]

Variants, on the same inputs:
  fused fwd, eager / replay        the two launches of vpn_occloss_fwd (lse and s are written: params needs a gradient);
  fused fwd+bwd, eager / replay    and the two of vpn_occloss_bwd, through autograd;
  composed fwd / fwd+bwd, eager    the same loss from torch ops in fp32 ([B,chunk,K,3] temporaries in query chunks that keep a
                                   chunk's tensors near 1 GB; the backward per chunk, so that the saved tensors stay as small);
  train step, without / with       the step of examples/train_step.py (stand-in network, batch 8, 16 primitives, torch Adam)
                                   without and with --occupancy-loss 1,0.1: forward, backward and the optimiser.
The eager variants are timed with the host clock around the call and a device synchronise, the replays between two device
events.  The variants alternate within every round; reported is the median [10th .. 90th percentile] of `rounds` rounds after 5
warm-up rounds; the composed variants run in every `--composed-every`-th round only.  Before timing, the fused and the composed
loss must agree to 1e-4 on the two values and on the gradient.  There is no speed bar; the expectation that is stated and checked
in the output is that the fused op is not slower than the composed one by more than the spread (90th - 10th percentile) of the
replays of the same run.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))
import vpn_amd  # noqa: E402
from vpn_amd import ops  # noqa: E402
from time_trunknorm import capture  # noqa: E402

K, TAU = 16, 0.05
ELEMENT_BUDGET = 2.5e8                  # fp32 elements of one [B,chunk,K,3] temporary of the composed loss: 1 GB


def make_inputs(B, Q, dev):
    g = torch.Generator().manual_seed(31 + B + Q)
    params = torch.cat([torch.rand(B, K, 3, generator=g) * 0.15 + 0.08, torch.randn(B, K, 3, generator=g), torch.rand(B, K, 1, generator=g),
                        (torch.rand(B, K, 3, generator=g) - 0.5) * 0.5], 2).float().to(dev).contiguous()
    kinds = [k % 2 for k in range(K)]
    queries = ops.grid_queries(32, device=dev) if Q == 32 ** 3 else (torch.rand(Q, 3, generator=g) - 0.5).to(dev)
    target = params.clone()
    target[:, :, 7:10] += 0.05
    return params, kinds, queries, ops.primitive_occupancy(target, kinds, queries)


def rotations(q):
    """make_pose of csrc/vpn_common.h from torch ops: q [...,4] -> R [...,3,3]."""
    h = ((q[..., 3] - torch.floor(q[..., 3])) * 2 * math.pi) / 2
    r = torch.cat([q[..., :3] * torch.sin(h)[..., None], torch.cos(h)[..., None]], -1)
    x, y, z, w = (r / r.norm(dim=-1, keepdim=True)).unbind(-1)
    return torch.stack([torch.stack([x * x - y * y - z * z + w * w, 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                        torch.stack([2 * (x * y + z * w), -x * x + y * y - z * z + w * w, 2 * (y * z - x * w)], -1),
                        torch.stack([2 * (x * z - y * w), 2 * (y * z + x * w), -x * x - y * y + z * z + w * w], -1)], -2)


def composed(params, sphere, queries, labels, up, backward):
    """out [2] of the loss from torch ops, in query chunks; backward: the gradient of (out * up).sum() is accumulated in params.grad."""
    B, Q = labels.shape
    chunk = max(1, int(ELEMENT_BUDGET // (B * K * 3)))
    total = torch.zeros(2, device=params.device)
    for s0 in range(0, Q, chunk):
        v, t, R = params[:, :, 0:3], params[:, :, 7:10], rotations(params[:, :, 3:7])
        d = queries[None, s0:s0 + chunk, None, :] - t[:, None]                              # [B,c,K,3]
        y = torch.einsum('bkji,bckj->bcki', R, d) / v[:, None]
        m = torch.where(sphere[None, None, :], (y * y).sum(-1), y.abs().amax(-1))
        z = (1 - m) / TAU
        l = torch.logsumexp(z, -1)
        lab = labels[:, s0:s0 + chunk].float()
        bce = (l.clamp(min=0) + torch.log1p(torch.exp(-l.abs()))) - lab * l
        ov = torch.relu(torch.sigmoid(z).sum(-1) - 1) ** 2
        part = torch.stack([bce.sum(), ov.sum()]) / (B * Q)
        if backward:
            (part * up).sum().backward()
        total = total + part.detach()
    return total


def train_steps(dev):
    """(step without the flag, step with --occupancy-loss 1,0.1) of examples/train_step.py at its default sizes."""
    import train_step as T
    B, prims, n, size = 8, 16, 128, 128
    batch = T.make_batch(B, prims, n, size, dev)
    occupancy = (vpn_amd.OccupancyLoss(1.0, 0.1),) + T.occupancy_queries(batch[1], T.target_assembly(B, prims, dev), batch[7])
    weights = (1.0, 1.0, 1.0, 0.1, 1.0)

    def make(extra):
        torch.manual_seed(1234)
        net = T.Heads(64, prims).to(dev)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        it = [0]

        def step():
            opt.zero_grad()
            total, _ = T.training_losses(net, *batch, n, weights, seed=1000 + it[0], **extra)
            total.backward()
            opt.step()
            it[0] += 1
        return step
    return make({}), make({'occupancy': occupancy})


def host_timed(step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def replay_timed(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def measure(variants, rounds, composed_every):
    samples = {k: [] for k in variants}
    for r in range(5 + rounds):
        for k, v in variants.items():
            if k.startswith('composed') and r % composed_every:
                continue
            t = v()
            if r >= 5:
                samples[k].append(t)
    return {k: [float(torch.quantile(torch.tensor(v, dtype=torch.float64), p)) for p in (0.5, 0.1, 0.9)] + [len(v)] for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=50)
    ap.add_argument('--composed-every', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'occloss_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_occloss.py needs a GPU: nothing is measured on a CPU')
    if args.rounds < 20:
        raise SystemExit('at least 20 rounds')
    dev = torch.device('cuda:0')
    lines = ['tools/time_occloss.py --rounds %d --composed-every %d on one MI355X (torch %s): the occupancy loss of B samples, K = %d, Q '
             'queries, uint8 labels, tau = %g; us, median [10th .. 90th percentile] of %d rounds after 5 warm-up rounds (the composed variants '
             'in every %dth round); the variants alternate within a round; eager: host clock around the call and a device synchronise; '
             'replay: two device events' % (args.rounds, args.composed_every, torch.__version__, K, TAU, args.rounds, args.composed_every)]
    up = torch.tensor([1.0, 0.1], device=dev)
    for Q in (32 ** 3, 4096):
        for B in (8, 64):
            params, kinds, queries, labels = make_inputs(B, Q, dev)
            kt = ops.kinds_tensor(kinds, dev)
            sphere = kt == vpn_amd.SPHERE
            p = params.clone().requires_grad_(True)

            def fwd():
                return ops.primitive_occupancy_loss(p, kt, queries, labels, TAU)

            def fwd_bwd():
                out = ops.primitive_occupancy_loss(p, kt, queries, labels, TAU)
                return out.detach(), torch.autograd.grad((out * up).sum(), [p])[0]

            pc = params.clone().requires_grad_(True)

            def composed_fwd():
                with torch.no_grad():
                    return composed(pc, sphere, queries, labels, up, False)

            def composed_fwd_bwd():
                pc.grad = None
                return composed(pc, sphere, queries, labels, up, True), pc.grad

            (out_f, grad_f), (out_c, grad_c) = fwd_bwd(), composed_fwd_bwd()
            e_out = float(((out_f - out_c).abs() / (1 + out_c.abs())).max())
            e_grad = float((grad_f - grad_c).abs().max() / grad_c.abs().max())
            if not (e_out <= 1e-4 and e_grad <= 1e-4):
                raise SystemExit('B = %d, Q = %d: the fused and the composed loss disagree: values %.2e, gradient %.2e' % (B, Q, e_out, e_grad))
            g_fwd, g_both = capture(fwd), capture(fwd_bwd)
            variants = {'fused fwd, eager': lambda: host_timed(fwd), 'fused fwd, replay': lambda: replay_timed(g_fwd),
                        'fused fwd+bwd, eager': lambda: host_timed(fwd_bwd), 'fused fwd+bwd, replay': lambda: replay_timed(g_both),
                        'composed fwd, eager': lambda: host_timed(composed_fwd), 'composed fwd+bwd, eager': lambda: host_timed(composed_fwd_bwd)}
            qs = measure(variants, args.rounds, args.composed_every)
            first = len(lines)
            slices, per = ops.occloss_plan(B, Q)
            lines.append('B = %d, Q = %d (backward: %d slices of %d queries; fused against composed: values %.1e, gradient %.1e)'
                         % (B, Q, slices, per, e_out, e_grad))
            for k in variants:
                lines.append('    %-26s %11.1f us [%11.1f .. %11.1f]  (%d samples)' % (k, *qs[k]))
            pairs = B * Q * K
            lines.append('    %d x %d x %d = %.3g (query, primitive) pairs: %.1f G pairs/s forward, %.1f G pairs/s forward + backward (replays)'
                         % (B, Q, K, pairs, pairs / qs['fused fwd, replay'][0] / 1e3, pairs / qs['fused fwd+bwd, replay'][0] / 1e3))
            for a in ('fwd', 'fwd+bwd'):
                spread = qs['fused %s, replay' % a][2] - qs['fused %s, replay' % a][1]
                ok = qs['fused %s, eager' % a][0] <= qs['composed %s, eager' % a][0] + spread
                lines.append('    expectation (fused %s, eager <= composed %s, eager + %.1f us, the spread of the replays): %s; the composed loss '
                             'takes %.2f x the eager op, %.2f x the replay'
                             % (a, a, spread, 'holds' if ok else 'DOES NOT HOLD', qs['composed %s, eager' % a][0] / qs['fused %s, eager' % a][0],
                                qs['composed %s, eager' % a][0] / qs['fused %s, replay' % a][0]))
            print('\n'.join(lines[first:]), flush=True)
            del g_fwd, g_both
    without, with_flag = train_steps(dev)
    qs = measure({'train step, without': lambda: host_timed(without), 'train step, with': lambda: host_timed(with_flag)}, args.rounds, 1)
    first = len(lines)
    lines.append('examples/train_step.py (stand-in network, batch 8, 16 primitives, 128 points a primitive, 128 x 128 silhouettes, torch Adam; '
                 'with: --occupancy-loss 1,0.1 on 16^3 + 2048 queries a sample)')
    for k in qs:
        lines.append('    %-26s %11.1f us [%11.1f .. %11.1f]  (%d samples)' % (k, *qs[k]))
    lines.append('    the flag adds %.1f us to the step (%.1f %%)' % (qs['train step, with'][0] - qs['train step, without'][0],
                                                                      100 * (qs['train step, with'][0] / qs['train step, without'][0] - 1)))
    print('\n'.join(lines[first:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
