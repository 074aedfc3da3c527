"""Time the trunk's tail on one MI355X: vpn_amd.batch_norm_act_mean (the tt_ kernels of csrc/trunknorm.hip), the last norm /
add / ReLU site of the ResNet-18 trunk with the global average pool, against the ATen composition the plain trunk runs
(nn.BatchNorm2d, add, in-place ReLU, nn.AdaptiveAvgPool2d) and against vpn_amd.batch_norm_act followed by ATen's pool, which
is what ResNet18(fused_norm=True) runs; then the whole ResNet-18 trunk plus pool with fused_norm, with and without
fused_tail.  Forward + backward in training mode, at B = 8 and B = 64 with 128 x 128 input (layer4 is [B, 512, 4, 4]); the map
and the features both have an upstream gradient (the GCN's case).  Writes profiles/trunktail_time.txt.

    python tools/time_trunktail.py [--replays 200] [--out profiles/trunktail_time.txt]

The method is that of tools/time_trunkpool.py: each variant's forward + backward is captured into a graph once; the graphs
of a row are replayed in turn in the same process, every replay between two device events; reported is the median (10th ..
90th percentile) of `replays` replays after 20 warm-up replays.  The site is the tail alone (no convolution): its input,
residual and upstream gradients stay allocated.  There is no speed bar: the numbers are reported, not asserted.  No GPU: the
script fails, it measures nothing on a CPU."""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402
from vpn_amd.modules.network import ResNet18, _trunk_features  # noqa: E402
from time_trunknorm import capture, measure  # noqa: E402


def site_steps(B, dev, C=512, side=4):
    g = torch.Generator().manual_seed(C + side)
    x = torch.randn(B, C, side, side, generator=g).to(dev).requires_grad_(True)
    res = torch.randn(B, C, side, side, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(B, C, side, side, generator=g).to(dev)
    dm = torch.randn(B, C, generator=g).to(dev)
    bns = [nn.BatchNorm2d(C).to(dev).train() for _ in range(3)]
    relu, pool = nn.ReLU(inplace=True), nn.AdaptiveAvgPool2d((1, 1))

    def grads(y, m, bn):
        return torch.autograd.grad([y, m], [x, res] + list(bn.parameters()), [dy, dm])

    def aten():
        y = relu(bns[0](x) + res)
        return grads(y, torch.flatten(pool(y), 1), bns[0])

    def norm():
        y = vpn_amd.batch_norm_act(x, bns[1], residual=res, relu=True)
        return grads(y, torch.flatten(pool(y), 1), bns[1])

    def fused():
        y, m = vpn_amd.batch_norm_act_mean(x, bns[2], residual=res, relu=True)
        return grads(y, m, bns[2])
    return {'ATen': aten, 'norm+ATen pool': norm, 'fused': fused}


def trunk_steps(B, dev):
    torch.manual_seed(0)
    norm = ResNet18(fused_norm=True).to(dev).train()
    tail = ResNet18(fused_norm=True, fused_tail=True).to(dev).train()
    tail.load_state_dict(norm.state_dict(), strict=True)
    imgs = torch.randn(B, 3, 128, 128, generator=torch.Generator().manual_seed(1)).to(dev)

    def make(model):
        params = [p for n, p in model.named_parameters() if not n.startswith('fc.')]

        def step():
            maps, feats = _trunk_features(model, imgs)
            return torch.autograd.grad(sum(m.sum() for m in maps) + feats.sum(), params)
        return step
    return {'fused_norm': make(norm), 'fused_norm+fused_tail': make(tail)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replays', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'trunktail_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_trunktail.py needs a GPU: nothing is measured on a CPU')
    if args.replays < 200:
        raise SystemExit('at least 200 replays per variant')
    dev = torch.device('cuda:0')
    lines = ['tools/time_trunktail.py --replays %d on one MI355X (torch %s): us per forward + backward, training mode, median '
             '[10th .. 90th percentile] of %d graph replays, each between two device events, after 20 warm-up replays; the '
             'variants of a row alternate' % (args.replays, torch.__version__, args.replays)]
    for B in (8, 64):
        lines.append('B = %d, 128 x 128 input' % B)
        for label, steps in (('layer4.1 bn2+add+relu+avgpool (C=512, N=%d)' % (B * 4 * 4), site_steps(B, dev)),
                             ('whole trunk, conv1 .. avgpool', trunk_steps(B, dev))):
            graphs = {k: capture(v) for k, v in steps.items()}
            t = {k: torch.tensor(v, dtype=torch.float64) * 1e3 for k, v in measure(graphs, args.replays).items()}
            q = {k: [float(torch.quantile(v, p)) for p in (0.5, 0.1, 0.9)] for k, v in t.items()}
            lines.append('  ' + label)
            for k in graphs:
                lines.append('    %-24s %8.1f us [%8.1f .. %8.1f]' % (k, *q[k]))
            names = list(graphs)
            lines.append('    %s / %s %5.2f' % (names[-2], names[-1], q[names[-2]][0] / q[names[-1]][0]))
            print('\n'.join(lines[-len(graphs) - 2:]), flush=True)
            del graphs
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
