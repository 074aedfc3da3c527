"""Time the trunk's norm / add / ReLU op on one MI355X: vpn_amd.batch_norm_act (csrc/trunknorm.hip) against the ATen
composition the plain trunk runs (nn.BatchNorm2d, `+ identity`, in-place ReLU), per site and for the whole ResNet-18 trunk,
forward + backward in training mode, at B = 8 and B = 64 with 128 x 128 input.  Writes profiles/trunknorm_time.txt
(DESIGN.md 4.18).

    python tools/time_trunknorm.py [--replays 200] [--out profiles/trunknorm_time.txt]

What is timed: each variant's forward + backward is captured into a graph once; the two graphs of a site are replayed in
turn in the same process, every replay between two device events; reported is the median (10th .. 90th percentile) of
`replays` replays after 20 warm-up replays.  A site is the norm ring alone (no convolution): its input, residual and
upstream gradient stay allocated.  The whole trunk includes the convolutions and the max-pool, which are the same library
calls in both variants.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402
from vpn_amd.modules.network import ResNet18, _trunk_maps  # noqa: E402

# (name, channels, side of the map at 128 x 128 input, residual): the stem and one `bn2 -> += identity -> relu` per stage
SITES = [('stem bn1+relu', 64, 64, False), ('layer1 bn2+add+relu', 64, 32, True), ('layer2 bn2+add+relu', 128, 16, True),
         ('layer3 bn2+add+relu', 256, 8, True), ('layer4 bn2+add+relu', 512, 4, True)]


def capture(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph


def site_steps(C, side, residual, B, dev):
    g = torch.Generator().manual_seed(C + side)
    x = torch.randn(B, C, side, side, generator=g).to(dev).requires_grad_(True)
    res = torch.randn(B, C, side, side, generator=g).to(dev).requires_grad_(True) if residual else None
    dy = torch.randn(B, C, side, side, generator=g).to(dev)
    leaves = [x] + ([res] if residual else [])
    bn_a, bn_f = nn.BatchNorm2d(C).to(dev).train(), nn.BatchNorm2d(C).to(dev).train()
    relu = nn.ReLU(inplace=True)

    def aten():
        out = bn_a(x)
        if residual:
            out = out + res
        out = relu(out)
        return torch.autograd.grad(out, leaves + list(bn_a.parameters()), dy)

    def fused():
        out = vpn_amd.batch_norm_act(x, bn_f, residual=res, relu=True)
        return torch.autograd.grad(out, leaves + list(bn_f.parameters()), dy)
    return aten, fused


def trunk_steps(B, dev):
    torch.manual_seed(0)
    plain = ResNet18().to(dev).train()
    fused = ResNet18(fused_norm=True).to(dev).train()
    fused.load_state_dict(plain.state_dict(), strict=True)
    imgs = torch.randn(B, 3, 128, 128, generator=torch.Generator().manual_seed(1)).to(dev)

    def make(model):
        params = [p for n, p in model.named_parameters() if not n.startswith('fc.')]

        def step():
            maps = _trunk_maps(model, imgs)
            return torch.autograd.grad(sum(m.sum() for m in maps), params)
        return step
    return make(plain), make(fused)


def measure(graphs, replays, warm=20):
    for _ in range(warm):
        for gr in graphs.values():
            gr.replay()
    torch.cuda.synchronize()
    samples = {k: [] for k in graphs}
    for _ in range(replays):
        for name, gr in graphs.items():                                  # the variants alternate
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gr.replay()
            b.record()
            b.synchronize()
            samples[name].append(a.elapsed_time(b))
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replays', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'trunknorm_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_trunknorm.py needs a GPU: nothing is measured on a CPU')
    if args.replays < 200:
        raise SystemExit('at least 200 replays per variant')
    dev = torch.device('cuda:0')
    lines = ['tools/time_trunknorm.py --replays %d on one MI355X (torch %s): us per forward + backward, training mode, median '
             '[10th .. 90th percentile] of %d graph replays, each between two device events, after 20 warm-up replays; the two '
             'variants of a row alternate; one-launch limit N <= %d' %
             (args.replays, torch.__version__, args.replays, vpn_amd.ops.TRUNKNORM_ONE_PASS_MAX)]
    for B in (8, 64):
        lines.append('B = %d, 128 x 128 input' % B)
        rows = [(name + ' (C=%d, N=%d)' % (C, B * side * side), site_steps(C, side, residual, B, dev))
                for name, C, side, residual in SITES]
        rows.append(('whole trunk, conv1 .. layer4', trunk_steps(B, dev)))
        for label, (aten, fused) in rows:
            graphs = {'ATen': capture(aten), 'hip': capture(fused)}
            t = {k: torch.tensor(v, dtype=torch.float64) * 1e3 for k, v in measure(graphs, args.replays).items()}
            q = {k: [float(torch.quantile(v, p)) for p in (0.5, 0.1, 0.9)] for k, v in t.items()}
            lines.append('  %-38s ATen %8.1f us [%8.1f .. %8.1f]   hip %8.1f us [%8.1f .. %8.1f]   ATen / hip %5.2f' %
                         (label, *q['ATen'], *q['hip'], q['ATen'][0] / q['hip'][0]))
            print(lines[-1], flush=True)
            del graphs
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
