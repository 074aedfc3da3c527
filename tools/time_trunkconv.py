"""Time the trunk's 3x3 convolutions on one MI355X: vpn_amd.conv3x3 (csrc/trunkconv.hip, f32-input MFMA) against the
library convolution the plain trunk runs (nn.Conv2d: ATen -> MIOpen), one convolution per stage and the whole ResNet-18
trunk in the four combinations of fused_norm x hip_conv, forward + backward in training mode, at B = 8 and B = 64 with
128 x 128 input.  Writes profiles/trunkconv_time.txt.  The ATen rows are the first per-convolution
measurement of this project: until now the convolutions' share of the trunk was a model from shapes and sums.

    python tools/time_trunkconv.py [--replays 200] [--out profiles/trunkconv_time.txt] [--batches 8,64]

What is timed: each variant's forward + backward (y, dx and dw) is captured into a graph once; the graphs of a row are
replayed in turn in the same process, every replay between two device events; reported is the median (10th .. 90th
percentile) of `replays` replays after 20 warm-up replays.  Next to a convolution's time: its 3 x 2 x 9 C^2 B H W flop as a
fraction of the 157.3 TFLOP/s fp32 matrix peak, and the time its weight traffic alone (w read twice, dw written once) would
take at 8 TB/s.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402
from vpn_amd.modules.network import ResNet18, _trunk_maps  # noqa: E402

# (stage, channels, side of the map at 128 x 128 input, convolutions of this shape in the trunk)
SITES = [('layer1', 64, 32, 4), ('layer2', 128, 16, 3), ('layer3', 256, 8, 3), ('layer4', 512, 4, 3)]
PEAK_FLOPS, HBM_BYTES = 157.3e12, 8.0e12


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


def site_steps(C, side, B, dev):
    g = torch.Generator().manual_seed(C + side)
    x = torch.randn(B, C, side, side, generator=g).to(dev).requires_grad_(True)
    w = (torch.randn(C, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(dev).requires_grad_(True)
    dy = torch.randn(B, C, side, side, generator=g).to(dev)

    def aten():
        return torch.autograd.grad(F.conv2d(x, w, None, 1, 1), [x, w], dy)

    def hip():
        return torch.autograd.grad(vpn_amd.conv3x3(x, w), [x, w], dy)
    return {'ATen': aten, 'hip': hip}


def trunk_steps(B, dev):
    torch.manual_seed(0)
    state = ResNet18().state_dict()
    imgs = torch.randn(B, 3, 128, 128, generator=torch.Generator().manual_seed(1)).to(dev)

    def make(**kwargs):
        model = ResNet18(**kwargs)
        model.load_state_dict(state, strict=True)
        model = model.to(dev).train()
        params = [p for n, p in model.named_parameters() if not n.startswith('fc.')]

        def step():
            maps = _trunk_maps(model, imgs)
            return torch.autograd.grad(sum(m.sum() for m in maps), params)
        return step
    return {'plain': make(), 'norm': make(fused_norm=True), 'conv': make(hip_conv=True), 'norm+conv': make(fused_norm=True, hip_conv=True)}


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


def quantiles(steps, replays):
    graphs = {k: capture(s) for k, s in steps.items()}
    t = {k: torch.tensor(v, dtype=torch.float64) * 1e3 for k, v in measure(graphs, replays).items()}
    return {k: [float(torch.quantile(v, p)) for p in (0.5, 0.1, 0.9)] for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replays', type=int, default=200)
    ap.add_argument('--batches', default='8,64')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'trunkconv_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_trunkconv.py needs a GPU: nothing is measured on a CPU')
    if args.replays < 200:
        raise SystemExit('at least 200 replays per variant')
    dev = torch.device('cuda:0')
    ops = vpn_amd.ops
    lines = ['tools/time_trunkconv.py --replays %d on one MI355X (torch %s): us per forward + backward (y, dx, dw), training mode, '
             'median [10th .. 90th percentile] of %d graph replays, each between two device events, after 20 warm-up replays; the '
             'variants of a row alternate.  ATen = nn.Conv2d / F.conv2d (the library, the parent\'s path; these rows are the '
             'project\'s first per-convolution measurement), hip = csrc/trunkconv.hip (tile %d x %d x %d, split target %d, at most '
             '%d slices).  peak: 54 C^2 B H W flop / time / 157.3 TFLOP/s; floor: 3 x 36 C^2 bytes of weight traffic at 8 TB/s.' %
             (args.replays, torch.__version__, args.replays, ops.CONV_TILE, ops.CONV_TILE, ops.CONV_TILE_K, ops.CONV_SPLIT_TARGET,
              ops.CONV_MAX_SPLIT)]
    for B in [int(b) for b in args.batches.split(',')]:
        lines.append('B = %d, 128 x 128 input' % B)
        for stage, C, side, count in SITES:
            q = quantiles(site_steps(C, side, B, dev), args.replays)
            flop = 3 * 2 * 9 * C * C * B * side * side
            floor_us = 3 * 36 * C * C / HBM_BYTES * 1e6
            S = [ops.conv3x3_splits(B, C, C, side, side, p) for p in (ops.CONV_FWD, ops.CONV_DX, ops.CONV_DW)]
            lines.append('  %s conv (C=%d, %dx%d, x%d in the trunk; slices fwd/dx/dw %d/%d/%d)  ATen %8.1f us [%8.1f .. %8.1f] %4.1f %% of peak   '
                         'hip %8.1f us [%8.1f .. %8.1f] %4.1f %% of peak   ATen / hip %5.2f   weight floor %5.2f us' %
                         (stage, C, side, side, count, *S, *q['ATen'], 100 * flop / (q['ATen'][0] * 1e-6) / PEAK_FLOPS,
                          *q['hip'], 100 * flop / (q['hip'][0] * 1e-6) / PEAK_FLOPS, q['ATen'][0] / q['hip'][0], floor_us))
            print(lines[-1], flush=True)
        q = quantiles(trunk_steps(B, dev), args.replays)
        for k, label in (('plain', 'whole trunk, plain (ATen norms, ATen convolutions)'), ('norm', 'whole trunk, fused_norm'),
                         ('conv', 'whole trunk, hip_conv'), ('norm+conv', 'whole trunk, fused_norm + hip_conv')):
            lines.append('  %-52s %8.1f us [%8.1f .. %8.1f]   plain / this %5.2f' % (label, *q[k], q['plain'][0] / q[k][0]))
            print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
