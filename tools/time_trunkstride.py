"""Time the trunk's strided convolutions on one MI355X: vpn_amd.conv2d (csrc/trunkstride.hip, f32-input MFMA) against the
library convolution the plain trunk runs (F.conv2d: ATen -> MIOpen) at each of the seven stride-2 sites of the ResNet-18
trunk, and the whole trunk plain, with fused_norm, with fused_norm + hip_conv and with fused_norm + hip_conv +
hip_conv_strided, forward + backward in training mode, at B = 8 and B = 64 with 128 x 128 input.  Writes
profiles/trunkstride_time.txt.  There is no speed bar: the figures are what the guarantee (exact fp32
products, one summation order, bit-equal runs) costs.

    python tools/time_trunkstride.py [--replays 200] [--out profiles/trunkstride_time.txt] [--batches 8,64]

The method is tools/time_trunkconv.py's: each variant's forward + backward is captured into a graph once; the graphs of a
row are replayed in turn in the same process, every replay between two device events; reported is the median (10th .. 90th
percentile) of `replays` replays after 20 warm-up replays.  The stem is timed as the trunk runs it: its input needs no
gradient, so its backward is the weight gradient alone (both variants).  No GPU: the script fails, it measures nothing on a
CPU."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402
from vpn_amd.modules.network import ResNet18, _trunk_maps  # noqa: E402
from time_trunkconv import quantiles  # noqa: E402

# (site, C_in, C_out, side of its input at 128 x 128, kernel, stride, padding, the input needs a gradient)
SITES = [('conv1', 3, 64, 128, 7, 2, 3, False)]
for _i, _c in enumerate((64, 128, 256)):
    SITES += [('layer%d.0.conv1' % (_i + 2), _c, 2 * _c, 32 >> _i, 3, 2, 1, True),
              ('layer%d.0.downsample.0' % (_i + 2), _c, 2 * _c, 32 >> _i, 1, 2, 0, True)]
PEAK_FLOPS = 157.3e12


def site_steps(Ci, Co, side, k, st, p, need_x, B, dev):
    g = torch.Generator().manual_seed(Ci + Co + side + k)
    out = (side + 2 * p - k) // st + 1
    x = torch.randn(B, Ci, side, side, generator=g).to(dev).requires_grad_(need_x)
    w = (torch.randn(Co, Ci, k, k, generator=g) * (2.0 / (k * k * Ci)) ** 0.5).to(dev).requires_grad_(True)
    dy = torch.randn(B, Co, out, out, generator=g).to(dev)
    wanted = [x, w] if need_x else [w]

    def aten():
        return torch.autograd.grad(F.conv2d(x, w, None, st, p), wanted, dy)

    def hip():
        return torch.autograd.grad(vpn_amd.conv2d(x, w, st, p), wanted, dy)
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
    return {'plain': make(), 'norm': make(fused_norm=True), 'norm+conv': make(fused_norm=True, hip_conv=True),
            'all': make(fused_norm=True, hip_conv=True, hip_conv_strided=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replays', type=int, default=200)
    ap.add_argument('--batches', default='8,64')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'trunkstride_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_trunkstride.py needs a GPU: nothing is measured on a CPU')
    if args.replays < 200:
        raise SystemExit('at least 200 replays per variant')
    dev = torch.device('cuda:0')
    ops = vpn_amd.ops
    lines = ['tools/time_trunkstride.py --replays %d on one MI355X (torch %s): us per forward + backward (y, dx, dw; the stem y and '
             'dw: its input needs no gradient), training mode, median [10th .. 90th percentile] of %d graph replays, each between '
             'two device events, after 20 warm-up replays; the variants of a row alternate.  ATen = F.conv2d (the library, the '
             'plain trunk\'s path), hip = csrc/trunkstride.hip (tile %d x %d x %d, split target %d, at most %d slices; data '
             'gradient in the masked form).  peak: 2 R R C_in C_out B OH OW flop per product / time / 157.3 TFLOP/s.' %
             (args.replays, torch.__version__, args.replays, ops.CONV_TILE, ops.CONV_TILE, ops.CONV_TILE_K, ops.CONV_SPLIT_TARGET,
              ops.CONV_MAX_SPLIT)]
    for B in [int(b) for b in args.batches.split(',')]:
        lines.append('B = %d, 128 x 128 input' % B)
        for name, Ci, Co, side, k, st, p, need_x in SITES:
            q = quantiles(site_steps(Ci, Co, side, k, st, p, need_x, B, dev), args.replays)
            out = (side + 2 * p - k) // st + 1
            flop = (3 if need_x else 2) * 2 * k * k * Ci * Co * B * out * out
            S = [ops.conv2d_splits(B, Ci, Co, side, side, k, st, p, pr) for pr in (ops.CONV_FWD, ops.CONV_DX, ops.CONV_DW)]
            lines.append('  %-22s (%3d -> %3d, %dx%d/%d, %3dx%-3d; slices fwd/dx/dw %2d/%2d/%2d)  ATen %8.1f us [%8.1f .. %8.1f] %4.1f %% of peak   '
                         'hip %8.1f us [%8.1f .. %8.1f] %4.1f %% of peak   ATen / hip %5.2f' %
                         (name, Ci, Co, k, k, st, side, side, *S, *q['ATen'], 100 * flop / (q['ATen'][0] * 1e-6) / PEAK_FLOPS,
                          *q['hip'], 100 * flop / (q['hip'][0] * 1e-6) / PEAK_FLOPS, q['ATen'][0] / q['hip'][0]))
            print(lines[-1], flush=True)
        q = quantiles(trunk_steps(B, dev), args.replays)
        for k, label in (('plain', 'whole trunk, plain (ATen norms, ATen convolutions)'), ('norm', 'whole trunk, fused_norm'),
                         ('norm+conv', 'whole trunk, fused_norm + hip_conv'),
                         ('all', 'whole trunk, fused_norm + hip_conv + hip_conv_strided')):
            lines.append('  %-56s %8.1f us [%8.1f .. %8.1f]   plain / this %5.2f' % (label, *q[k], q['plain'][0] / q[k][0]))
            print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
