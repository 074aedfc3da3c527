"""Time the trunk's inference form (ResNet18.fold, ops.conv2d_bias_act, csrc/trunkfold.hip) against what it
replaces on one MI355X: the eval-mode ResNet-18 trunk forward under no_grad on 128 x 128 images, B = 8 (train_gcn.py's
default) and B = 64.  Writes profiles/trunkfold_time.txt.

    python tools/time_trunkfold.py [--replays 50] [--out profiles/trunkfold_time.txt]

  (a) the whole trunk (_trunk_features: the four stage maps and the pooled features): plain (ATen convolutions and norms),
      fused_norm + fused_pool + fused_tail (csrc/trunknorm.hip around ATen's convolutions), folded;
  (b) the 20 convolution sites one by one: ATen's conv -> bn (eval) -> add -> relu against one conv2d_bias_act on the folded
      tensors (sites of one shape are timed once and counted);
  (c) the frozen VPNetOneRes forward of examples/train_gcn_step.py (16 primitives), plain against folded.

Each variant is captured into a graph once; the graphs of a row are replayed in turn in the same process, every replay
between two device events; reported is the median (10th .. 90th percentile) of `replays` replays after 20 warm-up replays.
There is no speed bar: the numbers are reported, not asserted.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402
from vpn_amd import ops  # noqa: E402
from vpn_amd.modules.network import ResNet18, VPNetOneRes, _trunk_features  # noqa: E402
from time_trunknorm import capture, measure  # noqa: E402


def _no_grad(f):
    def step():
        with torch.no_grad():
            return f()
    return step


def _randomise_norms(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    return model


def trunk_steps(B, dev):
    torch.manual_seed(1)
    state = _randomise_norms(ResNet18(), 2).state_dict()
    imgs = torch.randn(B, 3, 128, 128, generator=torch.Generator().manual_seed(3)).to(dev)
    forms = {'plain': dict(), 'norm + pool + tail': dict(fused_norm=True, fused_pool=True, fused_tail=True), 'folded': dict()}
    steps = {}
    for name, kwargs in forms.items():
        m = ResNet18(**kwargs)
        m.load_state_dict(state, strict=True)
        m = m.to(dev).eval()
        if name == 'folded':
            m.fold()
        steps[name] = _no_grad(lambda m=m: _trunk_features(m, imgs))
    return steps


def site_shapes(B, side=128):
    """[(label, count, (C_in, C_out, H, R, stride, pad), residual, relu)] of the trunk's 20 sites, one row a distinct shape."""
    rows = [('conv1 7x7/2', 1, (3, 64, side, 7, 2, 3), False, True)]
    s = side // 4
    rows += [('layer1 conv1', 2, (64, 64, s, 3, 1, 1), False, True), ('layer1 conv2 + identity', 2, (64, 64, s, 3, 1, 1), True, True)]
    for i, c in enumerate((64, 128, 256)):
        n = 'layer%d' % (i + 2)
        rows += [(n + '.0 conv1 3x3/2', 1, (c, 2 * c, s, 3, 2, 1), False, True),
                 (n + '.0 downsample 1x1/2', 1, (c, 2 * c, s, 1, 2, 0), False, False)]
        s //= 2
        rows += [(n + '.1 conv1', 1, (2 * c, 2 * c, s, 3, 1, 1), False, True),
                 (n + ' conv2 + identity', 2, (2 * c, 2 * c, s, 3, 1, 1), True, True)]
    assert sum(r[1] for r in rows) == 20
    return rows


def site_steps(B, cfg, residual, relu, dev):
    Ci, Co, side, R, st, p = cfg
    g = torch.Generator().manual_seed(Ci + Co + R)
    conv = nn.Conv2d(Ci, Co, R, st, p, bias=False).to(dev)
    bn = _randomise_norms(nn.BatchNorm2d(Co), Co).to(dev).eval()
    x = torch.randn(B, Ci, side, side, generator=g).to(dev)
    OH, OW = ops.conv2d_out_size(side, side, R, st, p)
    res = torch.randn(B, Co, OH, OW, generator=g).to(dev) if residual else None
    wf, bf = vpn_amd.fold_batch_norm(conv.weight, bn)

    def aten():
        out = bn(conv(x))
        if residual:
            out = out + res
        return F.relu(out, inplace=True) if relu else out

    def folded():
        return vpn_amd.conv2d_bias_act(x, wf, bf, res, st, p, relu)
    return {'ATen': _no_grad(aten), 'conv2d_bias_act': _no_grad(folded)}, ops.conv2d_splits(B, Ci, Co, side, side, R, st, p, ops.CONV_FWD)


def vpn_steps(B, dev):
    torch.manual_seed(4)
    base = VPNetOneRes(vp_num=16)
    _randomise_norms(base.resnet, 5)
    imgs = torch.randn(B, 3, 128, 128, generator=torch.Generator().manual_seed(6)).to(dev)
    steps = {}
    for name in ('plain', 'folded'):
        m = VPNetOneRes(vp_num=16)
        m.load_state_dict(base.state_dict(), strict=True)
        m = m.to(dev).eval()
        if name == 'folded':
            m.resnet.fold()
        steps[name] = _no_grad(lambda m=m: m(imgs))
    return steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replays', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'trunkfold_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_trunkfold.py needs a GPU: nothing is measured on a CPU')
    if args.replays < 50:
        raise SystemExit('at least 50 replays per variant')
    dev = torch.device('cuda:0')
    lines = ['tools/time_trunkfold.py --replays %d on one MI355X (torch %s): eval mode under no_grad, 128 x 128 images; us, median '
             '[10th .. 90th percentile] of %d graph replays, each between two device events, after 20 warm-up replays; the '
             'variants of a row alternate' % (args.replays, torch.__version__, args.replays)]

    def row(label, steps):
        graphs = {k: capture(v) for k, v in steps.items()}
        t = {k: torch.tensor(v, dtype=torch.float64) * 1e3 for k, v in measure(graphs, args.replays).items()}
        q = {k: [float(torch.quantile(v, p)) for p in (0.5, 0.1, 0.9)] for k, v in t.items()}
        first = len(lines)
        lines.append(label)
        base = q[next(iter(graphs))][0]
        for k in graphs:
            lines.append('    %-20s %8.1f us [%8.1f .. %8.1f]   %5.2f x the first variant' % (k, *q[k], q[k][0] / base))
        print('\n'.join(lines[first:]), flush=True)
        return {k: v[0] for k, v in q.items()}

    for B in (8, 64):
        row('(a) ResNet-18 trunk forward (four maps and the pooled features), B = %d' % B, trunk_steps(B, dev))
    for B in (8, 64):
        total = {'ATen': 0.0, 'conv2d_bias_act': 0.0}
        for label, count, cfg, residual, relu in site_shapes(B):
            steps, S = site_steps(B, cfg, residual, relu, dev)
            med = row('(b) B = %d, %s (x %d in the trunk): C %d -> %d at %d^2, %d slice%s' %
                      (B, label, count, cfg[0], cfg[1], cfg[2], S, '' if S == 1 else 's'), steps)
            for k in total:
                total[k] += count * med[k]
        lines.append('(b) B = %d, the 20 sites summed by their medians: ATen %.1f us, conv2d_bias_act %.1f us (%.2f x)' %
                     (B, total['ATen'], total['conv2d_bias_act'], total['conv2d_bias_act'] / total['ATen']))
        print(lines[-1], flush=True)
    for B in (8, 64):
        row('(c) frozen VPNetOneRes forward (16 primitives), B = %d' % B, vpn_steps(B, dev))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
