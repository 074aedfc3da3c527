"""Time the optimiser step on one MI355X: vpn_amd.Adam (csrc/optim.hip, one launch per step) against torch.optim.Adam's
default (foreach) form and its fused=True form, both from the installed torch, on the parameter sets of VPNetOneRes at
K = 16 and of GCNModel.  Writes profiles/optim_time.txt.

    python tools/time_optim.py [--reps 9] [--inner 20] [--out profiles/optim_time.txt]

What is timed: `inner` consecutive optimiser iterations between two device events, `reps` such samples per variant, the
variants alternating inside a repetition; reported is the median (10th .. 90th percentile) per iteration.  The gradients are
filled once and stay allocated: an iteration is `step()` alone, or `step()` followed by the zeroing the next backward needs
(`zero_grad(set_to_none=False)` for torch: a pass of its own; `step(zero_grad=True)` here: the same launch).  vpn_amd.Adam
is also timed as replays of a captured graph of `inner` steps; torch's two forms keep their step counts where a capture
cannot follow them (capturable=False, the default a user gets), so they are timed as plain calls only.  The byte model is 28
bytes per parameter (read p g m v, write p m v) and 32 with the zeroing; the rate printed is that model over the measured
time, not a counter reading.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402
from vpn_amd.modules.network import GCNModel  # noqa: E402


def clones(shapes, dev, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    ps = [torch.randn(s, generator=g).to(dev).requires_grad_(True) for s in shapes]
    for p in ps:
        p.grad = (torch.randn(p.shape, generator=g) * 1e-2).to(dev)
    return ps


def variants(shapes, dev, inner):
    """name -> (callable that runs `inner` iterations, bytes per parameter of the model)"""
    hyper = dict(lr=1e-4, betas=(0.9, 0.99), weight_decay=1e-6)          # train.py:83
    out = {}

    def torch_pair(name, **kw):
        ps = clones(shapes, dev, 1)
        opt = torch.optim.Adam(ps, **hyper, **kw)

        def step_only():
            for _ in range(inner):
                opt.step()

        def step_zero():
            for _ in range(inner):
                opt.step()
                opt.zero_grad(set_to_none=False)
        out[name + ' step'] = (step_only, 28)
        out[name + ' step + zero_grad'] = (step_zero, 32)

    torch_pair('torch foreach')
    torch_pair('torch fused', fused=True)
    for zero, nbytes in ((False, 28), (True, 32)):
        ps = clones(shapes, dev, 1)
        opt = vpn_amd.Adam(ps, **hyper)

        def plain(opt=opt, zero=zero):
            for _ in range(inner):
                opt.step(zero_grad=zero)
        label = 'vpn_amd step' + ('(zero_grad=True)' if zero else '')
        out[label] = (plain, nbytes)
        plain()                                                          # the table is uploaded before the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            plain()
        out[label + ', graph replay'] = (graph.replay, nbytes)
    return out


def measure(runs, reps):
    for fn, _ in runs.values():                                          # warm up every variant
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in runs}
    for _ in range(reps):
        for name, (fn, _) in runs.items():                               # the variants alternate
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            samples[name].append(a.elapsed_time(b))
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'optim_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_optim.py needs a GPU: nothing is measured on a CPU')
    dev = torch.device('cuda:0')
    sets = {'VPNetOneRes(vp_num=16)': [tuple(p.shape) for p in vpn_amd.VPNetOneRes(vp_num=16).parameters()],
            'GCNModel()': [tuple(p.shape) for p in GCNModel().parameters()]}
    lines = ['tools/time_optim.py --reps %d --inner %d on one MI355X (torch %s): us per optimiser iteration, median [10th .. 90th '
             'percentile] of %d samples of %d consecutive iterations between two device events; the variants alternate; GB/s = '
             'the byte model (28 bytes per parameter, 32 with gradient zeroing) over the median' %
             (args.reps, args.inner, torch.__version__, args.reps, args.inner)]
    for name, shapes in sets.items():
        n = sum(int(torch.Size(s).numel()) for s in shapes)
        lines.append('%s: %d tensors, %d parameters, %.1f MB at 28 bytes each' % (name, len(shapes), n, n * 28 / 1e6))
        runs = variants(shapes, dev, args.inner)
        for label, ms in measure(runs, args.reps).items():
            t = torch.tensor(ms, dtype=torch.float64) * 1e3 / args.inner
            med, lo, hi = (float(torch.quantile(t, q)) for q in (0.5, 0.1, 0.9))
            lines.append('  %-46s %9.1f us [%9.1f .. %9.1f]   %7.1f GB/s' % (label, med, lo, hi, n * runs[label][1] / med / 1e3))
        del runs
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
