"""Time the FC heads on one GPU: FcStackFunction (csrc/fcstack.hip, one launch per layer for all heads) against the same
parameters run through their nn.Sequential, that is torch's BLAS path (15 GEMMs forward, 30 backward, plus the head
post-processing launch).  Heads forward and forward + backward at B = 8 and B = 64 with K = 16, and SDNet's deform stack
at B = 8.  Both sides are captured into a HIP graph each and replayed in the same process, alternating; device events
around a burst of replays; median and the 10th..90th percentile of the per-replay time.  Achieved bytes/s is the weight
traffic the algorithm needs (forward: every weight once; forward + backward: read twice, dW written once) over the
measured time, against the measured HBM copy peak; the dX partial sums of the backward are extra traffic that this figure does
not count.

    python tools/time_network.py [--reps 30] [--burst 20] [--out profiles/network_time.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vpn_amd  # noqa: E402
from vpn_amd.modules.network import FcHeads, pack_head_outputs  # noqa: E402

HBM_PEAK = 6.29e12      # bytes/s, the measured float4 copy rate of the MI355X (8.0e12 on the datasheet)


def spread(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[len(ts) // 10], ts[(len(ts) * 9) // 10]


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--burst', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_network.py measures on a GPU only'
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    K = 16
    lines = ['FC heads, fp32, K = %d: fused stack (one launch per layer) vs nn.Sequential (BLAS); graph replay, %d reps of %d replays'
             % (K, args.reps, args.burst)]
    cases = [('VP heads', {'volume_fc': 3 * K, 'rotate_fc': 4 * K, 'translate_fc': 3 * K}, 'vp_pack', 8),
             ('VP heads', {'volume_fc': 3 * K, 'rotate_fc': 4 * K, 'translate_fc': 3 * K}, 'vp_pack', 64),
             ('SDNet deform', {'deform': 386 * 3}, 'tanh', 8)]
    for name, heads, epilogue, B in cases:
        net = FcHeads(heads).to(dev)
        seqs = [getattr(net, n) for n in heads]
        weights = sum(p.numel() for p in net.parameters() if p.dim() == 2)
        x = torch.randn(B, 512, device=dev, requires_grad=True)
        params = [p for p in net.parameters()]
        rule = dict(is_sigmoid=True, clamp_min=vpn_amd.config.VP_CLAMP_MIN, clamp_max=vpn_amd.config.VP_CLAMP_MAX,
                    volume_restrict=vpn_amd.config.VOLUME_RESTRICT) if epilogue == 'vp_pack' else {}

        def fused():
            return net.run_heads([x] * len(seqs), epilogue, **rule)

        def blas():
            raw = [s(x) for s in seqs]
            return pack_head_outputs(*raw) if epilogue == 'vp_pack' else torch.tanh(raw[0])

        wt = torch.randn_like(fused())

        def with_bwd(fwd):
            return lambda: torch.autograd.grad((fwd() * wt).sum(), [x] + params)

        with torch.no_grad():
            err = float((fused() - blas()).abs().max())
        for label, f_fn, b_fn, nbytes in (('forward', fused, blas, 4 * weights),
                                          ('forward + backward', with_bwd(fused), with_bwd(blas), 12 * weights)):
            graphs = {'fused': capture(f_fn), 'BLAS': capture(b_fn)}
            times = {k: [] for k in graphs}
            for _ in range(args.reps):
                for k, g in graphs.items():              # alternate the two inside every repetition
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.burst):
                        g.replay()
                    b.record()
                    torch.cuda.synchronize()
                    times[k].append(a.elapsed_time(b) / args.burst)
            f, c = spread(times['fused']), spread(times['BLAS'])
            lines.append('%-13s B = %2d  %-18s fused %.4f ms (%.4f .. %.4f) = %.2f TB/s of weight traffic, %.0f %% of the %.2f TB/s copy peak'
                         ' | BLAS %.4f ms (%.4f .. %.4f) | fused / BLAS = %.2f'
                         % (name, B, label, f[0], f[1], f[2], nbytes / f[0] / 1e9, 100 * nbytes / (f[0] * 1e-3) / HBM_PEAK,
                            HBM_PEAK / 1e12, c[0], c[1], c[2], f[0] / c[0]))
        lines.append('              max |fused - BLAS| of the outputs: %.2e; %d weights = %.1f MB' % (err, weights, 4 * weights / 1e6))
        with vpn_amd._lib.KernelProfile() as kp:
            with_bwd(fused)()
            torch.cuda.synchronize()
        for k, (n, ms) in sorted(kp.summary().items()):
            lines.append('              %-18s %2d x %.4f ms' % (k, n, ms))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
