"""Time the on-device ACD-mix data stage (modules/augmentation.acd_mix_data) on one GPU at S = 1 and S = 8
pairs of objects, n = 2048 points each, 8 + 8 hulls, 2048 union points from 4096 candidates, 20 views of 128 x 128: the
whole stage, its middle alone (ops.hull_augment + ops.union_surface on given candidates), and that middle done on the host
by the numpy restatement (tests/acdmix_ref.py, with the copies to the host), which is timing material only.  Device events
around every call, a warm-up of every shape, the sides alternating per repetition; median and the 10th..90th percentile of
each.  Then one profiled call per batch size: the device time of every kernel of the stage (the library's own launch
profile).

    python tools/time_acd_mix.py [--reps 20] [--host-reps 3] [--out profiles/acd_mix_time.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import vpn_amd  # noqa: E402
import acdmix_ref as AR  # noqa: E402
from vpn_amd import _lib, ops  # noqa: E402
from vpn_amd.modules import augmentation  # noqa: E402

DEV = 'cuda'
N, HULLS, VIEWS, SIZE, UNION, MARGIN = 2048, 8, 20, 128, 2048, 1e-3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ts):
    if len(ts) < 2:
        return ts[0], ts[0], ts[0]
    q = statistics.quantiles(ts, n=10)
    return statistics.median(ts), q[0], q[-1]


def clouds(S, g, centre):
    v = torch.randn(S, N, 3, generator=g)
    v = v / v.norm(dim=2, keepdim=True) * torch.tensor([0.4, 0.3, 0.25]) + torch.tensor(centre)
    return v.to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'acd_mix_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'timing needs the GPU'
    lines = ['ACD-mix data stage on %s: two clouds of %d points, %d + %d hulls, %d union points of %d candidates, margin %g, %d views '
             'of %d x %d, %d ground-truth points a view' % (torch.cuda.get_device_name(0), N, HULLS, HULLS, UNION, 2 * UNION, MARGIN, VIEWS,
                                                            SIZE, SIZE, 2048),
             'median [10th .. 90th percentile] over %d repetitions (host: %d), milliseconds' % (args.reps, args.host_reps), '']
    for S in (1, 8):
        g = torch.Generator().manual_seed(S)
        p1, p2 = clouds(S, g, (0.0, 0.0, 0.0)), clouds(S, g, (0.4, 0.0, 0.0))
        torch.manual_seed(S)
        _out = vpn_amd.acd_mix_data(p1, p2, views=VIEWS, img_size=SIZE, union_points=UNION, margin=MARGIN, return_parts=True)
        parts = _out[-1]
        torch.manual_seed(S)
        draws = {k: v.to(DEV) for k, v in augmentation._augment_draws(S, 2, HULLS, None, None, None, None, None, None).items()}
        colors = torch.rand(S, HULLS, 3, generator=g).to(DEV)
        cams = torch.stack([3.0 + torch.rand(S, VIEWS, generator=g) * 2, (torch.rand(S, VIEWS, generator=g) - 0.5) * 90,
                            torch.rand(S, VIEWS, generator=g) * 360], -1).to(DEV)
        h1 = vpn_amd.acd(p1 / p1.amax(dim=(1, 2), keepdim=True), HULLS)
        h2 = vpn_amd.acd(p2 / p2.amax(dim=(1, 2), keepdim=True), HULLS)
        merged = torch.cat([h1, h2], 1).contiguous()
        group = ops.const_tensor((0,) * HULLS + (1,) * HULLS, torch.int32, DEV)
        dirs, cand, cand_hull = parts['dirs'], parts['cand'], parts['cand_hull']
        aug = ('coin', 'u_num', 'scale', 'turn', 'shift', 'u_hull')

        def stage():
            return vpn_amd.acd_mix_data(p1, p2, views=VIEWS, img_size=SIZE, union_points=UNION, margin=MARGIN, colors=colors, cams=cams,
                                        seed=1, gt_seed=2, **draws)

        def middle():
            hulls, keep = ops.hull_augment(merged, group, *(draws[k] for k in aug))
            return ops.union_surface(hulls, keep, dirs, cand, cand_hull, UNION, MARGIN)

        def host_middle():
            t = time.perf_counter()
            d = {k: draws[k].cpu().numpy() for k in aug}
            hulls, keep = AR.hull_augment(merged.cpu().numpy(), group.cpu().numpy(), **d)
            AR.union_surface(hulls, keep, dirs.cpu().numpy(), cand.cpu().numpy(), cand_hull.cpu().numpy(), MARGIN, UNION)
            return (time.perf_counter() - t) * 1e3

        for _ in range(3):
            stage(); middle()
        torch.cuda.synchronize()
        ts, tm, tc = [], [], []
        for r in range(args.reps):
            ts.append(timed(stage))
            tm.append(timed(middle))
            if r < args.host_reps:
                tc.append(host_middle())
        for name, t in (('acd_mix_data (whole stage)', ts), ('hull_augment + union_surface (the middle)', tm),
                        ('numpy restatement of the middle, host', tc)):
            lines.append('S = %-2d  %-44s %10.3f [%.3f .. %.3f]' % ((S, name) + spread(t)))
        with _lib.KernelProfile() as kp:
            stage()
            torch.cuda.synchronize()
        prof = kp.summary()
        lines.append('S = %-2d  kernels of one call (calls x mean ms):' % S)
        for k, (calls, ms) in sorted(prof.items(), key=lambda kv: -kv[1][0] * kv[1][1]):
            lines.append('          %-34s %3d x %9.4f' % (k, calls, ms))
        lines.append('')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
