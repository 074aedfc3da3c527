"""Time the on-device point mix-up data stage (modules/augmentation.point_mixup_data) on one GPU at B = 8 and
B = 64, n = 2048, 16 hulls, 128 x 128 images: the whole stage, its cloud -> mesh step alone (ops.hull_meshes), and that
step done on the host by the numpy restatement (tests/reconstruct_ref.py, with the copy of the cloud to the host), which
is timing material only.  Device events around every call, a warm-up of every shape, the sides alternating per
repetition; median and the 10th..90th percentile of each.  Then one profiled call per batch size: the device time of
every kernel of the stage (the library's own launch profile).

    python tools/time_point_mixup.py [--reps 20] [--host-reps 3] [--out profiles/point_mixup_time.txt]"""
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
import reconstruct_ref as RR  # noqa: E402
from vpn_amd import _lib, ops  # noqa: E402

DEV = 'cuda'
N, HULLS, ITERS, SIZE = 2048, 16, 8, 128


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


def host_hulls(pts, dirs):
    t = time.perf_counter()
    p = pts.cpu().numpy()
    lab, cen, _ = RR.cluster_points(p, HULLS, ITERS)
    RR.support_hulls(p, lab, cen, dirs)
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'point_mixup_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'timing needs the GPU'
    lines = ['point mix-up data stage on %s: n = %d, %d hulls, %d Lloyd rounds, %d x %d images, %d new points' % (
        torch.cuda.get_device_name(0), N, HULLS, ITERS, SIZE, SIZE, 2048),
        'median [10th .. 90th percentile] over %d repetitions (host: %d), milliseconds' % (args.reps, args.host_reps), '']
    for B in (8, 64):
        g = torch.Generator().manual_seed(B)
        pts = (torch.rand(B, N, 3, generator=g) - 0.5).to(DEV) * 0.6
        idx = ops.partner_indices(torch.randperm(B, generator=g), B, DEV)
        colors = torch.rand(B, HULLS, 3, generator=g).to(DEV)
        dirs = ops.hull_template(HULLS, 'cpu')[0].numpy()

        def stage():
            return vpn_amd.point_mixup_data(pts, ratio=0.4, indices=idx, colors=colors, seed=1)

        def hulls():
            return ops.hull_meshes(pts, HULLS, ITERS)

        for _ in range(3):
            stage(); hulls()
        torch.cuda.synchronize()
        ts, th, tc = [], [], []
        for r in range(args.reps):
            ts.append(timed(stage))
            th.append(timed(hulls))
            if r < args.host_reps:
                tc.append(host_hulls(pts, dirs))
        for name, t in (('point_mixup_data (whole stage)', ts), ('ops.hull_meshes (cloud -> mesh)', th),
                        ('numpy restatement of cloud -> mesh, host', tc)):
            lines.append('B = %-2d  %-42s %10.3f [%.3f .. %.3f]' % ((B, name) + spread(t)))
        with _lib.KernelProfile() as kp:
            stage()
            torch.cuda.synchronize()
        prof = kp.summary()
        lines.append('B = %-2d  kernels of one call (calls x mean ms):' % B)
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
