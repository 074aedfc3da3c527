"""Time the batch augmentation stage on one GPU: cut_mix_data and mixup_points, each alone, at B = 8 and B = 64, N = 2048,
128 x 128 images, against the way the same thing is done WITHOUT this stage: the reference's per-sample loops
(modules/augmentation/cutmix.py:24-50, point_mixup.py:24-40) restated here on the API that existed before
(EarthMoverDistanceLoss on batches of one, 100 rounds; mask / cat / host randperm / gather per sample).  That baseline is
timing material only, not code under test.  Device events around every call, a warm-up of every shape, the two sides
alternating per repetition; median and the 10th..90th percentile spread of each side.

    python tools/time_augment.py [--reps 30] [--out FILE.json]
    python tools/time_augment.py --once      # one cut_mix_data and one mixup_points call at B = 8 (for a kernel trace)"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vpn_amd  # noqa: E402

DEV = 'cuda'
N, SIZE = 2048, 128


def baseline_adjust(points, n):
    if points.size(0) == n:
        return points
    if points.size(0) > n:
        return points[torch.randperm(points.size(0))[:n].to(DEV), :]
    return points[torch.randint(0, points.size(0), (n,)).to(DEV), :]


def baseline_cutmix(rgbs, sils, pts):
    B, _, _, W = rgbs.size()
    ratio = 0.3 + torch.rand(1).item() * 0.4
    ci, cut = int(W * ratio), (0.5 - ratio) * 2 * 0.30769
    idx = torch.randperm(B).to(DEV)
    rgbs = torch.cat([rgbs[..., :ci], rgbs[idx, ..., ci:]], dim=3)
    sils = torch.cat([sils[..., :ci], sils[idx, ..., ci:]], dim=3)
    out = torch.zeros_like(pts)
    for b in range(B):
        p1, p2 = pts[b], pts[idx[b]]
        out[b] = baseline_adjust(torch.cat([p1[p1[:, 2] >= cut], p2[p2[:, 2] < cut]], dim=0), pts.size(1))
    return rgbs, sils, out


def baseline_mixup(pts, emd=vpn_amd.EarthMoverDistanceLoss()):
    B = pts.size(0)
    r = torch.rand(1).item()
    idx = torch.randperm(B).to(DEV)
    out = torch.zeros_like(pts)
    for b in range(B):
        p1, p2 = pts[b], pts[idx[b]]
        _, a = emd(p1[None], p2[None], 0.005, 100)
        out[b] = (1 - r) * p1 + r * p2[a[0].long()]
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ts):
    q = statistics.quantiles(ts, n=10)
    return {'median_ms': statistics.median(ts), 'p10_ms': q[0], 'p90_ms': q[-1]}


def make(B):
    g = torch.Generator().manual_seed(B)
    pts = (torch.rand(B, N, 3, generator=g) - 0.5).to(DEV)
    rgbs = torch.rand(B, 3, SIZE, SIZE, generator=g).to(DEV)
    sils = (torch.rand(B, 1, SIZE, SIZE, generator=g) > 0.5).float().to(DEV)
    return pts, rgbs, sils


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default='', help='also write the results as JSON to this file')
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'timing needs the GPU'
    torch.manual_seed(0)
    if args.once:
        pts, rgbs, sils = make(8)
        vpn_amd.cut_mix_data(rgbs, sils, pts)
        vpn_amd.mixup_points(pts)
        torch.cuda.synchronize()
        return
    res = {}
    for B in (8, 64):
        pts, rgbs, sils = make(B)
        sides = {'cutmix': (lambda: vpn_amd.cut_mix_data(rgbs, sils, pts), lambda: baseline_cutmix(rgbs, sils, pts)),
                 'mixup': (lambda: vpn_amd.mixup_points(pts), lambda: baseline_mixup(pts))}
        for name, (new, old) in sides.items():
            for _ in range(3):
                new(); old()
            torch.cuda.synchronize()
            tn, to = [], []
            for _ in range(args.reps):
                tn.append(timed(new))
                to.append(timed(old))
            r = {'new': spread(tn), 'baseline': spread(to)}
            r['ratio_of_medians'] = r['baseline']['median_ms'] / r['new']['median_ms']
            r['faster_beyond_spread'] = r['new']['p90_ms'] < r['baseline']['p10_ms']
            res['%s_B%d' % (name, B)] = r
            print('%-6s B=%-2d  new %8.3f ms [%.3f .. %.3f]   baseline %8.3f ms [%.3f .. %.3f]   x%.1f' % (
                name, B, r['new']['median_ms'], r['new']['p10_ms'], r['new']['p90_ms'], r['baseline']['median_ms'],
                r['baseline']['p10_ms'], r['baseline']['p90_ms'], r['ratio_of_medians']), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'N': N, 'image': SIZE, 'reps': args.reps, 'results': res}, f, indent=1)


if __name__ == '__main__':
    main()
