"""Time one evaluation batch on one GPU at the reference's evaluation shape (test_gcn.py: B = 8, 2048 refined vertices
against 2048 ground-truth points, Chamfer + EMD with eps 0.005 and 50 rounds, 13 classes) and at B = 64:

  stage      EvaluationMeter.update, eager: scan and auction on two streams, one accumulate launch, no host sync
  graph      the same update captured once and replayed
  baseline   the reference's loop (test_gcn.py:142-152) composed from modules that existed before the stage:
             ChamferDistanceLoss(each_batch=True), EarthMoverDistanceLoss, torch.sqrt(dist).mean(1), then the 2 + 2 B
             .item() calls of the batch means and the class loop.  Timing material only, not code under test.

Every sample of a side is the host time of `--inner` consecutive batches that ends in a device synchronise, divided by
`--inner` (the baseline synchronises by itself; a device-event pair would leave its host work out).  Every side is warmed
up at every shape, the three sides alternate per repetition; median and the 10th..90th percentile of each.  Before timing,
the three sides are fed the same batch and their per-class results are compared (the stage's fp64 batch mean against the
baseline's fp32 one: (B + 3) 2^-24 relative).

    python tools/time_eval.py [--reps 30] [--inner 10] [--out FILE.txt]
    python tools/time_eval.py --once      # one eager update at B = 8 (for a kernel trace)"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vpn_amd  # noqa: E402

DEV = 'cuda'
N, C = 2048, 13
NAMES = ['class%02d' % i for i in range(C)]


class Baseline:
    """test_gcn.py:126-152 on this package's loss modules."""

    def __init__(self):
        self.cd_loss_func = vpn_amd.ChamferDistanceLoss()
        self.emd_loss_func = vpn_amd.EarthMoverDistanceLoss()
        self.reset()

    def reset(self):
        self.n = 0
        self.avg = {'cd': 0.0, 'emd': 0.0}
        self.cls = {'cd': [0.0] * C, 'emd': [0.0] * C}
        self.class_n = [0] * C

    @torch.no_grad()
    def update(self, predict, gt, class_indices):
        batch_cd_loss = self.cd_loss_func(predict, gt, each_batch=True)
        dist, _assignment = self.emd_loss_func(predict, gt, 0.005, 50)
        batch_emd_loss = torch.sqrt(dist).mean(1)
        self.avg['cd'] += batch_cd_loss.mean().item()
        self.avg['emd'] += batch_emd_loss.mean().item()
        self.n += 1
        for b in range(len(batch_cd_loss)):
            self.cls['cd'][class_indices[b]] += batch_cd_loss[b].item()
            self.cls['emd'][class_indices[b]] += batch_emd_loss[b].item()
            self.class_n[class_indices[b]] += 1


def make(B):
    g = torch.Generator().manual_seed(B)
    predict = (torch.rand(B, N, 3, generator=g) - 0.5).to(DEV)
    centres = torch.rand(B, 8, 3, generator=g) * 0.6 - 0.3
    which = torch.randint(0, 8, (B, N), generator=g)
    gt = torch.gather(centres, 1, which[..., None].expand(-1, -1, 3)) + 0.05 * torch.randn(B, N, 3, generator=g)
    return predict, gt.clamp(-0.5, 0.5).to(DEV), torch.arange(B) % C            # class indices on the host, like a DataLoader's


def host_timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def spread(ts):
    q = statistics.quantiles(ts, n=10)
    return statistics.median(ts), q[0], q[-1]


def agree(meter_res, base, B):
    bound = (B + 3) * 2.0 ** -24           # the fp32 batch mean's own rounding, and one fp32 ulp of every emd_b
    for key in ('cd', 'emd'):
        assert abs(meter_res[key] - base.avg[key] / base.n) <= bound * abs(meter_res[key]), key
        for c in range(C):
            if base.class_n[c]:
                want = base.cls[key][c] / base.class_n[c]
                # cd_b is the Chamfer module's value bit for bit; emd_b is the fp64 mean rounded once, torch's an fp32 mean
                assert abs(meter_res['class_' + key][c] - want) <= (0.0 if key == 'cd' else 2.0 ** -22 * want), (key, c)
    assert meter_res['class_n'] == base.class_n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--out', default='', help='also write the printed lines to this file')
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'timing needs the GPU'
    if args.once:
        predict, gt, idx = make(8)
        vpn_amd.EvaluationMeter(NAMES, DEV).update(predict, gt, idx)
        torch.cuda.synchronize()
        return
    lines = ['tools/time_eval.py --reps %d --inner %d on one MI355X: %d vs %d points, %d classes, Chamfer + EMD (eps 0.005, 50 '
             'rounds); ms per batch,' % (args.reps, args.inner, N, N, C),
             'median [10th .. 90th percentile] of %d samples, each the host time of %d consecutive batches up to a device '
             'synchronise; the sides alternate' % (args.reps, args.inner)]
    print('\n'.join(lines), flush=True)
    for B in (8, 64):
        predict, gt, idx = make(B)
        eager, replayed, base = vpn_amd.EvaluationMeter(NAMES, DEV), vpn_amd.EvaluationMeter(NAMES, DEV), Baseline()
        sidx = idx.to(device=DEV, dtype=torch.int32)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            replayed.update(predict, gt, sidx)                       # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            replayed.update(predict, gt, sidx)
        sides = {'stage': lambda: eager.update(predict, gt, idx), 'graph': graph.replay,
                 'baseline': lambda: base.update(predict, gt, idx)}
        # the same batch through all three: the same results
        replayed.reset()
        for fn in sides.values():
            fn()
        agree(eager.result(), base, B)
        assert replayed.result() == eager.result()
        for _ in range(3):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in sides}
        for _ in range(args.reps):
            for k, fn in sides.items():
                ts[k].append(host_timed(fn, args.inner))
        s = {k: spread(v) for k, v in ts.items()}
        line = 'B=%-2d  ' % B + '   '.join('%s %7.3f ms [%.3f .. %.3f]' % ((k,) + s[k]) for k in sides)
        line += '   baseline / stage x%.2f, baseline / graph x%.2f' % (s['baseline'][0] / s['stage'][0], s['baseline'][0] / s['graph'][0])
        lines.append(line)
        print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
