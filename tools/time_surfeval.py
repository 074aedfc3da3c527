"""Time the surface evaluation (SurfaceEvaluationMeter.update_mesh, csrc/surfeval.hip) on one MI355X:
B = 8 and B = 64 predicted meshes of V = 16 x 128 = 2048 vertices and F = 4032 faces, n = M = 2048 points, 13 classes, T = 2
thresholds.  Writes profiles/surfeval_time.txt.

    python tools/time_surfeval.py [--rounds 100] [--out profiles/surfeval_time.txt]

Three variants of one evaluation batch, on the same inputs:
  meter, eager     update_mesh as a loop calls it: sample_meshes, face_normals_at, chamfer_nn, vpn_surfeval_accumulate;
  composed, eager  the same metrics from what the package had before: sample_meshes, face normals in torch (gather, cross,
                   normalise), chamfer_nn, torch reductions for the row, then the reference's style of bookkeeping: the
                   batch sums and one row per sample fetched to the host and added in Python (B + 1 read-backs);
  meter, replay    update_mesh captured into a graph once and replayed.
The eager variants are timed with the host clock around the call and a device synchronise (the composed loop synchronises
by itself; a launch returns before its kernel ends), the replay between two device events.  The three alternate within
every round; reported is the median [10th .. 90th percentile] of `rounds` rounds after 20 warm-up rounds.  Before timing,
the two eager variants must agree on the rows (1e-5 relative: the composed normals are torch's) and the class counts.  There is no speed bar; the expectation that is
stated and checked in the output is that the eager meter is not slower than the composed loop by more than the spread
(90th - 10th percentile) of the replays of the same run.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402
from vpn_amd import ops  # noqa: E402
from time_gcn_factored import inputs  # noqa: E402
from time_trunknorm import capture  # noqa: E402

CLASSES, THRESHOLDS, POINTS = 13, (0.01, 0.02), 2048


class ComposedLoop:
    """The metrics of SurfaceEvaluationMeter from the operators the package had before it, with host bookkeeping."""

    def __init__(self, dev):
        self.thr2 = torch.tensor([t * t for t in THRESHOLDS], dtype=torch.float64).float().to(dev)
        self.reset()

    def reset(self):
        W = 6 + 3 * len(THRESHOLDS)
        self.total, self.class_sum, self.class_n, self.n = [0.0] * W, [[0.0] * W for _ in range(CLASSES)], [0] * CLASSES, 0

    def update(self, verts, faces, gt_points, gt_normals, class_indices, seed):
        B = verts.shape[0]
        points, fidx, _ = ops.sample_meshes(verts, faces, POINTS, seed)
        tri = faces.long()[fidx.long()]                                              # [B,n,3]
        c = torch.gather(verts, 1, tri.reshape(B, -1, 1).expand(-1, -1, 3)).reshape(B, POINTS, 3, 3)
        n_pred = torch.nn.functional.normalize(torch.cross(c[:, :, 1] - c[:, :, 0], c[:, :, 2] - c[:, :, 0], dim=-1), dim=-1)
        d1, i1, d2, i2 = ops.chamfer_nn(points, gt_points)
        nc1 = (n_pred * torch.gather(gt_normals, 1, i1.long()[..., None].expand(-1, -1, 3))).sum(-1).abs().double().mean(1)
        nc2 = (gt_normals * torch.gather(n_pred, 1, i2.long()[..., None].expand(-1, -1, 3))).sum(-1).abs().double().mean(1)
        q1, q2 = d1.double() ** 2, d2.double() ** 2                                   # the scan's distances are not squared
        p = (q1[:, :, None] < self.thr2.double()).double().mean(1)
        r = (q2[:, :, None] < self.thr2.double()).double().mean(1)
        f = torch.where(p + r > 0, 2 * p * r / (p + r).clamp_min(1e-300), torch.zeros_like(p))
        rows = torch.cat([torch.stack([q1.mean(1), q2.mean(1), d1.double().mean(1), d2.double().mean(1),
                                       nc1, nc2], 1), p, r, f], 1).float()
        for k, v in enumerate(rows.double().sum(0).tolist()):                         # the batch sums: one read-back
            self.total[k] += v
        for b in range(B):                                                           # one read-back per sample, as `.item()` does
            cls = class_indices[b]
            for k, v in enumerate(rows[b].tolist()):
                self.class_sum[cls][k] += v
            self.class_n[cls] += 1
        self.n += B
        return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'surfeval_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_surfeval.py needs a GPU: nothing is measured on a CPU')
    if args.rounds < 50:
        raise SystemExit('at least 50 rounds')
    dev = torch.device('cuda:0')
    lines = ['tools/time_surfeval.py --rounds %d on one MI355X (torch %s): one evaluation batch of B meshes, V = 2048, F = 4032, n = M = '
             '%d, %d classes, T = %d; us, median [10th .. 90th percentile] of %d rounds after 20 warm-up rounds; the three variants '
             'alternate within a round; eager: host clock around the call and a device synchronise; replay: two device events'
             % (args.rounds, torch.__version__, POINTS, CLASSES, len(THRESHOLDS), args.rounds)]
    for B in (8, 64):
        verts, faces, _maps, _glob, _rgbs = inputs(dev, B=B)
        del _maps, _glob, _rgbs
        faces = ops.faces_i32(faces, dev)
        gen = torch.Generator().manual_seed(28)
        gt_points = ((torch.rand(B, POINTS, 3, generator=gen) - 0.5) * 0.8).to(dev)
        gt_normals = torch.nn.functional.normalize(torch.randn(B, POINTS, 3, generator=gen), dim=-1).to(dev)
        cls_host = [b % CLASSES for b in range(B)]
        cls_dev = torch.tensor(cls_host, dtype=torch.int32, device=dev)
        meter = vpn_amd.SurfaceEvaluationMeter(['c%d' % i for i in range(CLASSES)], dev, thresholds=THRESHOLDS)
        replayed = vpn_amd.SurfaceEvaluationMeter(['c%d' % i for i in range(CLASSES)], dev, thresholds=THRESHOLDS)
        loop = ComposedLoop(dev)
        eager = lambda: meter.update_mesh(verts, faces, gt_points, cls_dev, n=POINTS, seed=5, gt_normals=gt_normals)
        composed = lambda: loop.update(verts, faces, gt_points, gt_normals, cls_host, 5)
        # results first: the same rows and, after one batch each, the same sums
        rows_m, rows_c = eager().double(), composed().double()
        worst = float(((rows_m - rows_c).abs() / rows_c.abs().clamp_min(1e-30)).max())
        if worst > 1e-5:
            raise SystemExit('B = %d: the meter and the composed loop disagree on the rows: %.2e relative' % (B, worst))
        res = meter.result()
        if res['class_n'] != loop.class_n or abs(res['fscore'][1] - loop.total[11] / loop.n) > 1e-6:
            raise SystemExit('B = %d: the meter and the composed loop disagree on the epoch' % B)
        graph = capture(lambda: replayed.update_mesh(verts, faces, gt_points, cls_dev, n=POINTS, seed=5, gt_normals=gt_normals))

        def host_timed(step):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6

        def replay_timed():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3

        variants = {'meter, eager': lambda: host_timed(eager), 'composed, eager': lambda: host_timed(composed), 'meter, replay': replay_timed}
        samples = {k: [] for k in variants}
        for r in range(20 + args.rounds):
            for k, v in variants.items():
                t = v()
                if r >= 20:
                    samples[k].append(t)
        q = {k: [float(torch.quantile(torch.tensor(v, dtype=torch.float64), p)) for p in (0.5, 0.1, 0.9)] for k, v in samples.items()}
        first = len(lines)
        lines.append('B = %d (rows agree within %.1e relative)' % (B, worst))
        for k in variants:
            lines.append('    %-16s %9.1f us [%9.1f .. %9.1f]' % (k, *q[k]))
        spread = q['meter, replay'][2] - q['meter, replay'][1]
        ok = q['meter, eager'][0] <= q['composed, eager'][0] + spread
        lines.append('    expectation (meter, eager <= composed, eager + %.1f us, the spread of the replays): %s; the composed loop takes '
                     '%.2f x the eager meter, %.2f x the replay' % (spread, 'holds' if ok else 'DOES NOT HOLD', q['composed, eager'][0] / q['meter, eager'][0],
                                                                    q['composed, eager'][0] / q['meter, replay'][0]))
        print('\n'.join(lines[first:]), flush=True)
        del graph
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
