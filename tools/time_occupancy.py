"""Time the volumetric evaluation (VolumeEvaluationMeter, csrc/occupancy.hip) on one MI355X: B = 8 and B = 64
samples, Q = 32^3 grid queries, K = 16 primitives, a predicted mesh of V = 16 x 128 = 2048 vertices and F = 4032 faces, ragged
ground truth of 2304 .. 2976 faces a mesh, 13 classes.  Writes profiles/occupancy_time.txt.

    python tools/time_occupancy.py [--rounds 50] [--out profiles/occupancy_time.txt]

Variants of one evaluation batch, on the same inputs:
  primitives, eager / replay   update_primitives: primitive_occupancy, mesh_occupancy of the ground truth, vpn_voliou_accumulate;
  mesh, eager / replay         update_mesh: mesh_occupancy of the prediction and of the ground truth, vpn_voliou_accumulate;
  winding, replay              ops.winding_number of the predicted mesh alone (three launches): B Q F (query, face) pairs;
  composed, eager              what update_mesh measures, from torch ops: the [B,chunk,F] table of solid angles of the prediction
                               in query chunks that fit in memory, the ground truth mesh by mesh, torch reductions for the row,
                               then the reference's style of bookkeeping (the batch sums and one row per sample fetched to
                               the host and added in Python).
The eager variants are timed with the host clock around the call and a device synchronise, the replays between two device
events.  The variants alternate within every round; reported is the median [10th .. 90th percentile] of `rounds` rounds after 5
warm-up rounds; the composed loop, which takes a large multiple of the others, runs in every `--composed-every`-th round only.
Before timing, the meter and the composed loop must agree on the counts of every sample but for queries whose composed winding
number lies within 1e-3 of 0.5.  There is no speed bar; the expectation that is stated and checked in the output is that the
eager meter is not slower than the composed loop by more than the spread (90th - 10th percentile) of the replays of the same
run.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpn_amd  # noqa: E402
from vpn_amd import ops  # noqa: E402
from vpn_amd.modules.meshing import uv_sphere  # noqa: E402
from time_trunknorm import capture  # noqa: E402

CLASSES, RESOLUTION, K = 13, 32, 16
PAIR_BUDGET = 6e7                       # (query, face) pairs of one chunk of the composed loop: about 3 GB of fp32 temporaries


def lattice(seg, rings):
    """A closed, outward-wound sphere lattice: rings x seg vertices and two poles, 2 seg rings faces."""
    v, f = [], []
    for r in range(rings):
        th = math.pi * (r + 1) / (rings + 1)
        for i in range(seg):
            t = 2 * math.pi * i / seg
            v.append([math.sin(th) * math.cos(t), math.sin(th) * math.sin(t), math.cos(th)])
    v += [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]
    top, bottom = rings * seg, rings * seg + 1
    for i in range(seg):
        j = (i + 1) % seg
        f += [[i, j, top], [(rings - 1) * seg + j, (rings - 1) * seg + i, bottom]]
        for r in range(rings - 1):
            f += [[r * seg + i, (r + 1) * seg + i, (r + 1) * seg + j], [r * seg + i, (r + 1) * seg + j, r * seg + j]]
    return torch.tensor(v), torch.tensor(f)


def make_inputs(B, dev):
    g = torch.Generator().manual_seed(29)
    sv, sf = uv_sphere()
    sv, sf = sv.cpu(), sf.cpu().flip(1)                                       # the template is wound clockwise seen from outside
    verts = torch.cat([sv[None] * (torch.rand(B, 1, 3, generator=g) * 0.15 + 0.08) + (torch.rand(B, 1, 3, generator=g) - 0.5) * 0.5
                       for _ in range(K)], 1)
    faces = torch.cat([sf + sv.shape[0] * k for k in range(K)])
    params = torch.cat([torch.rand(B, K, 3, generator=g) * 0.15 + 0.08, torch.randn(B, K, 3, generator=g), torch.rand(B, K, 1, generator=g),
                        (torch.rand(B, K, 3, generator=g) - 0.5) * 0.5], 2)
    kinds = [k % 2 for k in range(K)]
    meshes = []
    for b in range(B):
        v, f = lattice(48, 24 + b % 8)
        meshes.append((v * (torch.rand(3, generator=g) * 0.2 + 0.2) + (torch.rand(3, generator=g) - 0.5) * 0.2, f))
    gt = vpn_amd.MeshBatch.pack(meshes, dev)
    cls_host = [b % CLASSES for b in range(B)]
    return dict(verts=verts.to(dev).contiguous(), faces=ops.faces_i32(faces, dev), params=params.float().to(dev).contiguous(),
                kinds=ops.kinds_tensor(kinds, dev), gt=gt, cls_host=cls_host,
                cls_dev=torch.tensor(cls_host, dtype=torch.int32, device=dev))


def torch_winding(verts, faces, queries):
    """w [B,Q] from torch ops in fp32, in query chunks: verts [B,P,3], faces [F,3], queries [Q,3]."""
    B, F, Q = verts.shape[0], faces.shape[0], queries.shape[0]
    c0, c1, c2 = (verts[:, faces[:, k].long()][:, None] for k in range(3))    # [B,1,F,3]
    chunk = max(1, int(PAIR_BUDGET // (B * F)))
    out = []
    for s in range(0, Q, chunk):
        x = queries[None, s:s + chunk, None, :]
        a, b, c = c0 - x, c1 - x, c2 - x
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        num = (a * torch.cross(b, c, dim=-1)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out.append(torch.atan2(num, den).sum(-1) / (2 * math.pi))
    return torch.cat(out, 1)


class ComposedLoop:
    """The metric of VolumeEvaluationMeter.update_mesh from torch ops, with host bookkeeping."""

    def __init__(self):
        self.total, self.class_sum, self.class_n, self.n = [0.0] * 5, [[0.0] * 5 for _ in range(CLASSES)], [0] * CLASSES, 0

    def update(self, inp, queries):
        gt = inp['gt']
        w_pred = torch_winding(inp['verts'], inp['faces'], queries)
        w_gt = torch.cat([torch_winding(gt.verts[gt.host['vert_offset'][s]:gt.host['vert_offset'][s + 1]][None],
                                        gt.faces[gt.host['face_offset'][s]:gt.host['face_offset'][s + 1]], queries) for s in range(len(gt))])
        p, g = w_pred > 0.5, w_gt > 0.5
        counts = torch.stack([(p & g).sum(1), (p | g).sum(1), p.sum(1), g.sum(1)], 1).double()
        Q = float(queries.shape[0])
        num = counts[:, [0, 0, 0, 2, 3]]
        den = torch.cat([counts[:, 1:4], torch.full_like(counts[:, :2], Q)], 1)
        rows = torch.where(den > 0, num / den.clamp_min(1), torch.zeros_like(num)).float()
        for k, v in enumerate(rows.double().sum(0).tolist()):                         # the batch sums: one read-back
            self.total[k] += v
        for b, cls in enumerate(inp['cls_host']):                                     # one read-back per sample, as `.item()` does
            for k, v in enumerate(rows[b].tolist()):
                self.class_sum[cls][k] += v
            self.class_n[cls] += 1
        self.n += len(inp['cls_host'])
        return counts, w_pred, w_gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=50)
    ap.add_argument('--composed-every', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'occupancy_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_occupancy.py needs a GPU: nothing is measured on a CPU')
    if args.rounds < 20:
        raise SystemExit('at least 20 rounds')
    dev = torch.device('cuda:0')
    names = ['c%d' % i for i in range(CLASSES)]
    lines = ['tools/time_occupancy.py --rounds %d --composed-every %d on one MI355X (torch %s): one evaluation batch of B samples, Q = %d^3, '
             'K = %d, predicted mesh V = 2048 / F = 4032, ragged ground truth of 2304 .. 2976 faces a mesh, %d classes; us, median [10th .. '
             '90th percentile] of %d rounds after 5 warm-up rounds (the composed loop in every %dth round); the variants alternate within a '
             'round; eager: host clock around the call and a device synchronise; replay: two device events'
             % (args.rounds, args.composed_every, torch.__version__, RESOLUTION, K, CLASSES, args.rounds, args.composed_every)]
    for B in (8, 64):
        inp = make_inputs(B, dev)
        meter, replayed_p, replayed_m = (vpn_amd.VolumeEvaluationMeter(names, dev, resolution=RESOLUTION) for _ in range(3))
        q = meter.queries
        F = inp['faces'].shape[0]
        prims = lambda m=meter: m.update_primitives(inp['params'], inp['kinds'], inp['gt'], inp['cls_dev'])
        mesh = lambda m=meter: m.update_mesh(inp['verts'], inp['faces'], inp['gt'], inp['cls_dev'])
        loop = ComposedLoop()
        composed = lambda: loop.update(inp, q)
        # results first: the same counts but for queries whose winding number is within 1e-3 of the threshold
        (_, counts_m), (counts_c, w_pred, w_gt) = mesh(), composed()
        unsure = (((w_pred - 0.5).abs() < 1e-3) | ((w_gt - 0.5).abs() < 1e-3)).sum(1)
        off = (counts_m.double() - counts_c).abs().max(1).values
        if bool((off > unsure).any()):
            raise SystemExit('B = %d: the meter and the composed loop disagree on the counts by %s with %s unsure queries'
                             % (B, off.tolist(), unsure.tolist()))
        g_prims, g_mesh = capture(lambda: prims(replayed_p)), capture(lambda: mesh(replayed_m))
        g_wind = capture(lambda: ops.winding_number(inp['verts'], inp['faces'], q))

        def host_timed(step):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6

        def replay_timed(graph):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3

        variants = {'primitives, eager': lambda: host_timed(prims), 'primitives, replay': lambda: replay_timed(g_prims),
                    'mesh, eager': lambda: host_timed(mesh), 'mesh, replay': lambda: replay_timed(g_mesh),
                    'winding, replay': lambda: replay_timed(g_wind), 'composed, eager': lambda: host_timed(composed)}
        samples = {k: [] for k in variants}
        for r in range(5 + args.rounds):
            for k, v in variants.items():
                if k == 'composed, eager' and r % args.composed_every:
                    continue
                t = v()
                if r >= 5:
                    samples[k].append(t)
        qs = {k: [float(torch.quantile(torch.tensor(v, dtype=torch.float64), p)) for p in (0.5, 0.1, 0.9)] for k, v in samples.items()}
        first = len(lines)
        lines.append('B = %d (counts agree but for at most %d unsure queries a sample)' % (B, int(unsure.max())))
        for k in variants:
            lines.append('    %-20s %11.1f us [%11.1f .. %11.1f]  (%d samples)' % (k, *qs[k], len(samples[k])))
        pairs = B * q.shape[0] * F
        lines.append('    winding alone: %d x %d x %d = %.3g (query, face) pairs, %.1f G pairs/s'
                     % (B, q.shape[0], F, pairs, pairs / qs['winding, replay'][0] / 1e3))
        spread = qs['mesh, replay'][2] - qs['mesh, replay'][1]
        ok = qs['mesh, eager'][0] <= qs['composed, eager'][0] + spread
        lines.append('    expectation (mesh, eager <= composed, eager + %.1f us, the spread of the replays): %s; the composed loop takes '
                     '%.2f x the eager meter, %.2f x the replay' % (spread, 'holds' if ok else 'DOES NOT HOLD', qs['composed, eager'][0] / qs['mesh, eager'][0],
                                                                    qs['composed, eager'][0] / qs['mesh, replay'][0]))
        print('\n'.join(lines[first:]), flush=True)
        del g_prims, g_mesh, g_wind
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
