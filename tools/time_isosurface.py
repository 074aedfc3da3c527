"""Time the outer-surface extraction (csrc/isosurface.hip) on one MI355X: B = 8 and B = 64 samples, K = 16
primitives of the benchmark's parameter distribution (half cuboids, translations 0.15 U(-1,1)), lattices of N = 64 and N = 128
nodes a side.  Writes profiles/isosurface_time.txt.

    python tools/time_isosurface.py [--rounds 30] [--out profiles/isosurface_time.txt]

Variants, on the same inputs:
  field, replay                 ops.primitive_field on the N^3 lattice (one launch);
  extraction, replay            ops.isosurface of that field (four launches); the four kernels one by one from the library's
                                own event pairs (_lib.KernelProfile, mean of the profiled calls);
  union_meshes, replay          lattice -> field -> extraction;
  update_primitives, eager / replay   SurfaceEvaluationMeter.update_primitives with n = 2048 points a sample against 2048
                                ground-truth points: union_meshes, the ragged sampler, the nearest-neighbour scan, the bookkeeping;
  host, eager                   what a user must do without the operator: copy the field to the host and run the vectorised
                                numpy restatement (tests/isosurface_ref.py, fp32) -- for ONE sample, times B (stated as such).
Eager variants: the host clock around the call and a device synchronise; replays: two device events.  The variants alternate
within every round; reported is the median [10th .. 90th percentile] of `rounds` rounds after 3 warm-up rounds; the host variant
runs in every `--host-every`-th round only.  Beside the times: the bytes the extraction must move (the field read once, the
cell -> vertex table written for the active cells, the outputs written whole) over the HBM peak of 8 TB/s.  There is no speed
bar; the expectation stated and checked in the output is that the extraction is cheaper than the field that feeds it.  No GPU:
the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import vpn_amd  # noqa: E402
from vpn_amd import _lib, ops  # noqa: E402
import isosurface_ref as IR  # noqa: E402
from time_trunknorm import capture  # noqa: E402

CLASSES, K, POINTS = 13, 16, 2048
HBM_PEAK = 8e12                          # bytes per second


def make_inputs(B, dev):
    g = torch.Generator().manual_seed(1234)
    v = (torch.rand(B, K, 3, generator=g) + 0.1) / torch.tensor([8.0, 10.0, 10.0])
    q = torch.rand(B, K, 4, generator=g)
    t = 0.15 * (torch.rand(B, K, 3, generator=g) * 2 - 1)
    kinds = [vpn_amd.CUBOID] * (K // 2) + [vpn_amd.SPHERE] * (K - K // 2)
    gt = (torch.rand(B, POINTS, 3, generator=g) - 0.5) * 0.6
    return dict(params=torch.cat([v, q, t], 2).float().to(dev).contiguous(), kinds=ops.kinds_tensor(kinds, dev), gt=gt.to(dev),
                cls=torch.tensor([b % CLASSES for b in range(B)], dtype=torch.int32, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=30)
    ap.add_argument('--host-every', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'isosurface_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/time_isosurface.py needs a GPU: nothing is measured on a CPU')
    if args.rounds < 20:
        raise SystemExit('at least 20 rounds')
    dev = torch.device('cuda:0')
    names = ['c%d' % i for i in range(CLASSES)]
    lines = ['tools/time_isosurface.py --rounds %d --host-every %d on one MI355X (torch %s): K = %d primitives (half cuboids, translations '
             '0.15 U(-1,1)), N^3 lattice on [-0.5, 0.5]^3, default capacities 8 N^2 / 16 N^2, n = %d sampled against %d ground-truth points, %d '
             'classes; us, median [10th .. 90th percentile] of %d rounds after 3 warm-up rounds (the host variant in every %dth round); the '
             'variants alternate within a round; eager: host clock around the call and a device synchronise; replay: two device events; the '
             'four kernels: mean of the library\'s own event pairs over 10 profiled calls'
             % (args.rounds, args.host_every, torch.__version__, K, POINTS, POINTS, CLASSES, args.rounds, args.host_every)]
    for B in (8, 64):
        for N in (64, 128):
            inp = make_inputs(B, dev)
            cx, cy, cz, nodes = ops.lattice(N, device=dev)
            field = ops.primitive_field(inp['params'], inp['kinds'], nodes).view(B, N, N, N)
            surface = ops.isosurface(field, (cx, cy, cz))
            counts = surface.counts.cpu()
            if bool(counts[:, 3].any()):
                raise SystemExit('B = %d, N = %d: a sample overflows the default capacities: %s' % (B, N, counts.tolist()))
            # results first: sample 0 against the fp32 restatement, bit for bit
            host_field = field[0].cpu().numpy()
            coords = (cx.cpu().numpy(), cy.cpu().numpy(), cz.cpu().numpy())
            ref = IR.surface_nets(host_field, coords, 0.0, np.float32)
            nv, nf = int(counts[0, 0]), int(counts[0, 1])
            if (ref['verts'].shape[0], ref['faces'].shape[0]) != (nv, nf) or not np.array_equal(surface.faces[0, :nf].cpu().numpy(), ref['faces']) \
                    or not np.array_equal(surface.verts[0, :nv].cpu().numpy(), ref['verts']):
                raise SystemExit('B = %d, N = %d: the extraction differs from the restatement' % (B, N))
            eager_meter, replay_meter = (vpn_amd.SurfaceEvaluationMeter(names, dev) for _ in range(2))
            update = lambda m: m.update_primitives(inp['params'], inp['kinds'], inp['gt'], inp['cls'], resolution=N, n=POINTS, seed=3)
            g_field = capture(lambda: ops.primitive_field(inp['params'], inp['kinds'], nodes))
            g_iso = capture(lambda: ops.isosurface(field, (cx, cy, cz)))
            g_union = capture(lambda: vpn_amd.Meshing.union_meshes(inp['params'], inp['kinds'], resolution=N))
            g_update = capture(lambda: update(replay_meter))
            with _lib.KernelProfile() as kp:
                for _ in range(10):
                    ops.isosurface(field, (cx, cy, cz))
            kernels = kp.summary()

            def host():
                f = field.cpu().numpy()
                IR.surface_nets(f[0], coords, 0.0, np.float32)

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

            variants = {'field, replay': lambda: replay_timed(g_field), 'extraction, replay': lambda: replay_timed(g_iso),
                        'union_meshes, replay': lambda: replay_timed(g_union),
                        'update_primitives, eager': lambda: host_timed(lambda: update(eager_meter)),
                        'update_primitives, replay': lambda: replay_timed(g_update), 'host, eager': lambda: host_timed(host)}
            samples = {k: [] for k in variants}
            for r in range(3 + args.rounds):
                for k, v in variants.items():
                    if k == 'host, eager' and r % args.host_every:
                        continue
                    t = v()
                    if r >= 3:
                        samples[k].append(t)
            qs = {k: [float(torch.quantile(torch.tensor(v, dtype=torch.float64), p)) for p in (0.5, 0.1, 0.9)] for k, v in samples.items()}
            first = len(lines)
            per_n2 = counts[:, 0].double().mean().item() / (N * N)
            lines.append('B = %d, N = %d (%.2f vertices and %.2f faces per N^2 a sample on average, open edges %d, sample 0 equals the fp32 '
                         'restatement bit for bit)' % (B, N, per_n2, counts[:, 1].double().mean().item() / (N * N), int(counts[:, 2].sum())))
            for k in variants:
                note = '  (one sample\'s restatement; x %d samples: %.0f us)' % (B, qs[k][0] * B) if k == 'host, eager' else ''
                lines.append('    %-28s %11.1f us [%11.1f .. %11.1f]  (%d samples)%s' % (k, *qs[k], len(samples[k]), note))
            for name in ('iso_count_kernel', 'iso_scan_kernel', 'iso_vertex_kernel', 'iso_face_kernel'):
                hit = [v for key, v in kernels.items() if name in key]
                lines.append('    %-28s %11.1f us  (mean of %d calls)' % (name, hit[0][1] * 1e3, hit[0][0]) if hit else '    %-28s not profiled' % name)
            max_verts, max_faces = surface.verts.shape[1], surface.faces.shape[1]
            moved = B * (N ** 3 * 4 + max_verts * 12 + max_faces * 12 + 16) + int(counts[:, 0].sum()) * 4
            floor = moved / HBM_PEAK * 1e6
            lines.append('    bytes the extraction must move: %.1f MB, %.1f us at 8 TB/s; the extraction takes %.1f x that'
                         % (moved / 1e6, floor, qs['extraction, replay'][0] / floor))
            ok = qs['extraction, replay'][0] <= qs['field, replay'][0]
            lines.append('    expectation (extraction <= field): %s, the extraction takes %.2f x the field; the host route takes %.0f x '
                         'union_meshes' % ('holds' if ok else 'DOES NOT HOLD', qs['extraction, replay'][0] / qs['field, replay'][0],
                                           qs['host, eager'][0] * B / qs['union_meshes, replay'][0]))
            print('\n'.join(lines[first:]), flush=True)
            del g_field, g_iso, g_union, g_update, field, surface
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
