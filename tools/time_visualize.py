"""Time the visual dump of one sample on one GPU: the stage against what a user of the code before it had to do.

  stage      Visualizer.frames_vp_meshes(image, pack): all 13 / 37 views in ONE launch into the frame strip on the device,
             then ONE device-to-host copy of the strip (what render_vp_meshes does before PIL)
  baseline   the loop shape of visualize/render.py:18-21 on the renderer that existed before the stage: one
             VertexRenderer.render(pack, dist, elev, azim, image_size=(256, 256)) per view, each followed by .cpu().
             Timing material only: it yields one-colour soft silhouettes, no occlusion, no strip.
  and the same pair for triangle meshes: Visualizer.frames_vp_meshes on meshes whose vertices were edited (projection + render
  launch) against VertexRenderer.render_triangles per view.

Shapes: K = 16 and K = 64 primitives (composed meshes of 4032 and 16128 faces), 13 views (one elevation) and 37 views (three).
Every sample is the host time of `--inner` consecutive dumps, each ending in its device-to-host copy (both sides synchronise
by themselves through that copy), divided by `--inner`; every side is warmed up at every shape; the sides alternate per
repetition; median and the 10th..90th percentile.  The device time of the stage's launches alone is taken with a HIP-event
pair around `--inner` calls of frames_vp_meshes without the copy.

    python tools/time_visualize.py [--reps 20] [--inner 5] [--out FILE.txt]
    python tools/time_visualize.py --once      # one dump of each kind at K = 64, 37 views (for a kernel trace)"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vpn_amd  # noqa: E402
from vpn_amd import Meshing, PrimitivePack, TriangleMesh, VertexRenderer, Visualizer  # noqa: E402

DEV = 'cuda'
SIZE = 256


def make(K):
    g = torch.Generator().manual_seed(K)
    v = 0.06 + 0.14 * torch.rand(1, K, 3, generator=g) if K > 16 else 0.10 + 0.20 * torch.rand(1, K, 3, generator=g)
    p = torch.cat([v, torch.rand(1, K, 4, generator=g), 0.35 * (torch.rand(1, K, 3, generator=g) * 2 - 1)], 2).to(DEV)
    kinds = [vpn_amd.CUBOID] * (K // 4) + [vpn_amd.SPHERE] * (K - K // 4)
    pack = PrimitivePack(p, kinds)
    verts, faces = Meshing.mesh_primitives(p, kinds)
    # the K meshes of the sample with edited vertices: what the triangle path of the dump takes
    meshes, n0 = [], 0
    for k, kind in enumerate(kinds):
        tv, tf = Meshing.template(kind, torch.device(DEV))
        meshes.append(TriangleMesh((verts[0, n0:n0 + tv.shape[0]] * 1.0).contiguous(), tf))
        n0 += tv.shape[0]
    composed = TriangleMesh(verts[0].contiguous(), vpn_amd.ops.faces_i32(faces, DEV))
    image = torch.rand(3, 137, 137, generator=g).to(DEV)
    return image, pack, meshes, composed


def views(three, dist=2.0):
    elevs = (-30, 0, 30) if three else (0,)
    return [(dist, 0, 0)] + [(dist, e, a) for a in range(0, 360, 30) for e in elevs]


def host_timed(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def device_timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def spread(ts):
    q = statistics.quantiles(ts, n=10)
    return statistics.median(ts), q[0], q[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--out', default='', help='also write the printed lines to this file')
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'timing needs the GPU'
    if args.once:
        image, pack, meshes, _ = make(64)
        Visualizer.frames_vp_meshes(image, pack, is_three_elev=True).cpu()
        Visualizer.frames_vp_meshes(image, meshes, is_three_elev=True).cpu()
        torch.cuda.synchronize()
        return
    lines = ['tools/time_visualize.py --reps %d --inner %d on one MI355X: one sample, %d x %d pixels per view; ms per dump,'
             % (args.reps, args.inner, SIZE, SIZE),
             'median [10th .. 90th percentile] of %d samples, each the host time of %d consecutive dumps with their device-to-host '
             'copies; the sides alternate' % (args.reps, args.inner)]
    print('\n'.join(lines), flush=True)
    for K in (16, 64):
        image, pack, meshes, composed = make(K)
        for three in (False, True):
            vs = views(three)
            sides = {
                'stage': lambda: Visualizer.frames_vp_meshes(image, pack, is_three_elev=three).cpu(),
                'baseline': lambda: [VertexRenderer.render(pack, d, e, a, image_size=(SIZE, SIZE))[0].cpu() for d, e, a in vs],
                'stage_mesh': lambda: Visualizer.frames_vp_meshes(image, meshes, is_three_elev=three).cpu(),
                'baseline_mesh': lambda: [VertexRenderer.render_triangles(composed, d, e, a, image_size=(SIZE, SIZE))[0].cpu() for d, e, a in vs],
            }
            for _ in range(2):
                for fn in sides.values():
                    fn()
            torch.cuda.synchronize()
            ts = {k: [] for k in sides}
            for _ in range(args.reps):
                for k, fn in sides.items():
                    ts[k].append(host_timed(fn, args.inner))
            s = {k: spread(v) for k, v in ts.items()}
            dev_p = device_timed(lambda: Visualizer.frames_vp_meshes(image, pack, is_three_elev=three), args.inner)
            dev_m = device_timed(lambda: Visualizer.frames_vp_meshes(image, meshes, is_three_elev=three), args.inner)
            head = 'K=%-2d views=%-2d  ' % (K, len(vs))
            for a, b, dv, launches in (('stage', 'baseline', dev_p, '1 render launch'), ('stage_mesh', 'baseline_mesh', dev_m, 'projection + render launch')):
                line = head + '%-10s %8.3f ms [%.3f .. %.3f]   %-13s %8.3f ms [%.3f .. %.3f]   %s / %s x%.2f   stage on the device without the copy %.3f ms (%s; the baseline makes %d render calls)' % (
                    (a,) + s[a] + (b,) + s[b] + (b, a, s[b][0] / s[a][0], dv, launches, len(vs)))
                lines.append(line)
                print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
