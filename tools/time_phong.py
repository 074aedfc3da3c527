"""Time a dump of 20 Phong views of one mesh at 128 x 128 on one GPU against the colour turntable of the same mesh.

  phong      PhongRenderer.views(mesh, cams, uv, texture, 128): projection + Phong launch for all 20 views, then the
             silhouette launch (VertexRenderer.triangle_alpha) for the alpha channel
  turntable  Visualizer.turntable(mesh, cams, 128): the same projection and the same tile walk, vertex colours in place of
             texture and lighting, uint8 output (the yardstick: it existed before the Phong renderer)
  alpha      the silhouette launch alone

Shapes: the composed meshes of K = 16 and K = 64 ellipsoids (4032 and 16128 faces), one atlas texel per primitive.  Twice:
`host` is the host time of `--inner` consecutive dumps, each ending in the device-to-host copy of what it rendered (the
Phong side copies float RGB + alpha, 16 bytes a pixel; the turntable 3), divided by `--inner`; `device` is a HIP-event pair
around `--inner` dumps without the copies.  Every side is warmed up at every shape; the sides alternate per repetition;
median and the 10th..90th percentile.  Expectation: phong <= turntable + alpha, within the wider of the two sides' spreads.

    python tools/time_phong.py [--reps 10] [--inner 3] [--out FILE.txt]
    python tools/time_phong.py --once      # one dump of each side at 16128 faces (for a kernel trace)"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vpn_amd  # noqa: E402
from vpn_amd import Meshing, PhongRenderer, TriangleMesh, VertexRenderer, Visualizer, merge_meshes  # noqa: E402

DEV = 'cuda'
SIZE = 128
VIEWS = 20


def make(K):
    g = torch.Generator().manual_seed(K)
    v = 0.06 + 0.14 * torch.rand(1, K, 3, generator=g) if K > 16 else 0.10 + 0.20 * torch.rand(1, K, 3, generator=g)
    p = torch.cat([v, torch.rand(1, K, 4, generator=g), 0.35 * (torch.rand(1, K, 3, generator=g) * 2 - 1)], 2).to(DEV)
    kinds = [vpn_amd.SPHERE] * K                                       # 252 faces each: 4032 and 16128 faces
    verts, _ = Meshing.mesh_primitives(p, kinds)
    parts, n0 = [], 0
    for kind in kinds:
        tv, tf = Meshing.template(kind, torch.device(DEV))
        parts.append(TriangleMesh(verts[0, n0:n0 + tv.shape[0]].contiguous(), tf))
        n0 += tv.shape[0]
    mesh, uv, texture = merge_meshes(parts, colors=torch.rand(K, 3, generator=g))
    mesh.faces = vpn_amd.ops.faces_i32(mesh.faces, DEV)
    cams = torch.stack([3.0 + 2.0 * torch.rand(VIEWS, generator=g), (torch.rand(VIEWS, generator=g) - 0.5) * 90,
                        torch.rand(VIEWS, generator=g) * 360], 1).to(DEV)
    return mesh, uv, texture, cams


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


def sides_of(mesh, uv, texture, cams):
    meshes = [mesh] * VIEWS
    return {
        'phong': lambda: PhongRenderer.views(mesh, cams, uv, texture, img_size=SIZE),
        'turntable': lambda: (Visualizer.turntable(mesh, cams, image_size=SIZE),),
        'alpha': lambda: (VertexRenderer.triangle_alpha(meshes, cams[:, 0], cams[:, 1], cams[:, 2], SIZE, SIZE)[0],),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--inner', type=int, default=3)
    ap.add_argument('--out', default='', help='also write the printed lines to this file')
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'timing needs the GPU'
    if args.once:
        for fn in sides_of(*make(64)).values():
            [t.cpu() for t in fn()]
        torch.cuda.synchronize()
        return
    lines = ['tools/time_phong.py --reps %d --inner %d on one MI355X: one mesh, %d views of %d x %d pixels; ms per dump, median '
             '[10th .. 90th percentile] of %d samples of %d consecutive dumps; the sides alternate' % (args.reps, args.inner, VIEWS, SIZE, SIZE, args.reps, args.inner)]
    print(lines[0], flush=True)
    for K in (16, 64):
        mesh, uv, texture, cams = make(K)
        sides = sides_of(mesh, uv, texture, cams)
        for _ in range(2):
            for fn in sides.values():
                [t.cpu() for t in fn()]
        torch.cuda.synchronize()
        for mode, timed in (('host', lambda fn: host_timed(lambda: [t.cpu() for t in fn()], args.inner)), ('device', lambda fn: device_timed(fn, args.inner))):
            ts = {k: [] for k in sides}
            for _ in range(args.reps):
                for k, fn in sides.items():
                    ts[k].append(timed(fn))
            s = {k: spread(v) for k, v in ts.items()}
            allowed = max(s['phong'][2] - s['phong'][1], s['turntable'][2] - s['turntable'][1])
            excess = s['phong'][0] - (s['turntable'][0] + s['alpha'][0])
            line = 'faces=%-5d %-6s ' % (mesh.faces.shape[0], mode) + '   '.join('%s %7.3f ms [%.3f .. %.3f]' % ((k,) + s[k]) for k in sides)
            line += '   phong - (turntable + alpha) = %+.3f ms, wider spread %.3f ms: %s' % (excess, allowed, 'within' if excess <= allowed else 'SLOWER')
            lines.append(line)
            print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
