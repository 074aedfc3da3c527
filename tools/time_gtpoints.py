"""Time the ground-truth stage on one GPU against the only way the code before it could do the same work: gt_points (n = 2048,
two sets over one cumulative-area table, three launches a batch) on S = 64 synthetic meshes of different sizes, and a loop
of TriangleMesh.sample(2048) per mesh and per point set (two launches each) followed by one obj_to_view_points call, in the
same process on the same meshes.  Workloads (subdivided icospheres, vertices jittered, the face list cut to the wanted
length; no dataset needed):
  (a) face counts log-uniform in 2e2 .. 4e5;
  (b) one mesh of 4e5 faces beside 63 meshes of 1e3 faces.
Device events around every whole batch after a warm-up; median and the 10th..90th percentile spread; the kernels' own
times from the library's launch profile in a separate pass.  The first timed batches can still run below the steady clock:
the spread shows it, the median is what to read.  Packing (host) and the upload are on neither side.

    python tools/time_gtpoints.py [--reps 20] [--meshes 64] [--out profiles/gtpoints_time.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.set_num_threads(min(16, torch.get_num_threads()))
import vpn_amd  # noqa: E402

N = 2048


def icosphere_faces(sub):
    """Vertices [P,3] float64 and faces [F,3] int64 of an icosahedron subdivided `sub` times (20 * 4^sub faces), vectorised."""
    t = (1.0 + 5 ** 0.5) / 2
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                  [9, 8, 1]], np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(sub):
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
        uniq, inv = np.unique(e[:, 0] * len(v) + e[:, 1], return_inverse=True)
        m = v[uniq // len(v)] + v[uniq % len(v)]
        mid = len(v) + inv.reshape(3, -1)                              # midpoints of (ab, bc, ca) per face
        v = np.concatenate([v, m / np.linalg.norm(m, axis=1, keepdims=True)])
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        ab, bc, ca = mid
        f = np.concatenate([np.stack(x, 1) for x in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    return v, f


def synthetic_mesh(F, rng, cache):
    sub = 0
    while 20 * 4 ** sub < F:
        sub += 1
    if sub not in cache:
        cache[sub] = icosphere_faces(sub)
    v, f = cache[sub]
    f = f[rng.permutation(len(f))[:F]]
    used, local = np.unique(f, return_inverse=True)                    # keep the vertices the cut list uses
    v = v[used] * rng.uniform(0.3, 0.6) * rng.uniform(0.5, 1.5, 3) + rng.normal(0, 1e-3, (len(used), 3))
    return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(local.reshape(-1, 3).astype(np.int64))


def spread(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[len(ts) // 10], ts[(len(ts) * 9) // 10]


def timed(call, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return spread(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--meshes', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_gtpoints.py measures on a GPU; none is visible')
    S, rng, cache = args.meshes, np.random.default_rng(0), {}
    work = {'a': np.round(np.exp(rng.uniform(np.log(2e2), np.log(4e5), S))).astype(int).tolist(),
            'b': [400000] + [1000] * (S - 1)}
    lines = ['ground-truth stage: S = %d meshes, n = %d, 2 sets (canonical + view-centred); %d reps; medians (10th .. 90th percentile)'
             % (S, N, args.reps)]
    dists = torch.from_numpy(rng.uniform(0.8, 1.8, S).astype(np.float32)).cuda()
    elevs = torch.from_numpy(rng.uniform(-20, 40, S).astype(np.float32)).cuda()
    azims = torch.from_numpy(rng.uniform(0, 360, S).astype(np.float32)).cuda()
    for name, counts in work.items():
        meshes = [synthetic_mesh(F, rng, cache) for F in counts]
        batch = vpn_amd.MeshBatch.pack(meshes, 'cuda')
        tms = [vpn_amd.TriangleMesh(v.cuda(), f.int().cuda()) for v, f in meshes]     # int32 faces: no conversion in the loop

        def new():
            return vpn_amd.gt_points(batch, dists, elevs, azims, n=N, seed=1)

        def old():
            canon = torch.stack([m.sample(N, seed=1)[0] for m in tms])
            view = torch.stack([m.sample(N, seed=2)[0] for m in tms])
            return canon, vpn_amd.obj_to_view_points(view, dists, elevs, azims)

        for call in (new, old):
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        t_new, t_old = [], []
        for _ in range(2):                                             # alternate the two sides
            t_new.append(timed(new, args.reps))
            t_old.append(timed(old, max(3, args.reps // 2)))
        g, h = min(t_new), min(t_old)
        lines.append('(%s) %d faces in all, largest %d, %d chunks: gt_points %.3f ms (%.3f .. %.3f), %d library launches | '
                     'per-mesh loop %.3f ms (%.3f .. %.3f), %d library launches | ratio %.1fx'
                     % (name, sum(counts), max(counts), batch.chunks.size(0), g[0], g[1], g[2], vpn_amd.ops.RAGGED_LAUNCHES,
                        h[0], h[1], h[2], 4 * S + 1, h[0] / g[0]))
        with vpn_amd._lib.KernelProfile() as kp:
            new()
            torch.cuda.synchronize()
        for k, (n, ms) in sorted(kp.summary().items()):
            lines.append('      %-24s %d x %.4f ms' % (k, n, ms))
        with vpn_amd._lib.KernelProfile() as kp:
            old()
            torch.cuda.synchronize()
        for k, (n, ms) in sorted(kp.summary().items()):
            lines.append('      %-24s %d x %.4f ms (per-mesh loop)' % (k, n, ms))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
