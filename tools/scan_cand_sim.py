"""How many targets does a direction-1 workgroup of the Chamfer scan still have to scan in its candidate form (DESIGN
4.1)?  CPU simulation in fp64 of the kernel's rule on the step's clouds: per workgroup of 256 consecutive sampled points
c = the centre of their box, rho = max |a - c|, d_c = the distance from c to its nearest ground-truth point, candidates =
the ground-truth points within 2 rho + d_c of c; above the cap of 512 the workgroup scans everything.  Every query's true
nearest neighbour is checked to lie inside its workgroup's candidate set.
    python tools/scan_cand_sim.py > profiles/r06_scan_cand_sim.txt"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import vpn_oracle as O
import bench

CAP, WG = 512, 256


def sample(params, K, n, seed):
    return O.sample_primitives(params, [0] * K, O.philox_uniforms(seed, 0, params.shape[0], K, n)).numpy().astype(np.float64)


def sim(name, pts, gt):
    counts, scanned, missed = [], 0, 0
    M = gt.shape[1]
    for b in range(pts.shape[0]):
        for w0 in range(0, pts.shape[1], WG):
            a = pts[b, w0:w0 + WG]
            c = ((a.min(0) + a.max(0)) * 0.5).astype(np.float32).astype(np.float64)
            rho = np.sqrt(((a - c) ** 2).sum(1)).max()
            dc2 = ((gt[b] - c) ** 2).sum(1)
            R = 2 * rho + np.sqrt(dc2.min())
            keep = dc2 <= R * R * (1 + 3e-5)
            nn = ((a[:, None, :] - gt[b][None, :, :]) ** 2).sum(2).argmin(1)
            missed += int((~keep[nn]).sum())
            k = int(keep.sum())
            counts.append(k)
            scanned += min((k + 63) // 64 * 64, (M + 63) // 64 * 64) if k <= CAP else (M + 63) // 64 * 64
    c = np.array(counts)
    print('%-58s candidates of M = %d: mean %.0f p90 %.0f p99 %.0f max %d | scanned (padded to 64, cap %d) %.3f of M | '
          'workgroups above the cap %.1f %% | nearest neighbours outside their set: %d'
          % (name, M, c.mean(), np.percentile(c, 90), np.percentile(c, 99), c.max(), CAP, scanned / (len(c) * M),
             100.0 * (c > CAP).mean(), missed))


B = int(os.environ.get('B', 8))
params, gt = bench.synth_inputs(B, 32, 2048, 1234, 'cpu')
pts = sample(params, 32, 256, 1234)
sim('C3 (K = 32, n = 256), GT uniform in the cube (headline)', pts, gt.numpy().astype(np.float64))
gen = torch.Generator().manual_seed(7)
moved = params.clone()
moved[..., 0:3] *= 1.0 + 0.2 * (torch.rand(moved[..., 0:3].shape, generator=gen) - 0.5)       # sizes +-10 %
moved[..., 7:10] += 0.03 * (torch.rand(moved[..., 7:10].shape, generator=gen) - 0.5)          # centres +-0.015
sim('C3, GT on the surfaces of perturbed target primitives', pts, sample(moved, 32, 64, 7))
p64, g64 = bench.synth_inputs(B, 64, 2048, 1234, 'cpu')
sim('K = 64, n = 32 (a workgroup spans 8 primitives; N = 2048)', sample(p64, 64, 32, 1234), g64.numpy().astype(np.float64))
p16, g16 = bench.synth_inputs(B, 16, 2048, 1234, 'cpu')
sim('K = 16, n = 128 (reference default shape; N = 2048)', sample(p16, 16, 128, 1234), g16.numpy().astype(np.float64))
print('(the last two shapes have N = 2048 < CSKIP_MIN_TARGETS: the host rule keeps them on the full scan; shown for the geometry only)')
