"""Candidate form of the fp16 Chamfer scan (modes 6 and 7): a direction-1 workgroup serves 256 consecutive
sampled points, finds the ball that holds every target that can be nearest to (or tie for) one of them, and scans those
targets only; above 512 candidates, or with a bound that is not finite, it scans the whole cloud as before.  Nothing may
change a bit: every case compares the fp16 scan with brute force in dist1, idx1, dist2 and idx2.

Each case also counts the candidates of every workgroup on the CPU in fp64 by the kernel's rule and asserts that the
count lies well on one side of the cap (< 256 or > 1024), so the test knows which path a workgroup took."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_chamfer_skip import check_mode6, check_mode7, rand_params, same, vpn  # noqa: F401  (vpn: the module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CAP = 512                    # CCAND_CAP of vpn_chamfer_feat.h
WG = 256                     # queries per scan workgroup
N = 4096                     # the smallest cloud that takes the candidate form (CSKIP_MIN_TARGETS): 16 workgroups per sample


def cand_counts(p1, p2):
    """Candidates per workgroup [B, N / 256] by the kernel's rule, in fp64 on the fp32 inputs: c = the centre of the
    queries' box as the kernel stores it (fp32), rho = max |a - c|, d_c = min |b - c|, keep |b - c|^2 <= (2 rho + d_c)^2
    (1 + 3e-5).  inf where the bound is not finite (the workgroup scans everything)."""
    p1, p2 = p1.cpu().numpy(), p2.cpu().numpy()
    out = np.zeros((p1.shape[0], (p1.shape[1] + WG - 1) // WG))
    for b in range(p1.shape[0]):
        t = p2[b].astype(np.float64)
        for w in range(out.shape[1]):
            a = p1[b, w * WG:(w + 1) * WG]
            with np.errstate(all='ignore'):
                c = ((np.nanmin(a, 0) + np.nanmax(a, 0)) * np.float32(0.5)).astype(np.float64)
                rho = np.sqrt(((a.astype(np.float64) - c) ** 2).sum(1)).max()      # NaN if any query is
                d2 = ((t - c) ** 2).sum(1)
                R = 2 * rho + np.sqrt(np.nanmin(d2)) if np.isfinite(d2).any() else np.inf
                out[b, w] = np.inf if not np.isfinite(R) else (~(d2 > R * R * (1 + 3e-5))).sum()
    return out


def assert_sides(counts, expect):
    """Every workgroup well on one side of the cap; `expect`: 'cand' (all below), 'mixed' (both sides occur), or
    'full' (all above)."""
    low, high = counts < CAP / 2, counts > 2 * CAP
    assert (low | high).all(), 'a workgroup near the cap: %s' % counts[~(low | high)]
    if expect == 'cand':
        assert low.all(), counts
    elif expect == 'full':
        assert high.all(), counts
    else:
        assert low.any() and high.any(), counts


def blobs(gen, B, radius=0.08, n=N):
    """n / 256 blobs of 256 consecutive points per sample: centres in the cube, points inside a ball of `radius`."""
    g = n // WG
    centre = 0.7 * (torch.rand(B, g, 1, 3, generator=gen) - 0.5)
    d = torch.randn(B, g, WG, 3, generator=gen)
    d = d / d.norm(dim=3, keepdim=True) * radius * torch.rand(B, g, WG, 1, generator=gen) ** (1.0 / 3.0)
    return (centre + d).reshape(B, n, 3).contiguous()


def cube(gen, B, M):
    return torch.rand(B, M, 3, generator=gen) - 0.5


def run(vpn, p1, p2, what, expect, names=('dist1', 'idx1', 'dist2', 'idx2')):
    assert_sides(cand_counts(p1, p2), expect)
    check_mode6(vpn, p1.to(DEV), p2.to(DEV), what, names)


@pytest.mark.parametrize('B,M', [(1, 2048), (3, 700)])
def test_cand_blobs_in_a_uniform_cloud(vpn, B, M):
    """1. The C3 regime: compact blobs of 256 consecutive queries inside a uniform cloud."""
    gen = torch.Generator().manual_seed(100 + M)
    run(vpn, blobs(gen, B), cube(gen, B, M), 'blobs, M = %d' % M, 'cand')


def test_cand_and_fallback_share_a_launch(vpn):
    """2. The same blobs with some of them spread over the cube: candidate and full-scan workgroups in one launch."""
    gen = torch.Generator().manual_seed(2)
    p1, p2 = blobs(gen, 3), cube(gen, 3, 2048)
    p1[0, 5 * WG:6 * WG] = cube(gen, 1, WG)[0]
    p1[2, 0:WG] = cube(gen, 1, WG)[0]
    p1[2, 15 * WG:] = cube(gen, 1, WG)[0]
    run(vpn, p1, p2, 'blobs and spread workgroups', 'mixed')


def test_cand_duplicated_targets(vpn):
    """3. Duplicated ground-truth points at distant indices inside one candidate set: the lowest original index wins."""
    gen = torch.Generator().manual_seed(3)
    p1, p2 = blobs(gen, 3), cube(gen, 3, 2048)
    p2[:, 1700:2000] = p2[:, 0:300]
    p2[:, 900:1000] = p2[:, 1100:1200].flip(1)
    p1[:, 0:100] = p2[:, 0:100] + 1.0e-3            # queries whose nearest neighbour certainly has a twin
    run(vpn, p1, p2, 'duplicated targets', 'mixed' if (cand_counts(p1, p2) > CAP).any() else 'cand')


def lattice_case(gen, B=1, L=8):
    h = 1.0 / L
    ax = torch.arange(L, dtype=torch.float32) * h - 0.5
    lat = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(1, -1, 3).expand(B, -1, -1).contiguous()
    g = N // WG
    corner = torch.randint(2, L - 2, (B, g, 1, 3), generator=gen).float()            # a lattice point per workgroup
    # cell centres around it: 2 x 2 x 4 cells, each with 8 equidistant lattice corners; the box centre is the lattice point
    off = torch.stack([torch.randint(-1, 1, (B, g, WG), generator=gen), torch.randint(-1, 1, (B, g, WG), generator=gen),
                       torch.randint(-2, 2, (B, g, WG), generator=gen)], -1).float()
    q = (corner + off + 0.5) * h - 0.5
    return q.reshape(B, N, 3).contiguous(), lat


def test_cand_lattice_ties(vpn):
    """4. A lattice ground truth: every query has eight equidistant targets, far apart in index and so in different compact
    cells; the ties are resolved by the fix-up."""
    gen = torch.Generator().manual_seed(4)
    q, lat = lattice_case(gen)
    counts = cand_counts(q, lat)
    assert (counts > 64).all(), counts               # more than one compact cell of 64
    run(vpn, q, lat, 'lattice', 'cand')


def edge_case(gen, B=1):
    """Workgroup 0 of every sample: queries in the ball (c = 0, rho = 2^-4) that touch the box at +-rho on every axis, the
    nearest target to c at distance d_c = 2^-5 on the -x side, and targets on the sphere |b| = R = 2 rho + d_c within a few
    ulp either side (along +x: the nearest neighbour of the query at +rho x then lies on the edge of the ball and ties,
    to within those ulp, with the target nearest to c), nothing else within 0.3."""
    rho, dc = 0.0625, 0.03125
    R = 2 * rho + dc
    p1 = blobs(gen, B, radius=0.05)
    q = torch.randn(WG, 3, generator=gen)
    q = q / q.norm(dim=1, keepdim=True) * rho * torch.rand(WG, 1, generator=gen)
    q[0:6] = torch.tensor([[rho, 0, 0], [-rho, 0, 0], [0, rho, 0], [0, -rho, 0], [0, 0, rho], [0, 0, -rho]])
    q[6:16] = torch.tensor([rho, 0.0, 0.0]) * torch.linspace(0.9, 1.0, 10)[:, None]     # near the +x pole
    p1[:, 0:WG] = q
    far = cube(gen, B, 160)
    far = far / far.norm(dim=2, keepdim=True) * (0.3 + 0.2 * torch.rand(B, 160, 1, generator=gen))
    ulps = torch.tensor([-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0]) * 2.0 ** -24
    dirs = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0], [0.6, 0.8, 0.0]])
    edge = (dirs[:, None, :] * (R * (1.0 + ulps))[None, :, None]).reshape(-1, 3)            # 28 targets around the sphere
    near = torch.tensor([[-dc, 0.0, 0.0]])
    p2 = torch.cat([far[:, :80], edge.expand(B, -1, -1), far[:, 80:], near.expand(B, -1, -1)], 1).contiguous()
    return p1, p2


def test_cand_targets_on_the_ball_edge(vpn):
    """5. Targets on the sphere |b - c| = 2 rho + d_c to within a few ulp either side, and queries whose nearest targets
    sit at the edge of the ball."""
    gen = torch.Generator().manual_seed(5)
    p1, p2 = edge_case(gen, 3)
    run(vpn, p1, p2, 'ball edge', 'cand')


@pytest.mark.parametrize('M', [40, 777, 2047])
def test_cand_ragged_targets(vpn, M):
    """6. M below 64 and not a multiple of 64."""
    gen = torch.Generator().manual_seed(60 + M)
    run(vpn, blobs(gen, 3), cube(gen, 3, M), 'M = %d' % M, 'cand')


def one_candidate_case(gen, B=1):
    p1 = blobs(gen, B, radius=0.01)
    p2 = cube(gen, B, 300)
    p2 = p2 / p2.norm(dim=2, keepdim=True) * (0.45 + 0.05 * torch.rand(B, 300, 1, generator=gen))    # a shell
    p1[:, 0:WG] = 0.01 * (torch.rand(B, WG, 3, generator=gen) - 0.5)
    p2[:, 217] = torch.tensor([0.004, -0.002, 0.001])                                                  # the only target near workgroup 0
    return p1, p2


def test_cand_single_candidate(vpn):
    """6. A workgroup with exactly one candidate."""
    gen = torch.Generator().manual_seed(66)
    p1, p2 = one_candidate_case(gen, 3)
    counts = cand_counts(p1, p2)
    assert (counts[:, 0] == 1).all(), counts
    run(vpn, p1, p2, 'one candidate', 'cand')


@pytest.mark.parametrize('shift,scale', [((7.5, 0.0, 0.0), 1.0), ((7.5, 7.5, -7.5), 1.0), ((0.0, 0.0, 0.0), 9.0),
                                         ((0.0, 0.0, 0.0), 1000.0)])
def test_cand_translated_and_scaled(vpn, shift, scale):
    """7. Coordinates near 7.5 (their ulp far above the ulp of the distances; all three shifted: outside the fp16
    filter's domain as well), and clouds scaled x9 and x1000 (outside the domain)."""
    gen = torch.Generator().manual_seed(70 + int(scale))
    t = torch.tensor(shift)
    p1, p2 = (blobs(gen, 1) + t) * scale, (cube(gen, 1, 1500) + t) * scale
    run(vpn, p1.contiguous(), p2.contiguous(), 'shift %s scale %g' % (shift, scale), 'cand')


def test_cand_nan_and_inf(vpn):
    """8. NaN and inf in a query and in a target (distances only, as in the skip test: the filter's minimum tree does not
    order NaN the way brute force does).  A workgroup with such a query has no finite bound and scans everything."""
    gen = torch.Generator().manual_seed(8)
    p1, p2 = blobs(gen, 3), cube(gen, 3, 1500)
    p1[0, 300, 1] = math.nan
    p1[1, 4000] = math.inf
    p1[2, 77, 0] = -math.inf
    p2[0, 17, 2] = math.nan
    p2[1, 1000:1003] = math.nan
    p2[2, 5] = math.inf
    counts = cand_counts(p1, p2)
    assert np.isinf(counts[0, 1]) and np.isinf(counts[1, 15]) and np.isinf(counts[2, 0]), counts
    assert (counts[np.isfinite(counts)] < CAP / 2).all(), counts
    check_mode6(vpn, p1.to(DEV), p2.to(DEV), 'NaN and inf', names=('dist1', 'dist2'))


def test_cand_mode7_sampled(vpn):
    """9. Mode 7: the features written by the sampler's launch, B = 3, K = 16 primitives of n = 256 points (one per
    workgroup), a uniform ground truth of 700 points."""
    gen = torch.Generator().manual_seed(9)
    B, K, n, M = 3, 16, 256, 700
    params = rand_params(gen, B, K).to(DEV)
    kinds = vpn.kinds_tensor([1] * 5 + [0] * 11, torch.device(DEV))
    gt = cube(gen, B, M).to(DEV)
    pts = check_mode7(vpn, params, kinds, n, gt, 'mode 7, K = 16, n = 256')
    assert_sides(cand_counts(pts, gt), 'cand')


CHILD = r'''
import sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import vpn_amd
from test_chamfer_candidates import blobs, cube
from test_chamfer_skip import check_mode6
gen = torch.Generator().manual_seed(101)
check_mode6(vpn_amd, blobs(gen, 3).cuda(), cube(gen, 3, 2048).cuda(), 'switch off')
print('SWITCH-OFF-OK')
'''


def test_cand_switched_off(vpn):
    """VPN_CHAMFER_CAND=0 (read once per process: a child) runs the parent's scan on the blobs of case 1."""
    env = dict(os.environ, VPN_CHAMFER_CAND='0')
    r = subprocess.run([sys.executable, '-c', CHILD % (ROOT, os.path.join(ROOT, 'tests'))], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'SWITCH-OFF-OK' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
