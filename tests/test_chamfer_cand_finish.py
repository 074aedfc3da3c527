"""Prologue and finish of a candidate workgroup of the fp16 Chamfer scan (modes 6 and 7): the centre of its
ball comes from the stored tile box of its queries when that box is finite, and the candidate loop tracks cells of 16
compact positions, of which the exact finish evaluates four per lane.  None of it may change a bit: every case compares
the fp16 scan with brute force in dist1, idx1, dist2 and idx2, and asserts on the CPU in fp64 which side of the cap each
workgroup is on.  (The cases of section 3 were written for a prologue that keeps its targets in registers up to 2048
points and reads the planes twice above; that form did not pay and is not built -- DESIGN 8 -- the sizes either side of
that threshold stay as cases of the compaction passes.)"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_chamfer_candidates import CAP, N, WG, assert_sides, blobs, cand_counts, cube
from test_chamfer_skip import check_mode6, check_mode7, rand_params, same, vpn  # noqa: F401  (vpn: the module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def kept(a, t):
    """The targets `t` [M, 3] that the workgroup with the queries `a` [<= 256, 3] keeps, by the rule of cand_counts."""
    a, t = a.numpy(), t.numpy().astype(np.float64)
    c = ((a.min(0) + a.max(0)) * np.float32(0.5)).astype(np.float64)
    rho = np.sqrt(((a.astype(np.float64) - c) ** 2).sum(1)).max()
    d2 = ((t - c) ** 2).sum(1)
    R = 2 * rho + np.sqrt(d2.min())
    return ~(d2 > R * R * (1 + 3e-5))


def ball(gen, n, rho):
    """n points in the ball of radius rho around 0 that touch its box on every axis (box centre 0, max |a| = rho)."""
    d = torch.randn(n, 3, generator=gen)
    d = d / d.norm(dim=1, keepdim=True) * 0.9 * rho * torch.rand(n, 1, generator=gen) ** (1.0 / 3.0)
    d[n - 6:] = rho * torch.tensor([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    return d


# compact positions of the near-tied pairs: same span of 16 but the other half-wave; same half-wave, next row group;
# adjacent spans; adjacent blocks; adjacent pairs of blocks; first against last
PAIRS = [(3, 4), (7, 8), (15, 16), (31, 32), (63, 64), (0, 127)]
TWEAK = [0, 1, -1, 2, -2, 0]                                  # grid steps added to the smallest component of the second offset


def ring_case(gen, B=3, M=1024):
    """Workgroup 0 of every sample: queries in a ball of radius 0.05 around c0; targets 0 .. 127 all lie within 2 rho of c0
    (kept whatever d_c is, so index = compact position).  Query 1 + 7 k has its two nearest targets at the positions
    PAIRS[k], at offsets of length 0.004 that are a signed permutation of each other: query and offsets lie on a grid of
    2^-27 on which every sum is exact in fp32, so the two squared distances differ by their rounding alone, and by a
    few ulp more where one grid step is added to the smallest component.  Sample 0 as described, sample 1 with the two
    positions exchanged, sample 2 the same point twice (the lowest index wins)."""
    rho, r, grid = 0.05, 0.004, 2.0 ** -27
    c0 = torch.tensor([0.06, -0.06, 0.03])
    p1 = blobs(gen, B, radius=0.05)
    p2 = cube(gen, B, M)
    for b in range(B):
        q = c0 + ball(gen, WG, rho)
        q[1:1 + 7 * len(PAIRS):7] = torch.round(q[1:1 + 7 * len(PAIRS):7] * 2.0 ** 20) / 2.0 ** 20
        p1[b, 0:WG] = q
        d = torch.randn(128, 3, generator=gen)
        p2[b, 0:128] = c0 + d / d.norm(dim=1, keepdim=True) * (0.055 + 0.035 * torch.rand(128, 1, generator=gen))
        for k, (i, j) in enumerate(PAIRS):
            a = q[1 + 7 * k]
            u = torch.randn(3, generator=gen)
            off = torch.round(u / u.norm() * r / grid) * grid
            off2 = -off[[1, 2, 0]]
            off2[off2.abs().argmin()] += TWEAK[k] * grid
            if b % 3 == 1:
                i, j = j, i
            p2[b, i] = a + off
            p2[b, j] = a + off2 if b % 3 != 2 else p2[b, i]
    return p1, p2


@pytest.mark.parametrize('shift,scale', [((0.0, 0.0, 0.0), 1.0), ((0.0, 0.0, 0.0), 0.25), ((2.5, 0.0, 0.0), 1.0),
                                         ((0.4, 0.4, -0.4), 0.25), ((1.0, -1.0, 0.5), 3.0)])
def test_finish_cell_boundaries(vpn, shift, scale):
    """1. Near ties and exact duplicates across every kind of cell boundary of the candidate loop; a shift off the grid
    widens the near ties to the rounding of the coordinates."""
    gen = torch.Generator().manual_seed(1000 + int(scale * 8) + int(shift[0] * 2))
    p1, p2 = ring_case(gen)
    p1, p2 = ((p1 + torch.tensor(shift)) * scale).contiguous(), ((p2 + torch.tensor(shift)) * scale).contiguous()
    for b in range(p1.shape[0]):
        assert kept(p1[b, 0:WG], p2[b])[0:128].all()             # positions 0 .. 127 of workgroup 0 are targets 0 .. 127
    assert_sides(cand_counts(p1, p2), 'cand')
    check_mode6(vpn, p1.to(DEV), p2.to(DEV), 'rings, shift %s scale %g' % (shift, scale))


COUNTS = [1, 5, 16, 17, 63, 64, 65, 33, 65, 64, 63, 17, 16, 5, 1, 128]       # candidates of the 16 workgroups of a sample


def padding_case(gen, B=2):
    """Workgroup w: queries in a ball of radius 0.02 around a grid point, COUNTS[w] targets within 0.03 of it (kept:
    inside 2 rho), every other target at least 0.17 away (outside 2 rho + d_c <= 0.07); the clusters are interleaved in
    index, with 100 far targets among them."""
    g = N // WG
    grid = torch.tensor([[x, y, 0.0] for x in (-0.3, -0.1, 0.1, 0.3) for y in (-0.3, -0.1, 0.1, 0.3)])
    p1 = torch.empty(B, N, 3)
    p2 = []
    for b in range(B):
        t = []
        for w in range(g):
            p1[b, w * WG:(w + 1) * WG] = grid[w] + ball(gen, WG, 0.02)
            d = torch.randn(COUNTS[w], 3, generator=gen)
            t.append(grid[w] + d / d.norm(dim=1, keepdim=True) * 0.03 * torch.rand(COUNTS[w], 1, generator=gen))
        far = torch.randn(100, 3, generator=gen)
        t.append(far / far.norm(dim=1, keepdim=True) * 2.0)
        t = torch.cat(t)
        p2.append(t[torch.randperm(t.shape[0], generator=gen)])
    return p1, torch.stack(p2).contiguous()


def test_finish_padding(vpn):
    """2. Workgroups with 1, 5, 16, 17, 63, 64 and 65 candidates: the winner cell reaches the padding or ends at it."""
    gen = torch.Generator().manual_seed(2)
    p1, p2 = padding_case(gen)
    counts = cand_counts(p1, p2)
    assert (counts == np.array(COUNTS)[None, :]).all(), counts
    check_mode6(vpn, p1.to(DEV), p2.to(DEV), 'padding')


def test_finish_fewer_targets_than_a_pair(vpn):
    """2. M = 40: the whole cloud is less than one pair of blocks."""
    gen = torch.Generator().manual_seed(40)
    p1, p2 = blobs(gen, 3), cube(gen, 3, 40)
    assert_sides(cand_counts(p1, p2), 'cand')
    check_mode6(vpn, p1.to(DEV), p2.to(DEV), 'M = 40')


@pytest.mark.parametrize('M', [2048, 700, 2049, 2100, 4096])
def test_prologue_passes(vpn, M):
    """3. One compaction pass (M <= 2048: full and ragged) and two (padded size above 2048)."""
    gen = torch.Generator().manual_seed(300 + M)
    p1, p2 = blobs(gen, 2, radius=0.05), cube(gen, 2, M)
    assert_sides(cand_counts(p1, p2), 'cand')
    check_mode6(vpn, p1.to(DEV), p2.to(DEV), 'M = %d' % M)


def test_prologue_one_pass_nan_and_inf_targets(vpn):
    """3. A NaN target (kept by the rule: NaN compares false) and an infinite one at M = 2048.  Distances only, as
    in the other NaN tests: the filter's minimum tree does not order NaN the way brute force does."""
    gen = torch.Generator().manual_seed(33)
    p1, p2 = blobs(gen, 2), cube(gen, 2, 2048)
    p2[0, 17, 2] = math.nan
    p2[0, 2047] = math.inf
    p2[1, 1000:1003] = math.nan
    p2[1, 5, 0] = -math.inf
    assert_sides(cand_counts(p1, p2), 'cand')
    check_mode6(vpn, p1.to(DEV), p2.to(DEV), 'NaN and inf targets', names=('dist1', 'dist2'))


@pytest.mark.parametrize('K,n', [(16, 256), (22, 192)])
def test_box_source_mode7(vpn, K, n):
    """4. Mode 7, features and tile boxes written by the sampler's launch.  n = 256: one primitive per workgroup, the stored
    box is exact and gives the centre.  n = 192: tiles straddle primitives, their boxes are "all space" (and the last,
    partial tile is exact), so the workgroups compute their own.  200 targets: every workgroup is below the cap."""
    gen = torch.Generator().manual_seed(4 + n)
    B, M = 3, 200
    params = rand_params(gen, B, K).to(DEV)
    kinds = vpn.kinds_tensor([1] * 5 + [0] * (K - 5), torch.device(DEV))
    gt = cube(gen, B, M).to(DEV)
    pts = check_mode7(vpn, params, kinds, n, gt, 'mode 7, K = %d, n = %d' % (K, n))
    assert_sides(cand_counts(pts, gt), 'cand')


def test_box_source_partial_last_workgroup(vpn):
    """4. Mode 6 with N = 4100: the last workgroup has four queries, the box of its tile excludes the padding rows."""
    gen = torch.Generator().manual_seed(41)
    p1 = torch.cat([blobs(gen, 3), 0.3 + 0.01 * torch.rand(3, 4, 3, generator=gen)], 1).contiguous()
    p2 = cube(gen, 3, 700)
    counts = cand_counts(p1, p2)
    assert counts.shape[1] == 17
    assert_sides(counts, 'cand')
    check_mode6(vpn, p1.to(DEV), p2.to(DEV), 'N = 4100')


def test_box_source_nan_query(vpn):
    """4. A NaN query: its workgroup has no finite bound and scans everything, the others are unaffected."""
    gen = torch.Generator().manual_seed(42)
    p1, p2 = blobs(gen, 2), cube(gen, 2, 1500)
    p1[0, 300, 1] = math.nan
    p1[1, 4000] = math.nan
    counts = cand_counts(p1, p2)
    assert np.isinf(counts[0, 1]) and np.isinf(counts[1, 15]), counts
    assert (counts[np.isfinite(counts)] < CAP / 2).all() and np.isfinite(counts).sum() == 30, counts
    # the index of the NaN queries themselves is not specified (no target compares below their minimum): every other one is
    check_mode6(vpn, p1.to(DEV), p2.to(DEV), 'NaN query', names=('dist1', 'dist2', 'idx2'))
    ref = vpn.chamfer_nn(p1.to(DEV), p2.to(DEV), mode='brute')[1].cpu()
    got = vpn.chamfer_nn(p1.to(DEV), p2.to(DEV), mode='mfma16')[1].cpu()
    ok = ~torch.isnan(p1).any(dim=2)
    assert int((~ok).sum()) == 2 and torch.equal(got[ok], ref[ok]), 'NaN query: idx1 of the other queries differs from brute force'


def mixed_case():
    gen = torch.Generator().manual_seed(5)
    p1, p2 = blobs(gen, 3), cube(gen, 3, 2048)
    p1[0, 5 * WG:6 * WG] = cube(gen, 1, WG)[0]
    p1[1, 0:WG] = cube(gen, 1, WG)[0]
    p1[2, 15 * WG:] = cube(gen, 1, WG)[0]
    return p1, p2


CHILD = r'''
import sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import vpn_amd
from test_chamfer_cand_finish import mixed_case
p1, p2 = mixed_case()
for t in vpn_amd.chamfer_nn(p1.cuda(), p2.cuda(), mode='mfma16'):
    sys.stdout.write('OUT ' + t.cpu().numpy().tobytes().hex() + '\n')
'''


def test_cand_and_fallback_equal_the_switch(vpn):
    """5. Candidate and full-scan workgroups in one launch: brute force bit for bit, and the same bytes from a child process
    with VPN_CHAMFER_CAND=0 (read once per process), i.e. from the full scan of every workgroup."""
    p1, p2 = mixed_case()
    assert_sides(cand_counts(p1, p2), 'mixed')
    check_mode6(vpn, p1.to(DEV), p2.to(DEV), 'blobs and spread workgroups')
    got = vpn.chamfer_nn(p1.to(DEV), p2.to(DEV), mode='mfma16')
    env = dict(os.environ, VPN_CHAMFER_CAND='0')
    r = subprocess.run([sys.executable, '-c', CHILD % (ROOT, os.path.join(ROOT, 'tests'))], env=env, capture_output=True,
                       text=True, timeout=300)
    lines = [x[4:] for x in r.stdout.splitlines() if x.startswith('OUT ')]
    assert r.returncode == 0 and len(lines) == 4, r.stdout[-2000:] + r.stderr[-2000:]
    for name, t, h in zip(('dist1', 'idx1', 'dist2', 'idx2'), got, lines):
        assert t.cpu().numpy().tobytes().hex() == h, '%s differs from the scan with the candidate form switched off' % name
