"""Wave walk of the fp16 Chamfer scan (modes 6 and 7): from 4096 targets on, every direction-2 wave visits
the target tiles on its own, straight from the row buffer, with no LDS tile and no barrier, and requests the next tile
on a stale bound.  It takes the decisions of the shared tile loop, so nothing may change a bit: every case compares
modes 6 and 7 with brute force in dist1, idx1, dist2 and idx2 (mode 7 scans the features that the mode-6 call left in
the same workspace, or the sampler's), and one case compares with a child process that runs the shared tile loop
(VPN_CHAMFER_WAVEWALK=0), the Chamfer loss term formed from the per-workgroup sums included.

The targets are p1 (N >= 4096 points, 16 tiles of 256 at the least), the walking queries p2 (M points, 32 per wave,
256 per workgroup)."""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT
from test_chamfer_skip import check_mode7, rand_params, same, vpn  # noqa: F401  (vpn: the module fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N = 4096                     # the smallest target cloud that takes the form (CSKIP_MIN_TARGETS)
NAMES = ('dist1', 'idx1', 'dist2', 'idx2')


def scan_ws(p1, p2, mode, ws=None):
    """vpn_chamfer_fwd_ws in `mode` on an explicit workspace (new: filled with NaN); returns (d1, i1, d2, i2), ws."""
    from vpn_amd import _lib
    L = _lib.lib()
    B, n, m = p1.shape[0], p1.shape[1], p2.shape[1]
    nbytes = L.vpn_chamfer_workspace(B, n, m)
    if ws is None:
        ws = torch.full((nbytes // 4,), float('nan'), dtype=torch.float32, device=p1.device)
    d1 = torch.full((B, n), -1.0, device=p1.device); d2 = torch.full((B, m), -1.0, device=p1.device)
    i1 = torch.full((B, n), -1, dtype=torch.int32, device=p1.device); i2 = torch.full((B, m), -1, dtype=torch.int32, device=p1.device)
    _lib.call('vpn_chamfer_fwd_ws', _lib.ptr(p1), _lib.ptr(p2), B, n, m, _lib.ptr(d1), _lib.ptr(i1), _lib.ptr(d2),
              _lib.ptr(i2), _lib.ptr(ws), nbytes, mode, _lib.stream())
    return (d1, i1, d2, i2), ws


def check(vpn, p1, p2, what):
    p1, p2 = p1.contiguous().to(DEV), p2.contiguous().to(DEV)
    ref = vpn.chamfer_nn(p1, p2, mode='brute')
    six, ws = scan_ws(p1, p2, 6)
    seven, _ = scan_ws(p1, p2, 7, ws)
    for mode, got in ((6, six), (7, seven)):
        for name, x, y in zip(NAMES, got, ref):
            if name.startswith('idx'):
                # the index of a query whose distance is NaN, or that has a NaN coordinate itself, is not specified: such
                # a query has no nearest neighbour (brute force reports distance inf and index 0 for it, the filtered scan,
                # with the shared tile loop as with the wave walk, distance inf and index 0x7fffffff)
                q = p1 if name == 'idx1' else p2
                ok = ~torch.isnan(ref[0] if name == 'idx1' else ref[2]) & ~torch.isnan(q).any(2)
                x, y = x[ok], y[ok]
            assert same(x, y), '%s: mode %d %s differs from brute force' % (what, mode, name)


def cube(gen, B, n):
    return torch.rand(B, n, 3, generator=gen) - 0.5


@pytest.mark.parametrize('M', [33, 256, 257, 1500])
def test_walk_query_counts(vpn, M):
    """One wave and a lane, one workgroup, a ragged second workgroup, several workgroups."""
    gen = torch.Generator().manual_seed(800 + M)
    check(vpn, cube(gen, 2, N), cube(gen, 2, M), 'M = %d' % M)


@pytest.mark.parametrize('n', [4160, 4200])
def test_walk_short_last_tile(vpn, n):
    """A last tile of 2 blocks (4160 rows) and of 4 (4200 points in 4224 rows); some queries sit beside its points."""
    gen = torch.Generator().manual_seed(n)
    p1, p2 = cube(gen, 3, n), cube(gen, 3, 600)
    p2[:, :100] = p1[:, n - 100:] + 1.0e-3 * torch.randn(3, 100, 3, generator=gen)
    check(vpn, p1, p2, 'N = %d' % n)


def clustered_targets(gen, B, spread=0.01):
    """Sixteen tight clusters, one per tile, on a 4 x 2 x 2 grid of centres."""
    centres = torch.tensor([[x, y, z] for x in (-0.45, -0.15, 0.15, 0.45) for y in (-0.3, 0.3) for z in (-0.3, 0.3)])
    p1 = centres[:, None, :] + spread * torch.randn(16, 256, 3, generator=gen)
    return centres, p1.reshape(1, N, 3).expand(B, -1, -1).contiguous()


def test_walk_waves_need_disjoint_tiles(vpn):
    """Eight clusters of 32 queries, each beside a different target tile: the eight waves of the one workgroup want
    eight different tiles and skip the rest (with the shared tile every wave waited for every tile)."""
    gen = torch.Generator().manual_seed(31)
    centres, p1 = clustered_targets(gen, 2)
    p2 = (centres[1::2][:, None, :] + 0.02 * torch.randn(8, 32, 3, generator=gen)).reshape(1, 256, 3)
    p2 = torch.cat([p2, p2.flip(1)], 0)              # second sample: the clusters in the opposite order
    check(vpn, p1, p2, 'disjoint tiles')


def test_walk_all_or_nothing(vpn):
    """Every query beside one cluster: every wave can skip all tiles but one.  And targets whose every tile reaches both
    corners of the cube: no tile can be skipped, every request on the stale bound is used."""
    gen = torch.Generator().manual_seed(32)
    centres, p1 = clustered_targets(gen, 2)
    check(vpn, p1, centres[5] + 0.03 * torch.randn(2, 700, 3, generator=gen), 'one tile')
    u = cube(gen, 2, N)
    u[:, ::256] = torch.tensor([-0.5, -0.5, -0.5])
    u[:, 1::256] = torch.tensor([0.5, 0.5, 0.5])
    check(vpn, u, cube(gen, 2, 700), 'no skipping')


def test_walk_duplicates(vpn):
    """Duplicated targets in two tiles (the lowest index wins whichever tile a wave drops), and duplicated queries that
    the visiting order puts into different waves."""
    gen = torch.Generator().manual_seed(33)
    p1, p2 = cube(gen, 3, N), cube(gen, 3, 1500)
    p1[:, 3584:3840] = p1[:, 0:256]                   # tile 14 repeats tile 0
    p1[:, 2800:2900] = p1[:, 300:400]
    p2[:, 1000:1500] = p2[:, 0:500].flip(1)
    p2[:, 100:200] = p1[:, 3600:3700]                 # queries that sit on a duplicated target
    check(vpn, p1, p2, 'duplicates')


def test_walk_outside_fp16_domain(vpn):
    """Coordinates x 1000: outside the filter's domain the bound is infinite, every wave scans every tile."""
    gen = torch.Generator().manual_seed(34)
    check(vpn, cube(gen, 2, N) * 1000.0, cube(gen, 2, 600) * 1000.0, 'x1000')


def test_walk_nan_and_inf_queries(vpn):
    """A NaN and an infinite query beside ordinary ones in their waves: they never skip, their neighbours still do."""
    gen = torch.Generator().manual_seed(35)
    p1, p2 = cube(gen, 2, N), cube(gen, 2, 600)
    p2[0, 17, 2] = math.nan
    p2[1, 300] = math.nan
    p2[0, 401, 0] = math.inf
    p2[1, 5, 1] = -math.inf
    check(vpn, p1, p2, 'NaN and inf queries')


def test_walk_mode7_sampled(vpn):
    """Mode 7 through vpn_hotpath_sample_fwd (features, visiting order and tile boxes written by the sampler's launch
    into a workspace full of NaN): B = 2, K = 16 primitives of n = 256 points, 300 ground-truth points."""
    gen = torch.Generator().manual_seed(36)
    params = rand_params(gen, 2, 16).to(DEV)
    kinds = vpn.kinds_tensor([1] * 5 + [0] * 11, torch.device(DEV))
    check_mode7(vpn, params, kinds, 256, cube(gen, 2, 300).to(DEV), 'mode 7, K = 16, n = 256, M = 300')


def switch_case(vpn_amd):
    """What the switch must not change: the scan of a cloud with ties (mode 6), and the step's Chamfer loss term, which
    the raster launch forms from the per-workgroup sums the scan leaves behind (mode 7, K = 16, n = 256, M = 300)."""
    gen = torch.Generator().manual_seed(37)
    p1, p2 = cube(gen, 3, 4200), cube(gen, 3, 1500)
    p1[:, 3584:3840] = p1[:, 0:256]
    p2[:, 1000:1500] = p2[:, 0:500].flip(1)
    out = list(scan_ws(p1.to(DEV), p2.to(DEV), 6)[0])
    B, K, n, M, H, W = 2, 16, 256, 300, 16, 16
    assert vpn_amd._lib.lib().vpn_hotpath_fused_features(B, K, n, M) == 1
    params = rand_params(gen, B, K).to(DEV)
    cam = torch.tensor([[1.0, 0.0, 0.0]], device=DEV).expand(B, 3).contiguous()
    sil = (torch.rand(B, 1, H, W, generator=gen) > 0.5).float().to(DEV)
    dep = (2.0 - torch.rand(B, H, W, generator=gen)).to(DEV)
    with torch.no_grad():
        losses = vpn_amd.HotPathLossFunction.apply(params, vpn_amd.kinds_tensor([1] * 5 + [0] * 11, torch.device(DEV)), cam,
                                                   cube(gen, B, M).to(DEV), sil, dep, n, 7, 0, H, W, vpn_amd.config.RASTER_SIGMA,
                                                   vpn_amd.config.RASTER_GAMMA, vpn_amd.config.RASTER_Z_FAR, 1.0, 0.0, 0.0)
    out.append(losses[2].reshape(1))                 # the total with w_sil = w_depth = 0: the Chamfer term alone
    return [t.cpu() for t in out]


CHILD = r'''
import sys, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import vpn_amd
from test_chamfer_wavewalk import switch_case
torch.save(switch_case(vpn_amd), sys.argv[1])
print('SWITCH-OFF-OK')
'''


def test_walk_switched_off(vpn, tmp_path):
    """VPN_CHAMFER_WAVEWALK=0 (read once per process: a child) runs the shared tile loop: the same bits."""
    mine = switch_case(vpn)
    assert math.isfinite(float(mine[4])) and float(mine[4]) > 0.0
    path = str(tmp_path / 'shared_loop.pt')
    env = dict(os.environ, VPN_CHAMFER_WAVEWALK='0')
    r = subprocess.run([sys.executable, '-c', CHILD % (ROOT, os.path.join(ROOT, 'tests')), path], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'SWITCH-OFF-OK' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    theirs = torch.load(path)
    for name, x, y in zip(NAMES + ('chamfer loss term',), mine, theirs):
        assert torch.equal(x, y), '%s differs between the wave walk and the shared tile loop' % name
