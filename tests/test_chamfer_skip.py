"""Tile skipping of the fp16 Chamfer scan (modes 6 and 7): direction 2 visits the ground-truth cloud in
Morton-cell order and a wave skips every target tile whose box lies beyond all of its queries' current best.  Neither
may change a bit: every case below compares modes 6 and 7 with brute force in dist1, idx1, dist2 and idx2."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def vpn():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU (no CPU fallback exists)')
    import vpn_amd
    vpn_amd._lib.lib()
    return vpn_amd


def rand_params(gen, B, K):
    v = (torch.rand(B, K, 3, generator=gen) + 0.1) / torch.tensor([8.0, 10.0, 10.0])
    q = torch.rand(B, K, 4, generator=gen)
    t = 0.35 * (torch.rand(B, K, 3, generator=gen) * 2 - 1)
    return torch.cat([v, q, t], 2)


def same(x, y):
    """Bit-equal; NaN where the other has NaN."""
    if x.dtype == torch.float32:
        nx, ny = torch.isnan(x), torch.isnan(y)
        return torch.equal(nx, ny) and torch.equal(x[~nx].view(torch.int32), y[~ny].view(torch.int32))
    return torch.equal(x, y)


def check_mode6(vpn, p1, p2, what, names=('dist1', 'idx1', 'dist2', 'idx2')):
    ref = vpn.chamfer_nn(p1, p2, mode='brute')
    got = vpn.chamfer_nn(p1, p2, mode='mfma16')
    for name, x, y in zip(('dist1', 'idx1', 'dist2', 'idx2'), got, ref):
        if name not in names:
            continue
        if name.startswith('idx'):                    # the index of a query whose distance is NaN is not specified
            ok = ~torch.isnan(ref[0] if name == 'idx1' else ref[2])
            x, y = x[ok], y[ok]
        assert same(x, y), '%s: %s differs from brute force' % (what, name)


def sampled_mode7(vpn, params, kinds, n, gt, seed=99):
    """vpn_hotpath_sample_fwd writing the features (with the ground-truth order and the tile boxes) + the scan in mode
    7; returns the sampled points and (d1, i1, d2, i2).  The workspace starts as NaN: nothing may rely on old contents."""
    from vpn_amd import _lib
    L = _lib.lib()
    dev = torch.device(DEV)
    B, K = params.shape[0], params.shape[1]
    M, N, H, W = gt.shape[1], K * n, 16, 16
    cam = torch.tensor([[1.0, 0.0, 0.0]], device=dev).expand(B, 3).contiguous()
    rec = torch.empty((L.vpn_raster_records_size(B, K, H, W) // 4,), dtype=torch.float32, device=dev)
    lws = torch.zeros((L.vpn_raster_loss_workspace(B, H, W) // 4,), dtype=torch.float32, device=dev)
    nbytes = L.vpn_chamfer_workspace(B, N, M)
    ws = torch.full((nbytes // 4,), float('nan'), dtype=torch.float32, device=dev)
    pts = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    _lib.call('vpn_hotpath_sample_fwd', _lib.ptr(params), _lib.ptr(kinds), None, seed, None, 0, B, K, n, _lib.ptr(pts),
              _lib.ptr(cam), H, W, 0.05, _lib.ptr(rec), _lib.ptr(lws), _lib.ptr(gt), M, _lib.ptr(ws), nbytes, _lib.stream())
    d1 = torch.empty((B, N), device=dev); d2 = torch.empty((B, M), device=dev)
    i1 = torch.empty((B, N), dtype=torch.int32, device=dev); i2 = torch.empty((B, M), dtype=torch.int32, device=dev)
    _lib.call('vpn_chamfer_fwd_ws', _lib.ptr(pts), _lib.ptr(gt), B, N, M, _lib.ptr(d1), _lib.ptr(i1), _lib.ptr(d2),
              _lib.ptr(i2), _lib.ptr(ws), nbytes, 7, _lib.stream())
    return pts, (d1, i1, d2, i2)


def check_mode7(vpn, params, kinds, n, gt, what):
    pts, got = sampled_mode7(vpn, params, kinds, n, gt)
    ref = vpn.chamfer_nn(pts, gt, mode='brute')
    six = vpn.chamfer_nn(pts, gt, mode='mfma16')
    for name, x, y, z in zip(('dist1', 'idx1', 'dist2', 'idx2'), got, ref, six):
        assert same(x, y), '%s: mode 7 %s differs from brute force' % (what, name)
        assert same(z, y), '%s: mode 6 %s differs from brute force' % (what, name)
    return pts


def test_skip_bench_inputs(vpn):
    """The C3 bench inputs (B = 64, K = 32 spheres, n = 256, M = 2048), and a partly converged batch whose ground truth
    lies on the primitives' surfaces (a second draw of the same primitives)."""
    import bench
    params, gt = bench.synth_inputs(64, 32, 2048, 1234, torch.device(DEV))
    kinds = vpn.kinds_tensor([0] * 32, torch.device(DEV))
    check_mode7(vpn, params.contiguous(), kinds, 256, gt.contiguous(), 'C3')
    on_surface, _ = sampled_mode7(vpn, params.contiguous(), kinds, 64, gt.contiguous(), seed=7)
    check_mode7(vpn, params.contiguous(), kinds, 256, on_surface.contiguous(), 'C3, ground truth on the surfaces')


def test_skip_ties_and_duplicates(vpn):
    """Exact-distance ties: duplicated target points in different tiles (the lowest index must win whatever tile a wave
    skips or scans first), duplicated queries in different Morton cells of the visiting order, and a lattice whose
    distances tie in bulk."""
    gen = torch.Generator().manual_seed(5)
    B, N, M = 3, 4096, 1500
    p1 = torch.rand(B, N, 3, generator=gen) - 0.5
    p1[:, 3584:3840] = p1[:, 0:256]                   # tile 14 repeats tile 0
    p1[:, 2800:2900] = p1[:, 300:400]
    p2 = torch.rand(B, M, 3, generator=gen) - 0.5
    p2[:, 1000:1500] = p2[:, 0:500].flip(1)          # the same query twice, far apart in the original order
    check_mode6(vpn, p1.to(DEV), p2.to(DEV), 'duplicates')
    ax = torch.arange(16, dtype=torch.float32) / 16 - 0.5
    lat = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(1, -1, 3)     # 4096 lattice points
    q = (torch.rand(2, 1024, 3, generator=gen) * 16).floor() / 16 - 0.5 + 1.0 / 32        # lattice cell centres: 8-way ties
    check_mode6(vpn, lat.expand(2, -1, -1).contiguous().to(DEV), q.to(DEV), 'lattice')


def test_skip_all_or_nothing(vpn):
    """A target cloud of eight tight clusters, one per tile, against queries near one cluster: every wave can skip all
    tiles but one (sixteen tiles, two per cluster).  And a target cloud where every tile spans the whole cube: nothing can be skipped."""
    gen = torch.Generator().manual_seed(6)
    B = 2
    centres = torch.tensor([[x, y, z] for x in (-0.4, 0.4) for y in (-0.4, 0.4) for z in (-0.4, 0.4)])
    p1 = (centres.repeat(2, 1)[:, None, :] + 0.01 * torch.randn(16, 256, 3, generator=gen)).reshape(1, 4096, 3).expand(B, -1, -1)
    p2 = centres[5] + 0.05 * torch.randn(B, 1200, 3, generator=gen)
    check_mode6(vpn, p1.contiguous().to(DEV), p2.to(DEV), 'clusters')
    u = torch.rand(B, 4096, 3, generator=gen) - 0.5
    u[:, ::256] = torch.tensor([-0.5, -0.5, -0.5])   # every tile reaches both corners
    u[:, 1::256] = torch.tensor([0.5, 0.5, 0.5])
    check_mode6(vpn, u.to(DEV), (torch.rand(B, 1200, 3, generator=gen) - 0.5).to(DEV), 'no skipping')


# the skipping scan runs from CSKIP_MIN_TARGETS = 4096 sampled points on; (1000, 777) is the plain path
@pytest.mark.parametrize('N,M', [(4100, 777), (4097, 2050), (8192, 2047), (5000, 4097), (4352, 1000), (1000, 777)])
def test_skip_ragged_and_large(vpn, N, M):
    """Sizes that are not multiples of 32, 64 or 256, and ground-truth clouds above the one-workgroup ordering limit
    (2048 points: natural order, the tile boxes still apply)."""
    gen = torch.Generator().manual_seed(N * 7 + M)
    p1 = torch.rand(3, N, 3, generator=gen) - 0.5
    p2 = torch.rand(3, M, 3, generator=gen) - 0.5
    check_mode6(vpn, p1.to(DEV), p2.to(DEV), '%d x %d' % (N, M))


def test_skip_mode7_ragged(vpn):
    """Mode 7 with primitives whose rows do not fill whole tiles (tiles shared by two primitives get the box of all
    space), a ragged ground-truth cloud, odd batch sizes, and the C5 shape (2048 points: no skipping)."""
    gen = torch.Generator().manual_seed(11)
    for (B, K, n, M) in ((3, 41, 100, 777), (8, 16, 512, 2050), (5, 17, 256, 4500), (4, 64, 32, 2048)):
        params = rand_params(gen, B, K).to(DEV)
        kinds = torch.tensor(sorted((int(x) for x in torch.randint(0, 2, (K,), generator=gen)), reverse=True),
                             dtype=torch.int32)
        kinds = vpn.kinds_tensor(kinds.tolist(), torch.device(DEV))
        gt = (torch.rand(B, M, 3, generator=gen) - 0.5).to(DEV)
        check_mode7(vpn, params, kinds, n, gt, 'B=%d K=%d n=%d M=%d' % (B, K, n, M))


@pytest.mark.parametrize('scale', [9.0, 1000.0])
def test_skip_outside_fp16_domain(vpn, scale):
    """Clouds outside the fp16 filter's domain (|p|^2 > 64) never skip: their queries are resolved exactly."""
    gen = torch.Generator().manual_seed(int(scale))
    p1 = (torch.rand(2, 4096, 3, generator=gen) - 0.5) * scale
    p2 = (torch.rand(2, 1100, 3, generator=gen) - 0.5) * scale
    check_mode6(vpn, p1.to(DEV), p2.to(DEV), 'x%g' % scale)


def test_skip_outlier_and_nan(vpn):
    """One outlier in either cloud, and NaN coordinates in both (same NaN pattern as brute force)."""
    gen = torch.Generator().manual_seed(12)
    p1 = torch.rand(2, 4096, 3, generator=gen) - 0.5
    p2 = torch.rand(2, 1100, 3, generator=gen) - 0.5
    a, b = p1.clone(), p2.clone()
    a[0, 700] = torch.tensor([30.0, -2.0, 1.0])
    b[1, 40] = torch.tensor([-100.0, 0.0, 0.0])
    check_mode6(vpn, a.to(DEV), b.to(DEV), 'outliers')
    a, b = p1.clone(), p2.clone()
    a[0, 5, 1] = math.nan
    a[1, 3800] = math.nan
    b[0, 17, 2] = math.nan
    b[1, 1000:1003] = math.nan
    # indices are not compared: with NaN targets in a cloud the filtered scan's index already differs from brute force
    # without any skipping (the filter's minimum tree does not order NaN the way the brute-force compare does; same
    # count of differing indices before and after this change on these inputs)
    check_mode6(vpn, a.to(DEV), b.to(DEV), 'NaN', names=('dist1', 'dist2'))
