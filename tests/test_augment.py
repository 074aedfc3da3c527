"""GPU tests of the batch augmentation stage (modules/augmentation.py on csrc/augment.hip): CutMix pinned to the
reference's own output (tests/golden/g8_cutmix.npz, captured by tools/make_golden_augment.py), the uniformity and the
keying of its draws, the empty eligible list, and the point mix-up against oracle.emd_auction."""
import math

import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _fixture():
    z = load_golden('g8_cutmix')
    seeds = []
    for k in range(int(z['n_seeds'])):
        seeds.append({n: z['s%d_%s' % (k, n)] for n in ('seed', 'ratio', 'indices', 'img_cut_index', 'point_cut_ratio',
                                                        'rgbs', 'silhouettes', 'points', 'count', 'eligible')})
    return z['points'], z['rgbs'], z['silhouettes'], seeds


def _eligible(points, idx, cut):
    """The eligible candidate numbers of every sample, by torch on the CPU (cutmix.py:32)."""
    B, N, _ = points.shape
    cut = torch.as_tensor(cut, dtype=torch.float32).expand(B) if not isinstance(cut, float) else torch.full((B,), cut)
    out = []
    for b in range(B):
        p = int(idx[b])
        mask = torch.cat([points[b][:, 2] >= cut[b], points[p][:, 2] < cut[b]])
        out.append(torch.nonzero(mask).flatten())
    return out


def _check_against_lists(points, idx, elig, out, src, count, n_out=None):
    """count, src and out of one vpn_cutmix_points call against the eligible lists; returns the case kinds seen."""
    B, N, _ = points.shape
    n_out = N if n_out is None else n_out
    out, src, count = out.cpu(), src.cpu().long(), count.cpu()
    kinds = {}
    for b in range(B):
        p, e = int(idx[b]), elig[b]
        c = e.numel()
        assert int(count[b]) == c, (b, int(count[b]), c)
        cand = torch.cat([points[b], points[p]])
        assert int(src[b].min()) >= 0 and int(src[b].max()) < 2 * N
        assert torch.equal(out[b].view(torch.int32), cand[src[b]].view(torch.int32)), b      # bit for bit
        if c == 0:
            assert torch.equal(src[b], torch.arange(n_out) % N)
            kind = 'empty'
        else:
            assert bool(torch.isin(src[b], e).all()), b
            if c == n_out:
                assert torch.equal(src[b], e), b
                kind = 'fixed_point' if p == b else 'equal_other'
            elif c > n_out:
                assert src[b].unique().numel() == n_out, b
                kind = 'more'
            else:
                kind = 'fewer'
        kinds[kind] = kinds.get(kind, 0) + 1
    return kinds


def _mix_images(x, idx, ci):
    return torch.cat([x[..., :ci], x[idx.long()][..., ci:]], 3)


def test_images_equal_the_reference():
    import vpn_amd
    from vpn_amd import ops
    pts, rgbs, sils, seeds = _fixture()
    for s in seeds:
        torch.manual_seed(int(s['seed']))
        r, m, p = vpn_amd.cut_mix_data(rgbs.to(DEV), sils.to(DEV), pts.to(DEV))
        assert torch.equal(r.cpu(), s['rgbs']) and torch.equal(m.cpu(), s['silhouettes'])
        assert p.shape == pts.shape and not p.requires_grad and not r.requires_grad
    B, _, H, W = rgbs.shape
    idx = seeds[0]['indices']
    for ratio, ci in ((0.0, 0), (1.0, W), (0.5, W // 2)):
        r, m, _ = vpn_amd.cut_mix_data(rgbs.to(DEV), sils.to(DEV), pts.to(DEV), cut_ratio=ratio, indices=idx, seed=1)
        assert torch.equal(r.cpu(), _mix_images(rgbs, idx, ci)) and torch.equal(m.cpu(), _mix_images(sils, idx, ci))
    # rows of a multiple of four floats: 16-byte accesses when the tensors are aligned, element-wise when they start
    # 4 bytes past a 16-byte boundary; every cut, the ones inside a group of four included
    g = torch.Generator().manual_seed(5)
    a, s1 = torch.rand(B, 3, 6, 16, generator=g), torch.rand(B, 1, 6, 16, generator=g)
    idx_d = ops.partner_indices(idx, B, DEV)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    for ci in range(0, 17):
        for ia, ib in ((a.to(DEV), s1.to(DEV)), (shifted(a), shifted(s1)), (a.to(DEV), shifted(s1))):
            oa, ob = ops.cutmix_images(ia, ib, idx_d, ci)
            assert torch.equal(oa.cpu(), _mix_images(a, idx, ci)) and torch.equal(ob.cpu(), _mix_images(s1, idx, ci)), ci
    oa, ob = ops.cutmix_images(a.to(DEV), None, idx_d, 5)
    assert ob is None and torch.equal(oa.cpu(), _mix_images(a, idx, 5))


def test_points_follow_the_reference_lists():
    import vpn_amd
    pts, _, _, seeds = _fixture()
    B, N, _ = pts.shape
    seen = {}
    for s in seeds:
        elig = [s['eligible'][b, :int(s['count'][b])].long() for b in range(B)]
        out, src, count = vpn_amd.cut_mix_batch_points(pts.to(DEV), s['indices'], float(s['point_cut_ratio']), seed=11,
                                                       return_src=True)
        assert src.dtype == torch.int32 and count.dtype == torch.int32 and not out.requires_grad
        assert torch.equal(count.cpu(), s['count'])
        kinds = _check_against_lists(pts, s['indices'], elig, out, src, count)
        for b in range(B):
            if int(s['count'][b]) == N:                  # the list itself: the reference's output bit for bit
                assert torch.equal(out[b].cpu(), s['points'][b])
        for k, v in kinds.items():
            seen[k] = seen.get(k, 0) + v
    for kind in ('more', 'fewer', 'equal_other', 'fixed_point'):
        assert seen.get(kind, 0) >= 1, seen


@pytest.mark.parametrize('N', [1000, 2048, 4096, 8192])
def test_points_at_other_sizes(N):
    """Multiples and non-multiples of the workgroup size up to the LDS bound; a [B] tensor of cuts."""
    import vpn_amd
    g = torch.Generator().manual_seed(N)
    B = 5
    pts = torch.rand(B, N, 3, generator=g) - 0.5
    pts[1, :, 2] = pts[1, :, 2] * 0.2 + 0.3
    pts[3, :, 2] = pts[3, :, 2] * 0.2 + 0.3
    idx = torch.tensor([2, 3, 2, 0, 1])
    for cut in (0.05, torch.tensor([0.05, -0.1, 0.0, 0.1, -0.05])):
        out, src, count = vpn_amd.cut_mix_batch_points(pts.to(DEV), idx, cut, seed=N, return_src=True)
        kinds = _check_against_lists(pts, idx, _eligible(pts, idx, cut), out, src, count)
        assert all(kinds.get(k, 0) >= 1 for k in ('more', 'fewer', 'equal_other', 'fixed_point')), kinds


def test_adjust_point_num():
    import vpn_amd
    g = torch.Generator().manual_seed(9)
    pts = torch.rand(700, 3, generator=g) - 0.5
    for n_out in (700, 300, 1500):
        out, src = vpn_amd.adjust_point_num(pts.to(DEV), n_out, seed=3, return_src=True)
        src = src.cpu().long()
        assert out.shape == (n_out, 3) and torch.equal(out.cpu(), pts[src])
        if n_out == 700:
            assert torch.equal(src, torch.arange(700))
        elif n_out < 700:
            assert src.unique().numel() == n_out
        else:
            assert int(src.min()) >= 0 and int(src.max()) < 700 and src.unique().numel() > 500
    with pytest.raises(RuntimeError, match='from >= to'):
        vpn_amd.adjust_point_num(pts[:0].to(DEV), 10)


def test_draws_are_uniform():
    """R = 200 seeds.  count > N: candidate j is in a run's subset with probability p = N / count, so its share of the runs
    has standard deviation sqrt(p (1 - p) / R); count < N: each of the R N slots holds candidate j with probability
    q = 1 / count, standard deviation sqrt(q (1 - q) / (R N)).  Six standard deviations: about 2e-9 per candidate, under
    1e-5 for all of them together; the seeds are fixed, so the test is deterministic."""
    import vpn_amd
    pts, _, _, seeds = _fixture()
    B, N, _ = pts.shape
    s = seeds[0]
    count = s['count']
    more, fewer = int(count.argmax()), int(count.argmin())       # the longest and the shortest list: p, q far from 0 and 1
    assert int(count[more]) > N > int(count[fewer])
    R = 200
    hits_more, hits_fewer = torch.zeros(2 * N), torch.zeros(2 * N)
    dp = pts.to(DEV)
    for r in range(R):
        _, src, _ = vpn_amd.cut_mix_batch_points(dp, s['indices'], float(s['point_cut_ratio']), seed=1000 + r, return_src=True)
        src = src.cpu().long()
        hits_more += torch.bincount(src[more], minlength=2 * N)           # distinct entries: 0 or 1 per run
        hits_fewer += torch.bincount(src[fewer], minlength=2 * N)
    for b, hits, trials in ((more, hits_more, R), (fewer, hits_fewer, R * N)):
        c = int(count[b])
        e = s['eligible'][b, :c].long()
        prob = N / c if c > N else 1.0 / c
        sd = math.sqrt(prob * (1 - prob) / trials)
        share = hits / trials
        mask = torch.zeros(2 * N, dtype=torch.bool)
        mask[e] = True
        assert float(hits[~mask].sum()) == 0
        dev = (share[e] - prob).abs().max()
        print('sample %d count %d: largest deviation %.3g standard deviations' % (b, c, float(dev) / sd))
        assert float(dev) <= 6 * sd, (b, float(dev), sd)


def test_draws_are_keyed_on_seed_and_global_sample():
    import vpn_amd
    pts, _, _, seeds = _fixture()
    dp = pts.to(DEV)
    cut = 0.02
    idx = torch.tensor([1, 0, 3, 4, 2, 6, 7, 5])                 # samples 2..4 among themselves
    a = vpn_amd.cut_mix_batch_points(dp, idx, cut, seed=77, sample_base=10, return_src=True)
    b = vpn_amd.cut_mix_batch_points(dp, idx, cut, seed=77, sample_base=10, return_src=True)
    c = vpn_amd.cut_mix_batch_points(dp, idx, cut, seed=78, sample_base=10, return_src=True)
    d = vpn_amd.cut_mix_batch_points(dp, idx, cut, seed=77, sample_base=11, return_src=True)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    assert not torch.equal(a[1], c[1]) and not torch.equal(a[1], d[1])
    assert torch.equal(a[2], c[2])
    whole = vpn_amd.cut_mix_batch_points(dp, idx, cut, seed=77, return_src=True)
    part = vpn_amd.cut_mix_batch_points(dp[2:5].contiguous(), idx[2:5] - 2, cut, seed=77, sample_base=2, return_src=True)
    assert torch.equal(part[2], whole[2][2:5])
    assert torch.equal(part[1], whole[1][2:5]) and torch.equal(part[0], whole[0][2:5])      # candidate numbers are per sample
    kinds = _check_against_lists(pts, idx, _eligible(pts, idx, cut), *whole)
    assert kinds.get('more', 0) >= 1 and kinds.get('fewer', 0) >= 1


def test_empty_eligible_list_keeps_the_sample():
    import vpn_amd
    g = torch.Generator().manual_seed(21)
    B, N = 4, 2048
    pts = torch.rand(B, N, 3, generator=g) - 0.5
    pts[0, :, 2] = -0.1 - 0.4 * torch.rand(N, generator=g)       # entirely below the cut ...
    pts[1, :, 2] = 0.1 + 0.4 * torch.rand(N, generator=g)        # ... its partner entirely above
    idx = torch.tensor([1, 0, 3, 2])
    out, src, count = vpn_amd.cut_mix_batch_points(pts.to(DEV), idx, 0.0, seed=4, return_src=True)
    assert count.cpu().tolist()[:2] == [0, 2 * N]
    assert torch.equal(out[0].cpu(), pts[0]) and torch.equal(src[0].cpu().long(), torch.arange(N))
    kinds = _check_against_lists(pts, idx, _eligible(pts, idx, 0.0), out, src, count)
    assert kinds.get('empty') == 1 and kinds.get('more', 0) >= 1
    # the other samples are what they are without the empty one in the batch
    rest = vpn_amd.cut_mix_batch_points(pts[2:].to(DEV), idx[2:] - 2, 0.0, seed=4, sample_base=2, return_src=True)
    assert torch.equal(rest[0], out[2:]) and torch.equal(rest[1], src[2:]) and torch.equal(rest[2], count[2:])
    plain = vpn_amd.cut_mix_batch_points(pts.to(DEV), idx, 0.0, seed=4)
    assert torch.equal(plain, out)


def _lerp_cpu(p1, p2, assign, r):
    return (1 - r) * p1 + r * p2[assign.long()]                  # point_mixup.py:35-36, fp32 on the CPU


@pytest.mark.parametrize('n', [128, 256, 1030])
def test_mixup_equals_the_oracle_auction(n):
    import vpn_amd
    from oracle import vpn_oracle as O
    g = torch.Generator().manual_seed(n)
    B = 4
    pts = torch.rand(B, n, 3, generator=g) - 0.5
    idx = torch.tensor([2, 0, 3, 1])
    r = 0.37291
    ref_dist, ref_assign = O.emd_auction(pts, pts[idx], 0.005, 100)
    mixed, dist, assign = vpn_amd.mixup_points(pts.to(DEV), ratio=r, indices=idx, return_assignment=True)
    assert assign.dtype == torch.int32 and not mixed.requires_grad
    assert torch.equal(assign.cpu().long(), ref_assign.long()) and torch.equal(dist.cpu(), ref_dist)
    want = torch.stack([_lerp_cpu(pts[b], pts[idx[b]], ref_assign[b], r) for b in range(B)])
    assert torch.equal(mixed.cpu().view(torch.int32), want.view(torch.int32))
    assert torch.equal(vpn_amd.mixup_points(pts.to(DEV), ratio=r, indices=idx), mixed)
    m0 = vpn_amd.mixup_points(pts.to(DEV), ratio=0.0, indices=idx)
    m1 = vpn_amd.mixup_points(pts.to(DEV), ratio=1.0, indices=idx)
    assert torch.equal(m0.cpu(), pts)
    assert torch.equal(m1.cpu(), torch.stack([pts[idx[b]][ref_assign[b].long()] for b in range(B)]))


@pytest.mark.parametrize('B', [8, 64])
def test_mixup_at_the_training_shape(B):
    import vpn_amd
    n = 2048
    g = torch.Generator().manual_seed(B)
    pts = torch.rand(B, n, 3, generator=g) - 0.5
    idx = torch.randperm(B, generator=g)
    r = 0.6180339
    dp = pts.to(DEV)
    mixed, dist, assign = vpn_amd.mixup_points(dp, ratio=r, indices=idx, return_assignment=True)
    a = assign.cpu()
    assert int(a.min()) >= 0 and int(a.max()) < n
    want = torch.stack([_lerp_cpu(pts[b], pts[idx[b]], a[b], r) for b in range(B)])
    assert torch.equal(mixed.cpu().view(torch.int32), want.view(torch.int32))
    emd = vpn_amd.EarthMoverDistanceLoss()
    for b in range(B):                                           # the reference's shape: B auctions on batches of one
        d1, a1 = emd(dp[b][None], dp[int(idx[b])][None], 0.005, 100)
        assert torch.equal(a1[0], assign[b]) and torch.equal(d1[0], dist[b]), b


def test_stage_makes_no_host_synchronisation():
    import vpn_amd
    from vpn_amd import ops
    g = torch.Generator().manual_seed(2)
    B, N = 8, 2048
    pts = (torch.rand(B, N, 3, generator=g) - 0.5).to(DEV)
    rgbs, sils = torch.rand(B, 3, 32, 32, generator=g).to(DEV), torch.rand(B, 1, 32, 32, generator=g).to(DEV)
    idx = ops.partner_indices(torch.randperm(B, generator=g), B, DEV)

    def stage():
        r, s, p = vpn_amd.cut_mix_data(rgbs, sils, pts)
        q = vpn_amd.cut_mix_batch_points(pts, idx, 0.03)
        m = vpn_amd.mixup_points(p)
        return r, s, p, q, m

    stage()                                                      # warm-up: code objects, the auction's LDS limit
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        res = stage()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in res)


def test_stage_captures_into_a_graph():
    import vpn_amd
    from vpn_amd import ops
    g = torch.Generator().manual_seed(3)
    B, N = 8, 2048
    pts = (torch.rand(B, N, 3, generator=g) - 0.5).to(DEV)
    idx = ops.partner_indices(torch.randperm(B, generator=g), B, DEV)
    idx2 = ops.partner_indices(torch.randperm(B, generator=g), B, DEV)

    def stage():
        p = vpn_amd.cut_mix_batch_points(pts, idx, -0.04, seed=5)
        return p, vpn_amd.mixup_points(p, ratio=0.4, indices=idx2)

    want = stage()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = stage()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    pts.add_(0.01)                                               # the replay reads the inputs where they are
    want = stage()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
