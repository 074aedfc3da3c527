"""The auction recovers a sample whose workgroups could not all be resident together.

With G > 1 workgroups per sample the auction's group barrier needs every workgroup of the sample resident at once; when
another process or stream holds CUs that may not hold, the bounded wait gives up and flags the sample.  Every launch with
G > 1 is therefore followed, on the same stream, by a launch at G = 1 that recomputes exactly the flagged samples.  These
tests drive that path deterministically through the test hook of vpn_emd_fwd_ex (bit b of the mask: sample b gives up at
its first group barrier, without waiting) and require the result of a G = 1 run -- the oracle's bits -- with the number of
recomputed samples counted on the device."""
import os

import pytest
import torch

from oracle import vpn_oracle as O

DEV = 'cuda'
MASK = 0b10100101                  # samples 0, 2, 5, 7 of a batch of 8 give up
EPS, ITERS = 0.005, 50


def _clouds(B, n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(B, n, 3, generator=gen), torch.rand(B, n, 3, generator=gen)


def _fwd(x1, x2, max_group, mask=None):
    """One auction through the C ABI on the current stream: vpn_emd_fwd_ex with `mask`, or plain vpn_emd_fwd for None."""
    import vpn_amd
    L, p = vpn_amd._lib.lib(), vpn_amd._lib.ptr
    B, n, _ = x1.shape
    dist = torch.full((B, n), -7.0, device=DEV)
    assign = torch.full((B, n), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty((max(1, L.vpn_emd_workspace(B, n) // 4),), device=DEV)
    args = (p(x1), p(x2), B, n, EPS, ITERS, p(dist), p(assign), p(ws), max_group, vpn_amd._lib.stream())
    if mask is None:
        vpn_amd._lib.call('vpn_emd_fwd', *args)
    else:
        vpn_amd._lib.call('vpn_emd_fwd_ex', *args, mask)
    return dist, assign


@pytest.fixture
def form():
    """VPN_EMD_FORM for the duration of one test (the library reads it on every call)."""
    old = os.environ.get('VPN_EMD_FORM')

    def set_form(f):
        os.environ['VPN_EMD_FORM'] = f
    yield set_form
    if old is None:
        os.environ.pop('VPN_EMD_FORM', None)
    else:
        os.environ['VPN_EMD_FORM'] = old


@pytest.mark.gpu
@pytest.mark.parametrize('kernel,n', [('team', 2048), ('team', 1030), ('local', 3000), ('streaming', 1030)])
def test_given_up_samples_are_recomputed(form, kernel, n):
    import vpn_amd
    form(kernel)
    B = 8
    c1, c2 = _clouds(B, n, 500 + n)
    x1, x2 = c1.to(DEV), c2.to(DEV)
    d1, a1 = _fwd(x1, x2, 1, 0)                                  # one workgroup per sample: no group barrier at all
    assert vpn_amd.emd_last_group() == 1
    r0 = vpn_amd.emd_recovered_samples()
    d, a = _fwd(x1, x2, 4, MASK)
    assert vpn_amd.emd_last_group() == 4                         # the group barrier really ran (and gave up)
    assert vpn_amd.emd_recovered_samples() - r0 == bin(MASK).count('1')
    assert not bool(torch.isnan(d).any()) and int(a.min()) >= 0 and int(a.max()) < n
    assert torch.equal(a, a1) and torch.equal(d, d1)
    rd, ra = O.emd_auction(c1, c2, EPS, ITERS)
    assert torch.equal(a.cpu(), ra) and torch.equal(d.cpu(), rd)
    # mask 0: nothing recomputed, the same bits as plain vpn_emd_fwd
    r1 = vpn_amd.emd_recovered_samples()
    d0, a0 = _fwd(x1, x2, 4, 0)
    dp, ap = _fwd(x1, x2, 4)
    assert vpn_amd.emd_last_group() == 4
    assert vpn_amd.emd_recovered_samples() == r1
    assert torch.equal(a0, ap) and torch.equal(d0, dp) and torch.equal(a0, a1) and torch.equal(d0, d1)


@pytest.mark.gpu
def test_recovery_launch_replays_from_a_graph(form):
    """The recovery is enqueued without any host synchronisation: a captured call replays it."""
    import vpn_amd
    from vpn_amd import ops
    form('team')
    B, n = 8, 2048
    c1, c2 = _clouds(B, n, 77)
    x1, x2 = c1.to(DEV), c2.to(DEV)
    d1, a1 = _fwd(x1, x2, 1, 0)
    old = ops.EMD_TEST_GIVEUP_MASK
    ops.EMD_TEST_GIVEUP_MASK = MASK
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.EmdFunction.apply(x1, x2, EPS, ITERS, 4)        # warm-up outside the capture (LDS limits, allocator)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            d, a = ops.EmdFunction.apply(x1, x2, EPS, ITERS, 4)
    finally:
        ops.EMD_TEST_GIVEUP_MASK = old
    assert vpn_amd.emd_last_group() == 4
    for _ in range(2):
        r0 = vpn_amd.emd_recovered_samples()
        d.fill_(float('nan'))
        a.fill_(-1)
        graph.replay()
        assert vpn_amd.emd_recovered_samples() - r0 == bin(MASK).count('1')
        assert torch.equal(a, a1) and torch.equal(d, d1)


@pytest.mark.gpu
def test_trainstep_with_given_up_samples_equals_the_unforced_step():
    """The auction inside TrainStepLossFunction, on its side stream beside the step's other kernels: forcing samples to
    give up changes neither the five terms nor the gradient by a single bit."""
    import vpn_amd
    from vpn_amd import ops
    assert ops.EMD_SIDE_STREAM
    B, K, n, H = 8, 16, 128, 64                                  # the reference's K and n: N = M = 2048
    g = torch.Generator().manual_seed(11)
    v = (torch.rand(B, K, 3, generator=g) + 0.1) / torch.tensor([8.0, 10.0, 10.0])
    params = torch.cat([v, torch.rand(B, K, 4, generator=g), 0.35 * (torch.rand(B, K, 3, generator=g) * 2 - 1)], 2)
    gt_view = torch.rand(B, K * n, 3, generator=g) - 0.5
    dists, elevs = 1.0 + 0.5 * torch.rand(B, generator=g), 20.0 + 20.0 * torch.rand(B, generator=g)
    azims, angles = 360.0 * torch.rand(B, generator=g), 30.0 * torch.rand(B, generator=g)
    gt_canon = O.view_to_obj_points(gt_view, dists, elevs, azims, angles)
    gt_sil = (torch.rand(B, 1, H, H, generator=g) > 0.6).float()
    params, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles = (
        x.to(DEV) for x in (params, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles))
    kinds = vpn_amd.kinds_tensor([1] * 4 + [0] * (K - 4), DEV)
    w = (1.0, 0.5, 1.0, 0.1, 1.0)

    def step(mask):
        old = ops.EMD_TEST_GIVEUP_MASK
        ops.EMD_TEST_GIVEUP_MASK = mask
        try:
            p = params.clone().requires_grad_(True)
            out = vpn_amd.TrainStepLossFunction.apply(p, kinds, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles, n, 31,
                                                      0, H, H, w)
            out[5].backward()
        finally:
            ops.EMD_TEST_GIVEUP_MASK = old
        return torch.stack([o.detach() for o in out]), p.grad
    t0, g0 = step(0)
    r0 = vpn_amd.emd_recovered_samples()
    t1, g1 = step(MASK)
    assert vpn_amd.emd_last_group() > 1
    assert vpn_amd.emd_recovered_samples() - r0 == bin(MASK).count('1')
    assert bool(torch.isfinite(t1).all()) and bool(torch.isfinite(g1).all())
    assert torch.equal(t0, t1) and torch.equal(g0, g1)
