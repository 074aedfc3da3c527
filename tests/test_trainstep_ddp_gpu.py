"""Two ranks on ONE GPU running the five-term training step (TrainStepLossFunction: view-centred and canonical Chamfer,
silhouette, VP-diversity, EMD) on their shards, at the reference's shapes (K = 16, n = 128: N = M = 2048).  The ranks'
auctions share the device with each other and with their own steps' kernels, so a sample's auction workgroups need not
all be resident together -- the case the auction's G = 1 recovery exists for.  The shards' gradients meet through
vpn_amd.dist.GradAllGather over gloo and must equal the single-process batch: bit for bit without the render (every
term's gradient is per sample and B, world are powers of two), <= 1e-6 relative with it (as tests/test_dist_gpu.py),
the loss mean within 1e-6 relative, nothing NaN.

The children are forked from the fork server tests/conftest.py starts before any test touches the GPU."""
import multiprocessing as mp
import os
import sys

import pytest
import torch

from conftest import ROOT

B, K, n, H = 8, 16, 128, 64
SEED = 2024
WEIGHTS = {'reference': (1.0, 0.0, 0.0, 0.1, 1.0),             # config.py:13-17
           'all': (1.0, 0.5, 1.0, 0.1, 1.0)}
KINDS = {'spheres': [0] * K, 'mixed': [1] * 5 + [0] * (K - 5)}   # the first C primitives are cuboids (train.py:112-116)


def _inputs():
    from oracle import vpn_oracle as O
    g = torch.Generator().manual_seed(17)
    v = (torch.rand(B, K, 3, generator=g) + 0.1) / torch.tensor([8.0, 10.0, 10.0])
    params = torch.cat([v, torch.rand(B, K, 4, generator=g), 0.35 * (torch.rand(B, K, 3, generator=g) * 2 - 1)], 2)
    gt_view = torch.rand(B, K * n, 3, generator=g) - 0.5
    dists = 1.0 + 0.5 * torch.rand(B, generator=g)
    elevs = 20.0 + 20.0 * torch.rand(B, generator=g)
    azims = 360.0 * torch.rand(B, generator=g)
    angles = 30.0 * torch.rand(B, generator=g)
    gt_canon = O.view_to_obj_points(gt_view, dists, elevs, azims, angles)
    gt_sil = (torch.rand(B, 1, H, H, generator=g) > 0.6).float()
    return params, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles


def _step(lo, hi, weights, kinds):
    """Samples [lo, hi) on the GPU: (local mean loss, grad [hi-lo, K, 10]) as CPU tensors."""
    import vpn_amd
    dev = torch.device('cuda', 0)
    params, *rest = [x[lo:hi].to(dev) for x in _inputs()]
    p = params.requires_grad_(True)
    out = vpn_amd.TrainStepLossFunction.apply(p, vpn_amd.kinds_tensor(kinds, dev), *rest, n, SEED, lo, H, H, weights)
    out[5].backward()
    return out[5].detach().cpu(), p.grad.cpu()


def _worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)                                   # both ranks share the one device of the box
    import vpn_amd
    from vpn_amd.dist import GradAllGather, shard_bounds
    lo, hi = shard_bounds(B, rank, world)
    res = {}
    for wname, weights in WEIGHTS.items():
        for kname, kinds in KINDS.items():
            loss, grad = _step(lo, hi, weights, kinds)
            g, l = GradAllGather(B, K, torch.device('cpu'), rank, world).reduce(grad, loss)
            res[wname + '/' + kname] = (g.clone(), l.clone())
    res['recovered'] = vpn_amd.emd_recovered_samples()
    if rank == 0:
        torch.save(res, os.path.join(outdir, 'r0.pt'))
    dist.destroy_process_group()


@pytest.mark.gpu
def test_trainstep_two_ranks_on_one_gpu_match_single_process(tmp_path):
    ctx = mp.get_context('forkserver')
    port = 29700 + ((os.getpid() + 1000) % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        if p.is_alive():
            p.kill()
        assert p.exitcode == 0, 'rank process failed (exit code %s)' % p.exitcode
    got = torch.load(os.path.join(str(tmp_path), 'r0.pt'), weights_only=True)
    print('auction samples recomputed on rank 0: %d' % got['recovered'])
    for wname, weights in WEIGHTS.items():
        for kname, kinds in KINDS.items():
            loss, grad = _step(0, B, weights, kinds)             # the whole batch in this process
            g, l = got[wname + '/' + kname]
            assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(l)), (wname, kname)
            assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
            if weights[2] == 0.0:                              # no render: every term per sample
                assert torch.equal(g, grad), (wname, kname, float((g - grad).abs().max()))
            else:
                assert float((g - grad).abs().max() / grad.abs().max()) <= 1e-6, (wname, kname)
            assert abs(float(l) - float(loss)) <= 1e-6 * abs(float(loss)), (wname, kname, float(l), float(loss))
