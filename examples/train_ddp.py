"""Data-parallel training loop of the reference (train.py:211-296) on the drop-in surface: BASELINE config C5
(K=64 primitives, 256x256, one process per GPU, DDP).

    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 examples/train_ddp.py [--steps 20]
    ... examples/train_ddp.py --loss trainstep [--cuboids C] [--steps 20]

Two losses:

  * `--loss hip_loss` (default): the hot path alone (HotPathLossFunction: Chamfer + silhouette), K = 64 at 256 x 256;
  * `--loss trainstep`: the step train.py really runs (train.py:243-262) -- TrainStepLossFunction with all five terms
    (view-centred Chamfer, canonical Chamfer, silhouette, VP-diversity, EMD) at the reference's weights (config.py:13-17)
    and shapes (K = 16 primitives, SAMPLE_NUM = 128: N = M = 2048, as the EMD term needs), the first C of the primitives
    cuboids (`--cuboids C`, train.py:112-116), a host seed per step.  The EMD auction shares the GPU with the step's other
    kernels and, when several ranks share one GPU, with the other ranks: a sample whose auction workgroups cannot all be
    resident is recomputed by the auction itself (vpn_amd.emd_recovered_samples() counts them), so any placement of ranks
    gives the same result; one process per GPU is what is fast.

The reference's ResNet-18 trunk + three heads (modules/network/vpnet_one_resnet.py:28-43, :100-106; 23.4 M
parameters = 93.5 MB of fp32 gradients per step at K=64) is out of scope: a stand-in
network with the same three heads takes its place, wrapped in torch's DistributedDataParallel over RCCL exactly as the
real one would be:

  * the whole loss of the step is ONE autograd node (HotPathLossFunction: sampler -> Chamfer -> raster + image losses;
    TrainStepLossFunction for --loss trainstep),
    so backward runs  hot-path backward -> head post-processing backward -> network backward;  DDP's reducer launches
    the bucketed all-reduce of a bucket of NETWORK gradients (bucket_cap_mb, 25 MB default: 4 buckets for 93.5 MB) as
    soon as the bucket is complete, on its own stream: the collective of the last layers' buckets overlaps the
    backward of the earlier layers.  Nothing of the hot path is exchanged: its gradient w.r.t. (v, q, t) is per sample
    and flows into the local network replica (the kernel-only exchange of BASELINE config C4 is vpn_amd.dist);
  * the reference's resnet18 carries an `fc` layer its forward never uses (vpnet_one_resnet.py:45-57): under DDP that
    needs find_unused_parameters=True (or deleting the layer).  The stand-in has an unused head on purpose so the flag
    is exercised;
  * every rank draws its own surface points: the Philox key is (seed of the step, GLOBAL sample index), so the
    union over ranks is the batch a single process would have drawn (sample_base = rank * B_local);
  * the reference's loop divides by BATCH_SIZE constants and crashes on a last partial batch (train.py:127,137,289);
    nothing here depends on the batch size.

`run(rank, world, device, loss_fn, ...)` is the loop with the loss injectable: tests/test_ddp_cpu.py drives it over gloo on
the CPU with the oracle as the loss (the HIP operators need a GPU) and checks the DDP gradients against a single
process."""
import argparse
import os
import sys

import torch
import torch.distributed as dist
import torch.nn as nn
from torch.nn.parallel import DistributedDataParallel as DDP

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Heads(nn.Module):
    """Stand-in for VPNetOneRes (vpnet_one_resnet.py:28-43): features -> raw head outputs (volumes [B,3K], rotates
    [B,4K], translates [B,3K]).  `unused_fc` plays the resnet's never-called fc layer."""

    def __init__(self, feat, K, hidden=256):
        super().__init__()
        self.trunk = nn.Sequential(nn.Linear(feat, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU())
        self.volume_fc, self.rotate_fc, self.translate_fc = nn.Linear(hidden, 3 * K), nn.Linear(hidden, 4 * K), nn.Linear(hidden, 3 * K)
        self.unused_fc = nn.Linear(hidden, 10)

    def forward(self, x):
        h = self.trunk(x)
        return self.volume_fc(h), self.rotate_fc(h), self.translate_fc(h)


def hip_loss(heads_out, batch, kinds, sample_num, seed, sample_base, size):
    """Loss of one step on the HIP hot path: head post-processing -> one autograd node for everything else."""
    import vpn_amd
    gt_points, gt_sil, cam = batch
    params = vpn_amd.pack_head_outputs(*heads_out)                                  # vpnet_one_resnet.py:34-41, :67-85
    out = vpn_amd.HotPathLossFunction.apply(params, vpn_amd.kinds_tensor(kinds, params.device), cam, gt_points, gt_sil, None,
                                            sample_num, seed, sample_base, size, size, vpn_amd.config.RASTER_SIGMA,
                                            vpn_amd.config.RASTER_GAMMA, vpn_amd.config.RASTER_Z_FAR, 1.0, 1.0, 0.0)
    return out[2]


TRAINSTEP_WEIGHTS = (1.0, 0.0, 0.0, 0.1, 1.0)   # (L_VIEW_CD, L_CAN_CD, L_SIL, L_VP_DIV, L_EMD), config.py:13-17


def trainstep_loss(heads_out, batch, kinds, sample_num, seed, sample_base, size):
    """Loss of one step of train.py (:243-262) on the HIP path: head post-processing -> TrainStepLossFunction (all five
    terms in one autograd node).  batch = make_trainstep_batch's (gt_view, gt_canon, gt_sil, dists, elevs, azims, angles)."""
    import vpn_amd
    from vpn_amd import config
    weights = (config.L_VIEW_CD, config.L_CAN_CD, config.L_SIL, config.L_VP_DIV, config.L_EMD)
    params = vpn_amd.pack_head_outputs(*heads_out)
    out = vpn_amd.TrainStepLossFunction.apply(params, vpn_amd.kinds_tensor(kinds, params.device), *batch, sample_num, int(seed),
                                              sample_base, size, size, weights)
    return out[5]


def make_trainstep_batch(B, K, feat, M, size, device, seed, lo, hi):
    """Synthetic global batch of the five-term step (seeded identically on every rank), this rank's slice [lo, hi):
    features, then the view-centred GT cloud [B,M,3], a canonical GT cloud [B,M,3], silhouettes [B,1,size,size] and the
    cameras (dists, elevs, azims, angles [B]: the arguments of view_to_obj_points, train.py:158-161)."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, feat, generator=g)
    gt_view = torch.rand(B, M, 3, generator=g) - 0.5
    gt_canon = torch.rand(B, M, 3, generator=g) - 0.5
    gt_sil = (torch.rand(B, 1, size, size, generator=g) > 0.7).float()
    dists = 1.0 + 0.5 * torch.rand(B, generator=g)
    elevs = 20.0 + 20.0 * torch.rand(B, generator=g)
    azims = 360.0 * torch.rand(B, generator=g)
    angles = 30.0 * torch.rand(B, generator=g)
    dt = torch.get_default_dtype()
    return feats[lo:hi].to(device), tuple(x[lo:hi].to(device, dt) for x in (gt_view, gt_canon, gt_sil, dists, elevs, azims, angles))


def make_batch(B, K, feat, M, size, device, seed, lo, hi):
    """Synthetic global batch (seeded identically on every rank), this rank's slice [lo, hi)."""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(B, feat, generator=g)
    gt_points = torch.rand(B, M, 3, generator=g) - 0.5
    gt_sil = (torch.rand(B, 1, size, size, generator=g) > 0.7).float()
    cam = torch.tensor([[1.0, 0.0, 0.0]]).expand(B, 3).contiguous()                 # train.py:172-174
    return feats[lo:hi].to(device), (gt_points[lo:hi].to(device), gt_sil[lo:hi].to(device), cam[lo:hi].to(device))


def run(rank, world, device, loss_fn, steps=3, global_batch=8, K=8, feat=32, sample_num=16, M=64, size=16, lr=1e-2,
        bucket_cap_mb=25, log=None, make_optimizer=None, batch_fn=None, cuboids=0):
    """The DDP loop.  loss_fn(heads_out, batch, kinds, sample_num, seed, sample_base, size) -> scalar local-mean loss;
    batch_fn(B, K, feat, M, size, device, seed, lo, hi) -> (features, batch) builds it (default make_batch;
    make_trainstep_batch for trainstep_loss); the first `cuboids` primitives are cuboids, the rest spheres.
    Returns the model (unwrapped) after `steps` optimiser steps."""
    assert global_batch % world == 0
    per = global_batch // world
    lo, hi = rank * per, (rank + 1) * per
    torch.manual_seed(1234)                                                         # same initial weights on every rank
    net = Heads(feat, K).to(device)
    model = DDP(net, device_ids=[device.index] if device.type == 'cuda' else None, bucket_cap_mb=bucket_cap_mb,
                find_unused_parameters=True) if world > 1 or dist.is_initialized() else net
    opt = make_optimizer(net.parameters()) if make_optimizer else torch.optim.Adam(net.parameters(), lr=lr)   # train.py:93-103
    kinds = [1] * cuboids + [0] * (K - cuboids)                                     # config.py:33-34, train.py:112-116
    batch_fn = batch_fn or make_batch
    for it in range(steps):
        feats, batch = batch_fn(global_batch, K, feat, M, size, device, 100 + it, lo, hi)
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(model(feats), batch, kinds, sample_num, 1000 + it, lo, size)  # local mean; DDP averages the gradients
        loss.backward()                                                             # bucketed all-reduce overlaps this
        opt.step()
        if log is not None:
            log(it, loss)
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--global-batch', type=int, default=64)
    ap.add_argument('--loss', choices=['hip_loss', 'trainstep'], default='hip_loss')
    ap.add_argument('--prims', type=int, default=None)        # hip_loss: 64 (C5); trainstep: 16 (config.py:34)
    ap.add_argument('--cuboids', type=int, default=0)         # the first C primitives are cuboids (config.py:33)
    ap.add_argument('--sample-num', type=int, default=128)    # config.py:8
    ap.add_argument('--size', type=int, default=None)         # hip_loss: 256; trainstep: 128 (config.py:49)
    ap.add_argument('--optimizer', default='torch', choices=('torch', 'hip'),
                    help='hip: vpn_amd.Adam (one launch per step, csrc/optim.hip) with the reference\'s betas (0.9, 0.99)')
    args = ap.parse_args()
    trainstep = args.loss == 'trainstep'
    K = args.prims or (16 if trainstep else 64)
    size = args.size or (128 if trainstep else 256)
    if not 0 <= args.cuboids <= K:
        ap.error('--cuboids must be between 0 and the number of primitives')
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    ngpu = torch.cuda.device_count()
    shared = world > ngpu                                     # more ranks than GPUs: ranks share devices
    dev = torch.device('cuda', local_rank % ngpu)
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29533')
        if shared:                                            # RCCL takes one rank per device: gloo (host copies) instead
            dist.init_process_group('gloo', rank=rank, world_size=world)
        else:
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)    # RCCL over xGMI

    def hip_adam(params):
        import vpn_amd
        return vpn_amd.Adam(params, lr=1e-3, betas=(0.9, 0.99))                     # train.py:83

    def log(it, loss):
        if rank == 0:
            print('step %3d  local loss %.5f' % (it, float(loss.detach())), flush=True)
    run(rank, world, dev, trainstep_loss if trainstep else hip_loss, steps=args.steps, global_batch=args.global_batch, K=K,
        feat=64, sample_num=args.sample_num, M=K * args.sample_num if trainstep else 2048, size=size, lr=1e-3, log=log,
        batch_fn=make_trainstep_batch if trainstep else None, cuboids=args.cuboids,
        make_optimizer=hip_adam if args.optimizer == 'hip' else None)
    if trainstep and rank == 0:
        import vpn_amd
        print('EMD samples recomputed by the auction (workgroups not co-resident): %d' % vpn_amd.emd_recovered_samples(),
              flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
