"""The five-term training step of examples/train_ddp.py (`--loss trainstep`: make_trainstep_batch, mixed primitive kinds)
driven through the DDP loop `run()` over gloo with world size 2 on the CPU.  The HIP operators need a GPU, so the loss
injected here is the oracle's train_step restated for a shard -- the Philox draws keyed by the GLOBAL sample index
(sample_base), which oracle.train_step fixes at 0 -- in float64: two ranks must end with the weights a single process
gets on the whole batch."""
import importlib.util
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

K, CUBOIDS, SAMPLE_NUM, SIZE, STEPS, GLOBAL_BATCH = 4, 1, 8, 16, 3, 4
M = K * SAMPLE_NUM                  # the EMD term needs as many GT points as predicted ones


def _example():
    spec = importlib.util.spec_from_file_location('train_ddp', os.path.join(ROOT, 'examples', 'train_ddp.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def oracle_trainstep_loss(heads_out, batch, kinds, sample_num, seed, sample_base, size):
    """oracle.train_step's five terms (train.py:243-262) on this rank's shard, differentiable through the head outputs."""
    from oracle import vpn_oracle as O
    gt_view, gt_canon, gt_sil, dists, elevs, azims, angles = batch
    w = _example().TRAINSTEP_WEIGHTS
    p = O.head_post_process(*heads_out)
    B = p.shape[0]
    pred = O.sample_primitives(p, kinds, O.philox_uniforms(seed, sample_base, B, len(kinds), sample_num).to(p.dtype))
    total = O.chamfer_loss(pred, gt_view) * w[0]
    total = total + O.chamfer_loss(O.view_to_obj_points(pred, dists, elevs, azims, angles), gt_canon) * w[1]
    if w[2]:
        alpha, _ = O.raster(p, kinds, torch.tensor([[1.0, 0.0, 0.0]], dtype=p.dtype).expand(B, 3), size, size)
        total = total + (alpha - gt_sil.reshape(B, size, size)).abs().mean() * w[2]
    total = total + O.chamfer_loss(p[:, :, 7:10], gt_view, w1=0.5, w2=1.0) * w[3]
    _, assign = O.emd_auction(pred.detach(), gt_view, 0.005, 50)
    picked = torch.gather(gt_view, 1, assign.long()[..., None].expand(-1, -1, 3))
    return total + torch.sqrt(((pred - picked) ** 2).sum(-1)).mean() * w[4]


def _run(rank, world):
    dtype = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)                     # as tests/test_ddp_cpu.py: the loop, not the CPU's BLAS
    try:
        ex = _example()
        return ex.run(rank, world, torch.device('cpu'), oracle_trainstep_loss, steps=STEPS, global_batch=GLOBAL_BATCH, K=K,
                      feat=16, sample_num=SAMPLE_NUM, M=M, size=SIZE, bucket_cap_mb=0.01,
                      make_optimizer=lambda p: torch.optim.SGD(p, lr=0.05), batch_fn=ex.make_trainstep_batch, cuboids=CUBOIDS)
    finally:
        torch.set_default_dtype(dtype)


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    net = _run(rank, world)
    if rank == 0:
        torch.save({k: v.clone() for k, v in net.state_dict().items()}, out)
    dist.destroy_process_group()


def test_trainstep_batch_builder_shapes():
    ex = _example()
    feats, batch = ex.make_trainstep_batch(6, K, 16, M, SIZE, torch.device('cpu'), 3, 2, 5)
    assert feats.shape == (3, 16)
    gt_view, gt_canon, gt_sil, dists, elevs, azims, angles = batch
    assert gt_view.shape == gt_canon.shape == (3, M, 3) and gt_sil.shape == (3, 1, SIZE, SIZE)
    assert dists.shape == elevs.shape == azims.shape == angles.shape == (3,)
    _, whole = ex.make_trainstep_batch(6, K, 16, M, SIZE, torch.device('cpu'), 3, 0, 6)
    assert all(torch.equal(a, b[2:5]) for a, b in zip(batch, whole))      # a shard is a slice of the global batch


def test_trainstep_ddp_two_ranks_match_single_process(tmp_path):
    out = str(tmp_path / 'w.pt')
    port = 29900 + ((os.getpid() + 1000) % 2000)
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    got = torch.load(out, weights_only=True)
    ref = _run(0, 1).state_dict()
    assert set(got) == set(ref)
    for k in ref:
        if k.startswith('unused_fc'):
            assert torch.equal(got[k], ref[k])
        else:
            assert torch.allclose(got[k], ref[k], rtol=1e-5, atol=1e-6), k
    moved = sum(float((ref[k] - _example().Heads(16, K).state_dict()[k]).abs().sum()) for k in ref if 'trunk' in k)
    assert moved > 0
