"""CPU checks of the evaluation stage (modules/evaluation.py, csrc/evaluate.hip): the entry points exist, size the state as
documented and validate their arguments without a GPU; the accumulate kernel uses no scratch; the host side of the meter
(merge, result, report) on hand-filled states; the all-reduce of the state over two gloo ranks; the g9 fixture."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN, ROOT, load_golden
from test_kernel_budget_cpu import _resources

SIZE_CAP = 402312            # the largest fixture committed before g9_eval.npz
NAMES = ['airplane', 'rifle', 'display', 'table']


def test_entry_points_exist_and_validate_without_a_gpu():
    import vpn_amd._lib as lib
    L = lib.lib()
    assert L.vpn_abi_version() == lib.ABI_VERSION == 9
    # 3 + 2 C doubles and 2 + C int64 in one buffer
    assert L.vpn_eval_state_size(13) == (3 + 2 * 13) * 8 + (2 + 13) * 8 == 352
    assert L.vpn_eval_state_size(1) == 64
    assert L.vpn_eval_state_size(0) == 0 and L.vpn_eval_state_size(-3) == 0
    f = ctypes.c_void_p(64)              # never dereferenced: every call below is refused before a launch
    acc = L.vpn_eval_accumulate
    assert acc(None, None, None, None, 8, 128, 128, 13, 1.0, 1.0, 1.0, None, None, None, None) == -1
    for missing in range(5):             # dist1, dist2, class_index, state, cd_b: each is required
        a = [f, f, f, f, f]
        a[missing] = None
        assert acc(a[0], a[1], None, a[2], 8, 128, 96, 13, 1.0, 1.0, 1.0, a[3], a[4], None, None) == -1, missing
    assert acc(f, f, f, f, 8, 128, 128, 13, 1.0, 1.0, 1.0, f, f, None, None) == -1          # emd_dist without emd_b
    assert acc(f, f, f, f, 8, 128, 96, 13, 1.0, 1.0, 1.0, f, f, f, None) == -1              # emd_dist with N != M
    for B, N, M, C in ((0, 128, 128, 13), (8, 0, 128, 13), (8, 128, 0, 13), (8, 128, 128, 0), (-1, 128, 128, 13)):
        assert acc(f, f, None, f, B, N, M, C, 1.0, 1.0, 1.0, f, f, None, None) == -1, (B, N, M, C)
    assert acc(f, f, None, f, 8, 128, 96, 13, 1.0, 1.0, 1.0, ctypes.c_void_p(68), f, None, None) == -1   # state not 8-byte aligned


def test_accumulate_kernel_uses_no_scratch():
    r = _resources('evaluate.hip', 'eval_accumulate_kernel')
    assert r['ScratchSize'] == 0, r
    assert r['LDS'] <= 16 * 1024, r              # the staged chunk of 1024 samples: 12 KB and the reduction cells


def _filled(C, seed):
    """A state as an evaluation would leave it, filled by hand; class 1 never occurs."""
    from vpn_amd import ops
    g = torch.Generator().manual_seed(seed)
    s = ops.eval_state(C, 'cpu')
    d, n = ops.eval_state_fields(s, C)
    n[2:] = torch.randint(1, 9, (C,), generator=g)
    n[2 + 1] = 0
    n[0] = 3 + seed
    n[1] = seed % 2
    d[0], d[1] = torch.rand(2, generator=g, dtype=torch.float64) * float(n[0])
    d[3:3 + C] = torch.rand(C, generator=g, dtype=torch.float64) * n[2:]
    d[3 + C:] = torch.rand(C, generator=g, dtype=torch.float64) * n[2:]
    d[3 + 1] = d[3 + C + 1] = 0.0
    return s


def test_merge_is_the_field_wise_sum():
    from vpn_amd import EvaluationMeter, ops
    C = len(NAMES)
    a, b = _filled(C, 1), _filled(C, 2)
    m = EvaluationMeter.merge(a, b)
    (da, na), (db, nb), (dm, nm) = (ops.eval_state_fields(t, C) for t in (a, b, m))
    assert torch.equal(dm, da + db) and torch.equal(nm, na + nb)
    assert m.data_ptr() not in (a.data_ptr(), b.data_ptr())
    assert torch.equal(ops.eval_state_fields(a, C)[1], na)              # the inputs are left as they were
    with pytest.raises(ValueError):
        EvaluationMeter.merge(a, _filled(C + 1, 1))


def test_result_and_report_on_a_hand_filled_state(capsys):
    import vpn_amd
    from vpn_amd import EvaluationMeter, ops
    assert vpn_amd.EvaluationMeter is vpn_amd.modules.EvaluationMeter is vpn_amd.modules.evaluation.EvaluationMeter
    C = len(NAMES)
    s = _filled(C, 2)                                                   # n_invalid == 0
    d, n = ops.eval_state_fields(s, C)
    meter = EvaluationMeter(NAMES, 'cpu')
    meter.load_state(s)
    res = meter.result()
    nb = int(n[0])
    assert res['n_batches'] == nb and res['n_invalid'] == 0 and res['class_n'] == n[2:].tolist()
    assert res['cd'] == float(d[0]) / nb and res['emd'] == float(d[1]) / nb
    for c in range(C):
        if c == 1:
            assert res['class_cd'][c] is None and res['class_emd'][c] is None
        else:
            assert res['class_cd'][c] == float(d[3 + c]) / int(n[2 + c])
            assert res['class_emd'][c] == float(d[3 + C + c]) / int(n[2 + c])
    assert all(type(v) in (float, int, type(None)) for k in ('class_cd', 'class_emd', 'class_n') for v in res[k])
    capsys.readouterr()
    meter.report(epoch=7)
    out = capsys.readouterr().out
    lines = out.splitlines()
    assert '\nEpoch 7\n' in out and lines.count('=' * 30) == 2
    rows = [l for l in lines if 'cd loss' in l and not l.startswith('total')]
    assert len(rows) == C - 1 and not any(l.startswith('rifle') for l in lines)       # the empty class prints no line
    for c, name in enumerate(NAMES):
        if c != 1:
            assert name + ' \t\tcd loss = %.6f, emd loss = %.6f' % (res['class_cd'][c], res['class_emd'][c]) in lines
    assert 'total \t\tcd loss = %.6f, emd loss = %.6f' % (res['cd'], res['emd']) in lines
    assert 'n_invalid' not in out
    # Chamfer only: the other script's format; n_invalid is shown when it is not zero
    s1 = _filled(C, 1)
    d1, n1 = ops.eval_state_fields(s1, C)
    m1 = EvaluationMeter(NAMES, 'cpu', emd=False)
    m1.load_state(s1)
    r1 = m1.report()
    out = capsys.readouterr().out
    lines = out.splitlines()
    assert r1['emd'] is None and r1['class_emd'] == [None] * C and r1['n_invalid'] == 1
    assert lines.count('=' * 28) == 2 and 'Epoch' not in out
    for c, name in enumerate(NAMES):
        if c != 1:
            assert name + ' avg cd loss = %.6f' % r1['class_cd'][c] in lines
    assert not any(l.startswith('rifle') for l in lines)
    assert 'total avg cd loss = %.6f' % r1['cd'] in lines
    assert any(l.startswith('n_invalid = 1') for l in lines)
    m1.reset()
    r0 = m1.result()
    assert r0['n_batches'] == 0 and r0['cd'] is None and r0['class_cd'] == [None] * C and r0['class_n'] == [0] * C
    with pytest.raises(ValueError):
        EvaluationMeter([], 'cpu')
    with pytest.raises(RuntimeError, match='GPU only'):                 # there is no CPU path for the metrics themselves
        m1.update(torch.rand(2, 8, 3), torch.rand(2, 8, 3), [0, 1])
    with pytest.raises(ValueError, match='as many predicted'):
        meter.update(torch.rand(2, 8, 3), torch.rand(2, 9, 3), [0, 1])


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import vpn_amd
    from vpn_amd import EvaluationMeter
    meter = EvaluationMeter(NAMES, 'cpu')
    mine = _filled(len(NAMES), 1 + rank)
    meter.load_state(mine)
    res = meter.result(group=dist.group.WORLD)
    assert torch.equal(meter.state, mine)                               # the rank's own state is not overwritten
    torch.save(res, out % rank)
    dist.destroy_process_group()


def test_result_over_two_ranks_equals_the_merged_result(tmp_path):
    from vpn_amd import EvaluationMeter
    out = str(tmp_path / 'r%d.pt')
    port = 29500 + ((os.getpid() + 977) % 2000)
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    meter = EvaluationMeter(NAMES, 'cpu')
    meter.load_state(EvaluationMeter.merge(_filled(len(NAMES), 1), _filled(len(NAMES), 2)))
    want = meter.result()
    assert want['n_batches'] == 4 + 5 and want['n_invalid'] == 1
    for rank in range(2):
        assert torch.load(out % rank, weights_only=True) == want, rank


def test_g9_fixture_holds_the_three_class_cases():
    path = os.path.join(GOLDEN, 'g9_eval.npz')
    assert os.path.getsize(path) <= SIZE_CAP
    with np.load(path, allow_pickle=False):
        pass
    z = load_golden('g9_eval')
    sizes = z['batch_sizes'].tolist()
    C = int(z['num_classes'])
    cls = z['class_index']
    assert sum(sizes) == z['pred'].shape[0] == z['gt'].shape[0] == cls.numel() == z['loss_b'].numel()
    assert sizes[-1] < sizes[0] and int(z['n_batches']) == len(sizes)
    assert z['class_sum'].dtype == torch.float64 and z['total'].dtype == torch.float64 and z['loss_b'].dtype == torch.float32
    per_batch = list(torch.split(cls, sizes))
    counts = torch.bincount(cls, minlength=C)
    assert torch.equal(counts, z['class_n']) and int(cls.min()) >= 0 and int(cls.max()) < C
    assert bool((counts == 0).any())                                                    # a class that never occurs
    assert any(int(torch.bincount(b, minlength=C).max()) >= 3 for b in per_batch)       # several times within one batch
    assert any(all(bool((b == c).any()) for b in per_batch) for c in range(C))          # a class hit in every batch
    # the recorded sums are the bookkeeping of test.py:104-108 applied to the recorded per-sample losses
    total, sums = 0.0, [0.0] * C
    for lb, cb in zip(torch.split(z['loss_b'], sizes), per_batch):
        total += lb.mean().item()
        for v, c in zip(lb, cb):
            sums[int(c)] += v.item()
    assert sums == z['class_sum'].tolist() and total == float(z['total_sum']) and total / len(sizes) == float(z['total'])
