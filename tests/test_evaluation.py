"""GPU tests of the evaluation stage (modules/evaluation.py on csrc/evaluate.hip): the Chamfer half pinned to the reference's
own per-sample losses and bookkeeping (tests/golden/g9_eval.npz, captured by tools/make_golden_eval.py), the bookkeeping
against Python's `+= x.item()` bit for bit, the per-sample values against this package's own Chamfer and auction modules, no
host synchronisation, graph replay, and the edge cases."""
import pytest
import torch

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAMES13 = ['airplane', 'rifle', 'display', 'table', 'telephone', 'car', 'chair', 'bench', 'lamp', 'cabinet', 'loudspeaker',
           'sofa', 'watercraft']


def _raw(meter):
    """(sums float64 [3 + 2 C], counts int64 [2 + C]) of a meter's state, on the host."""
    from vpn_amd import ops
    return ops.eval_state_fields(meter.state.cpu(), meter.C)


def _host_bookkeeping(batches, C, emd):
    """test_gcn.py:126-152 (test.py:83-108) in Python floats on per-sample values that are already on the host:
    batches = [(cd_b, emd_b or None, class indices)].  Indices outside [0, C) are counted, not added."""
    tot = {'cd': 0.0, 'emd': 0.0}
    sums = {'cd': [0.0] * C, 'emd': [0.0] * C}
    class_n, n, invalid = [0] * C, 0, 0
    for cd, em, idx in batches:
        tot['cd'] += cd.mean().item()
        if emd:
            tot['emd'] += em.mean().item()
        n += 1
        for b in range(len(cd)):
            c = int(idx[b])
            if not 0 <= c < C:
                invalid += 1
                continue
            sums['cd'][c] += cd[b].item()
            if emd:
                sums['emd'][c] += em[b].item()
            class_n[c] += 1
    return tot, sums, class_n, n, invalid


def _clouds(B, N, M, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, N, 3, generator=g) - 0.5).to(DEV), (torch.rand(B, M, 3, generator=g) - 0.5).to(DEV)


def _clustered(B, n, seed):
    """A uniform cloud and a clustered one (eight blobs) in the unit cube around the origin."""
    g = torch.Generator().manual_seed(seed)
    uniform = torch.rand(B, n, 3, generator=g) - 0.5
    centres = torch.rand(B, 8, 3, generator=g) * 0.6 - 0.3
    which = torch.randint(0, 8, (B, n), generator=g)
    blobs = torch.gather(centres, 1, which[..., None].expand(-1, -1, 3)) + 0.05 * torch.randn(B, n, 3, generator=g)
    return uniform.to(DEV), blobs.clamp(-0.5, 0.5).to(DEV)


def test_chamfer_half_against_the_reference():
    from vpn_amd import EvaluationMeter
    z = load_golden('g9_eval')
    sizes = z['batch_sizes'].tolist()
    C = int(z['num_classes'])
    meter = EvaluationMeter(NAMES13[:C], DEV, emd=False)
    got = []
    for p, g, c in zip(torch.split(z['pred'], sizes), torch.split(z['gt'], sizes), torch.split(z['class_index'], sizes)):
        cd_b, emd_b = meter.update(p.to(DEV), g.to(DEV), c)          # c: a CPU int64 tensor, as a DataLoader yields it
        assert emd_b is None and cd_b.shape == (p.shape[0],) and cd_b.dtype == torch.float32
        got.append(cd_b)
    got = torch.cat(got).cpu()
    e = rel_err(got, z['loss_b'])
    print('per-sample cd rel_err', e)
    assert e <= 1e-4
    res = meter.result()
    sums, counts = _raw(meter)
    assert res['class_n'] == z['class_n'].tolist() == counts[2:].tolist()
    assert res['n_batches'] == int(z['n_batches']) and res['n_invalid'] == 0
    e_cls = rel_err(sums[3:3 + C], z['class_sum'])
    e_tot = abs(res['cd'] - float(z['total'])) / float(z['total'])
    print('class sums rel_err', e_cls, 'total rel_err', e_tot)
    assert e_cls <= 1e-4 and e_tot <= 1e-4
    assert res['emd'] is None and res['class_emd'] == [None] * C
    for c in range(C):
        if int(z['class_n'][c]) == 0:
            assert res['class_cd'][c] is None
        else:
            assert abs(res['class_cd'][c] - float(z['class_sum'][c]) / int(z['class_n'][c])) <= 1e-4 * float(z['class_sum'].max())


def test_bookkeeping_is_exact():
    """The class sums are Python's `+= x.item()` in sample order on the per-sample values the meter returned: bit-equal as
    float64.  The totals: the reference averages a batch in fp32, the kernel in fp64; an fp32 mean of B positive values is
    within (B + 1) * 2^-24 relative of the exact one (B - 1 additions and one division, each within 2^-24, first order), the
    fp64 one within (B + 1) * 2^-53."""
    from vpn_amd import EvaluationMeter
    C, B, n = 5, 8, 256
    meter = EvaluationMeter(NAMES13[:C], DEV, emd=True)
    g = torch.Generator().manual_seed(5)
    batches = []
    for k, b in enumerate((B, B, B, 3)):
        p, q = _clustered(b, n, 50 + k)
        idx = torch.randint(0, C - 1, (b,), generator=g)             # class C - 1 never occurs
        idx[0] = 2                                                   # class 2 in every batch
        cd_b, emd_b = meter.update(p, q, idx.to(DEV))                # a device int64 tensor
        batches.append((cd_b.cpu(), emd_b.cpu(), idx))
    tot, want, class_n, nb, invalid = _host_bookkeeping(batches, C, True)
    sums, counts = _raw(meter)
    assert counts.tolist() == [nb, invalid] + class_n and invalid == 0 and class_n[C - 1] == 0
    assert sums[3:3 + C].tolist() == want['cd']                      # float64 == float64: the same bits
    assert sums[3 + C:].tolist() == want['emd']
    assert float(sums[2]) == 0.0                                     # the ticket slot is back at zero
    res = meter.result()
    for c in range(C):
        if class_n[c]:
            assert res['class_cd'][c] == want['cd'][c] / class_n[c] and res['class_emd'][c] == want['emd'][c] / class_n[c]
    bound = (B + 1) * 2.0 ** -24
    for key, slot in (('cd', 0), ('emd', 1)):
        err = abs(float(sums[slot]) - tot[key]) / tot[key]
        print(key, 'total rel diff', err, 'bound', bound)
        assert err <= bound
        assert res[key] == float(sums[slot]) / nb


@pytest.mark.parametrize('B,N,M', [(4, 128, 96), (2, 2048, 2048), (2, 8192, 2048)])
def test_cd_b_equals_the_chamfer_module(B, N, M):
    from vpn_amd import ChamferDistanceLoss, EvaluationMeter
    p, q = _clouds(B, N, M, N + M)
    want = ChamferDistanceLoss()(p, q, each_batch=True)
    meter = EvaluationMeter(NAMES13, DEV, emd=False)
    cd_b, _ = meter.update(p, q, [b % 13 for b in range(B)])
    assert torch.equal(cd_b, want)
    scaled = EvaluationMeter(NAMES13, DEV, emd=False, cd_scale=0.25)         # a power of two: exact
    cd_s, _ = scaled.update(p, q, [0] * B)
    assert torch.equal(cd_s, want * 0.25)


def test_emd_b_against_the_auction_module():
    from vpn_amd import ChamferDistanceLoss, EarthMoverDistanceLoss, EvaluationMeter
    B, n = 8, 2048
    p, q = _clustered(B, n, 4)
    dist = EarthMoverDistanceLoss()(p, q, 0.005, 50)[0]
    want = torch.sqrt(dist).double().mean(1).float()
    meter = EvaluationMeter(NAMES13, DEV, emd=True)
    idx = torch.arange(B, dtype=torch.int32, device=DEV)
    cd_1, emd_1 = meter.update(p, q, idx)
    cd_2, emd_2 = meter.update(p, q, idx)
    ulps = (emd_1.view(torch.int32) - want.view(torch.int32)).abs().max().item()
    print('emd_b vs rounded fp64 mean: max ulps', ulps, 'values', emd_1.tolist())
    assert ulps <= 1
    assert torch.equal(emd_1, emd_2) and torch.equal(cd_1, cd_2)            # run-to-run: the same bits
    assert torch.equal(cd_1, ChamferDistanceLoss()(p, q, each_batch=True))   # the scan beside the auction: the same values
    assert bool((emd_1 > 0).all()) and bool(torch.isfinite(emd_1).all())
    res = meter.result()
    assert res['n_batches'] == 2 and res['class_n'] == [2] * B + [0] * (13 - B)
    assert res['class_emd'][0] == (float(emd_1[0]) + float(emd_1[0])) / 2


def test_update_makes_no_host_synchronisation():
    from vpn_amd import EvaluationMeter
    B, n = 8, 2048
    p, q = _clustered(B, n, 6)
    meter = EvaluationMeter(NAMES13, DEV, emd=True)
    cd_only = EvaluationMeter(NAMES13, DEV, emd=False)
    on_device = torch.arange(B, device=DEV)
    on_host = torch.arange(B)                                               # int64, as the DataLoader yields them
    meter.update(p, q, on_device)                                            # warm-up: code objects, the auction's LDS limit
    cd_only.update(p, q, on_host)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        a = meter.update(p, q, on_device)
        b = meter.update(p, q, on_host)
        c = meter.update(p, q, list(range(B)))
        d = cd_only.update(p, q, on_host)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], c[1]) and torch.equal(a[0], d[0]) and d[1] is None
    assert meter.result()['n_batches'] == 4 and cd_only.result()['n_batches'] == 2


def test_update_replays_from_a_graph():
    from vpn_amd import EvaluationMeter
    B, n = 8, 2048
    batches = [_clustered(B, n, 70 + k) + (torch.tensor([(3 * k + b) % 13 for b in range(B)], dtype=torch.int32),)
               for k in range(3)]
    eager = EvaluationMeter(NAMES13, DEV, emd=True)
    for p, q, idx in batches:
        eager.update(p, q, idx.to(DEV))
    want = eager.result()
    meter = EvaluationMeter(NAMES13, DEV, emd=True)
    sp, sq, sidx = batches[0][0].clone(), batches[0][1].clone(), batches[0][2].to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        meter.update(sp, sq, sidx)                                           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    meter.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cd_b, emd_b = meter.update(sp, sq, sidx)
    assert meter.result()['n_batches'] == 0                                  # capturing ran nothing
    for p, q, idx in batches:
        sp.copy_(p)
        sq.copy_(q)
        sidx.copy_(idx)
        graph.replay()
    torch.cuda.synchronize()
    got = meter.result()
    assert got == want                                                       # Python floats and ints: bit-equal
    assert got['n_batches'] == 3 and sum(got['class_n']) == 3 * B


def test_edge_cases():
    from vpn_amd import ChamferDistanceLoss, EvaluationMeter
    C = 4
    meter = EvaluationMeter(NAMES13[:C], DEV, emd=False)
    p, q = _clouds(6, 128, 96, 11)
    idx = [-1, C, 0, 1, 1, 3]
    cd_b, _ = meter.update(p, q, idx)
    cd = cd_b.cpu()
    tot, want, class_n, nb, invalid = _host_bookkeeping([(cd, None, idx)], C, False)
    sums, counts = _raw(meter)
    assert invalid == 2 and counts.tolist() == [1, 2, 1, 2, 0, 1]
    assert sums[3:3 + C].tolist() == want['cd'] and want['cd'][2] == 0.0     # out-of-range samples touch no class sum ...
    exact = sum(float(v) for v in cd) / 6                                    # ... and are part of the total
    assert abs(float(sums[0]) - exact) <= 1e-15
    assert torch.equal(cd_b, ChamferDistanceLoss()(p, q, each_batch=True))
    res = meter.result()
    assert res['n_invalid'] == 2 and res['class_cd'][2] is None and res['class_n'] == [1, 2, 0, 1]
    # a short last batch weighs like a full one in the total
    p3, q3 = _clouds(3, 128, 96, 12)
    cd3, _ = meter.update(p3, q3, torch.tensor([2, 2, 0]))
    res = meter.result()
    assert res['n_batches'] == 2 and res['class_n'] == [2, 2, 2, 1] and res['n_invalid'] == 2
    exact2 = (exact + sum(float(v) for v in cd3.cpu()) / 3) / 2
    assert abs(res['cd'] - exact2) <= 1e-15
    meter.reset()
    sums, counts = _raw(meter)
    assert not bool(sums.any()) and not bool(counts.any())
    res = meter.result()
    assert res['n_batches'] == 0 and res['cd'] is None and res['class_n'] == [0] * C
    # the EMD metric needs equal clouds: refused before anything is launched or added
    both = EvaluationMeter(NAMES13[:C], DEV, emd=True)
    with pytest.raises(ValueError, match='as many predicted'):
        both.update(p, q, idx)
    assert both.result()['n_batches'] == 0
    with pytest.raises(ValueError):
        meter.update(p, q, [0, 1])                                           # two indices for a batch of six


def test_large_batch_and_many_classes():
    """More samples than the finishing workgroup stages at a time (1024) and more classes than it has lanes (256)."""
    from vpn_amd import EvaluationMeter
    B, C = 1100, 300
    names = ['c%d' % i for i in range(C)]
    p, q = _clouds(B, 8, 8, 13)
    g = torch.Generator().manual_seed(14)
    idx = torch.randint(0, C, (B,), generator=g)
    idx[1050] = 299
    idx[7] = C + 5
    meter = EvaluationMeter(names, DEV, emd=False)
    cd_b, _ = meter.update(p, q, idx)
    cd_b2, _ = meter.update(p, q, idx)
    cd = cd_b.cpu()
    tot, want, class_n, nb, invalid = _host_bookkeeping([(cd, None, idx), (cd, None, idx)], C, False)
    sums, counts = _raw(meter)
    assert torch.equal(cd_b, cd_b2)
    assert counts.tolist() == [2, 2] + class_n
    assert sums[3:3 + C].tolist() == want['cd']
    assert abs(float(sums[0]) - 2 * float(cd.double().mean())) <= 1e-12


@pytest.mark.parametrize('flags', [[], ['--gcn']])
def test_eval_step_example_prints_a_table(flags):
    import os
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'eval_step.py'), '--batches', '4', '--epoch', '3'] + flags,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert 'Epoch 3' in r.stdout
    key = 'cd loss = ' if flags else 'avg cd loss = '
    rows = [l for l in lines if key in l and not l.startswith('total')]
    total = [l for l in lines if l.startswith('total') and key in l]
    assert len(rows) == 13 and len(total) == 1, r.stdout            # 8 + 8 + 8 + 5 samples cycling over 13 classes
    for l in rows + total:
        v = float(l.split(key)[1].split(',')[0])
        assert v == v and 0.0 < v < float('inf'), l
    assert 'n_invalid' not in r.stdout
