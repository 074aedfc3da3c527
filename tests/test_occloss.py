"""The occupancy loss on the GPU (vpn_amd.primitive_occupancy_loss, primitive_soft_occupancy, ops.OccupancyLossFunction,
OccupancyLoss, csrc/occloss.hip) against the float64 statement of tests/occloss_ref.py: parity of the losses,
of the logit and the overlap sum per query and of the gradient at the shapes where the kernels take another path, the field's
bits for one primitive, skipped queries, the module, reproducibility, no host synchronisation, graph capture, a descent, the
example.

The bar is the project's max(1e-4, 4 x own), own being the error of the restatement's fp32 mode against float64 on the same
input (tests/test_occloss_cpu.py prints it: about 6e-8 on the losses, 1e-5 per query, 2e-6 on the gradient)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import occloss_ref as LR
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GRADS = ((1.0, 0.0), (0.0, 1.0), (0.3, 2.0))


def _slice(B):
    """The backward's slice at a small Q, read from the library."""
    import vpn_amd
    return vpn_amd.occloss_plan(B, 1)[1]


def _shapes():
    s1 = _slice(2)
    return {
        'q1': dict(B=2, kinds=(1, 0, 0), Q=1, seed=21, tau=0.05),
        'q257': dict(B=3, kinds=(1, 0, 0), Q=257, seed=22, tau=0.05),
        'k300': dict(B=1, kinds=(1, 0, 0) * 100, Q=65, seed=23, tau=0.1),                 # two stagings of 256 records
        'k1': dict(B=2, kinds=(0,), Q=70, seed=24, tau=0.02),
        'slice+1': dict(B=2, kinds=(0, 1), Q=s1 + 1, seed=25, tau=0.05),
        '2slices+1': dict(B=2, kinds=(1, 0, 0, 1, 0), Q=2 * s1 + 1, seed=26, tau=0.05),
        'qpl8': dict(B=64, kinds=(0, 1), Q=8193, seed=27, tau=0.05),                      # eight queries a lane, 4 slices + 1
    }


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The case and its float64 reference, computed once and shared: inputs, forward, the gradient for every upstream gradient,
    and own."""
    c = _shapes()[name]
    params, queries, labels = LR.case(c['B'], c['kinds'], c['Q'], c['seed'])
    f = LR.forward(params, c['kinds'], queries, labels, c['tau'])
    grads = {g: LR.backward(params, c['kinds'], queries, labels, c['tau'], g, fwd=f) for g in GRADS}
    own = LR.errors(params, c['kinds'], queries, labels, c['tau'], GRADS[2])
    return dict(c, params=params, queries=queries, labels=labels, fwd=f, grads=grads, own=own)


def _bar(own):
    return max(1e-4, 4 * own)


def _run(params, kinds, queries, labels, tau, g):
    """(out, n_skipped, dparams) through the op."""
    import vpn_amd
    p = params.clone().requires_grad_(True)
    out, skipped = vpn_amd.primitive_occupancy_loss(p, kinds, queries, labels, tau, return_skipped=True)
    (grad,) = torch.autograd.grad((out * torch.tensor(g, device=DEV)).sum(), [p])
    return out.detach(), skipped, grad


@pytest.mark.parametrize('name', ['q1', 'q257', 'k300', 'k1', 'slice+1', '2slices+1', 'qpl8'])
def test_parity_with_the_float64_restatement(name):
    import vpn_amd
    r = _reference(name)
    B, Q, kinds, tau, f = r['B'], r['Q'], list(r['kinds']), r['tau'], r['fwd']
    slices, per = vpn_amd.occloss_plan(B, Q)
    assert slices == -(-Q // per)
    if name in ('slice+1', '2slices+1'):
        assert Q % per == 1 and slices == Q // per + 1
    if name == 'qpl8':
        assert per == 8 * 256 and slices == 5
    params, labels = torch.from_numpy(r['params']).to(DEV), torch.from_numpy(r['labels']).to(DEV)
    shared = torch.from_numpy(r['queries']).to(DEV)
    logit, overlap = vpn_amd.primitive_soft_occupancy(params, kinds, shared, tau)
    want_l, want_s = f['lse'], f['s']
    fin = np.isfinite(want_l)
    assert np.array_equal(np.isfinite(logit.cpu().numpy()), fin)
    e_l = float((np.abs(logit.cpu().numpy().astype(np.float64) - want_l)[fin] / (1 + np.abs(want_l[fin]))).max())
    e_s = float((np.abs(overlap.cpu().numpy().astype(np.float64) - want_s) / (1 + np.abs(want_s))).max())
    bar_o, bar_q, bar_g = (_bar(o) for o in r['own'])
    print('%s: own %.2e %.2e %.2e | logit %.2e  overlap sum %.2e (bar %.1e)' % ((name,) + r['own'] + (e_l, e_s, bar_q)))
    assert e_l <= bar_q and e_s <= bar_q
    first = None
    for g in GRADS:
        out, skipped, grad = _run(params, kinds, shared, labels, tau, g)
        assert int(skipped) == f['n_skipped'] == 0
        e_o = float((np.abs(out.cpu().numpy().astype(np.float64) - f['out']) / (1 + np.abs(f['out']))).max())
        want = r['grads'][g]
        e_g = float(np.abs(grad.cpu().numpy().astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-300))   # no overlap anywhere: exactly 0
        print('%s g %s: losses %.2e (bar %.1e)  dparams %.2e (bar %.1e)' % (name, g, e_o, bar_o, e_g, bar_g))
        assert e_o <= bar_o and e_g <= bar_g
        if first is None:
            first = (out, grad)
    if name == 'qpl8':
        return
    # fp32 labels that hold the same values, and the queries repeated per sample: the same bits
    out_f, _, grad_f = _run(params, kinds, shared, labels.float(), tau, GRADS[0])
    out_r, _, grad_r = _run(params, kinds, shared[None].expand(B, -1, -1).contiguous(), labels, tau, GRADS[0])
    for got in ((out_f, grad_f), (out_r, grad_r)):
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])


def test_one_primitive_gives_the_field_bit_for_bit():
    import vpn_amd
    for kinds in ([0], [1]):
        params, queries, _ = LR.case(3, kinds, 300, 31)
        params, queries = torch.from_numpy(params).to(DEV), torch.from_numpy(queries).to(DEV)
        logit, overlap = vpn_amd.primitive_soft_occupancy(params, kinds, queries, 0.25)
        field = vpn_amd.primitive_field(params, kinds, queries)
        assert torch.equal(logit, -4.0 * field)
        assert torch.equal(logit <= 0, field >= 0)


def test_skipped_queries_are_counted_and_nothing_is_a_nan():
    kinds = [1, 0, 0]
    params, queries, labels = LR.case(3, kinds, 300, 41, shared=False)
    labels = labels.astype(np.float32)
    queries[0, 5, 1] = np.nan
    queries[1, 299, 0] = np.inf
    labels[0, 9] = np.nan
    params[1, 2, 0] = 0.0                                                       # one primitive without an extent
    params[1, 1, 4] = np.nan                                                    # and one without a rotation
    params[2, :, 1] = 0.0                                                       # a sample none of whose primitives is left
    f = LR.forward(params, kinds, queries, labels, 0.05)
    assert f['n_skipped'] == 3 + 300
    want = LR.backward(params, kinds, queries, labels, 0.05, GRADS[2], fwd=f)
    own = LR.errors(np.where(np.isfinite(params), params, 0.5).astype(np.float32), kinds, np.nan_to_num(queries, nan=0.0, posinf=0.0),
                    np.nan_to_num(labels), 0.05, GRADS[2])
    out, skipped, grad = _run(torch.from_numpy(params).to(DEV), kinds, torch.from_numpy(queries).to(DEV), torch.from_numpy(labels).to(DEV),
                              0.05, GRADS[2])
    assert int(skipped) == f['n_skipped']
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all())
    got = grad.cpu().numpy().astype(np.float64)
    assert not got[1, 1].any() and not got[1, 2].any() and not got[2].any() and got[0].any() and got[1, 0].any()
    e_o = float((np.abs(out.cpu().numpy() - f['out']) / (1 + np.abs(f['out']))).max())
    e_g = float(np.abs(got - want).max() / np.abs(want).max())
    print('skipped: losses %.2e  dparams %.2e  own %.2e %.2e' % (e_o, e_g, own[0], own[2]))
    assert e_o <= _bar(own[0]) and e_g <= _bar(own[2])


def test_module_equals_its_parts_and_a_zero_weight_stays_finite():
    import vpn_amd
    r = _reference('q257')
    kinds = list(r['kinds'])
    params, labels = torch.from_numpy(r['params']).to(DEV), torch.from_numpy(r['labels']).to(DEV)
    queries = torch.from_numpy(r['queries']).to(DEV)
    for w in ((1.0, 0.25), (1.0, 0.0), (0.0, 1.0)):
        module = vpn_amd.OccupancyLoss(*w, tau=r['tau'])
        p = params.clone().requires_grad_(True)
        loss = module(p, kinds, queries, labels)
        loss.backward()
        out, skipped, grad = _run(params, kinds, queries, labels, r['tau'], w)
        assert torch.equal(module.last, out) and torch.equal(module.last_skipped, skipped) and not module.last.requires_grad
        assert torch.equal(loss.detach(), (out * torch.tensor(w, device=DEV)).sum())
        assert torch.equal(p.grad, grad)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    # without a gradient nothing is saved and the result is the same
    with_grad = _run(params, kinds, queries, labels, r['tau'], GRADS[0])[0]
    plain = vpn_amd.primitive_occupancy_loss(params, kinds, queries, labels, r['tau'])
    assert torch.equal(plain, with_grad) and not plain.requires_grad


def test_bit_equal_runs_no_host_synchronisation_and_graph_replay():
    import vpn_amd
    r = _reference('2slices+1')
    kinds = vpn_amd.kinds_tensor(list(r['kinds']), DEV)
    labels, queries = torch.from_numpy(r['labels']).to(DEV), torch.from_numpy(r['queries']).to(DEV)
    sp = torch.from_numpy(r['params']).to(DEV).requires_grad_(True)          # the static input of the capture
    up = torch.tensor(GRADS[2], device=DEV)

    def step():
        out, skipped = vpn_amd.primitive_occupancy_loss(sp, kinds, queries, labels, r['tau'], return_skipped=True)
        return [out.detach(), skipped] + list(torch.autograd.grad((out * up).sum(), [sp]))

    eager = [t.clone() for t in step()]                                   # warm-up: library handles, the kinds' host copy
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        strict = step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for a, b in zip(strict, eager):
        assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for k in range(3):                                                    # three replays equal three eager calls
        with torch.no_grad():
            sp.mul_(1.0 + 0.05 * k).add_(0.01 * k)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in captured]
        for a, b in zip(replayed, step()):
            assert torch.equal(a, b)
        assert float(replayed[2].abs().max()) > 0


def test_descent_through_the_op_lowers_the_loss_and_raises_the_iou():
    import vpn_amd
    start, kinds, queries, labels = LR.descent_case()
    q, lab = torch.from_numpy(queries).to(DEV), torch.from_numpy(labels).to(DEV)
    p = torch.from_numpy(start).to(DEV).requires_grad_(True)
    iou0, losses = LR.iou(start, kinds, queries, labels), []
    for _ in range(50):
        out = vpn_amd.primitive_occupancy_loss(p, list(kinds), q, lab, 0.05)
        (g,) = torch.autograd.grad(out[0], [p])
        losses.append(out[0].detach())
        with torch.no_grad():
            p -= 0.02 * g
    last = float(vpn_amd.primitive_occupancy_loss(p.detach(), list(kinds), q, lab, 0.05)[0])
    iou1 = LR.iou(p.detach().cpu().numpy(), kinds, queries, labels)
    print('descent through the op: loss %.4f -> %.4f, IoU %.3f -> %.3f' % (float(losses[0]), last, iou0, iou1))
    assert last < float(losses[0]) and iou1 > iou0


def test_train_step_example_runs_with_occupancy_loss():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'train_step.py'), '--steps', '2', '--occupancy-loss', '1,0.1'],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith('step ')]
    assert len(lines) == 2 and all(' occ ' in l and '(occupancy ' in l and ', overlap ' in l for l in lines), r.stdout
    for l in lines:
        occ = float(l.split('(occupancy ')[1].split(',')[0])
        ov = float(l.split(', overlap ')[1].split(')')[0])
        assert occ == occ and 0 < occ < float('inf') and ov == ov and 0 <= ov < float('inf'), l
