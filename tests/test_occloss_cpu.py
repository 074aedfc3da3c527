"""CPU checks of the occupancy loss (ops.primitive_occupancy_loss, ops.primitive_soft_occupancy, OccupancyLoss;
csrc/occloss.hip): the analytic gradient of tests/occloss_ref.py against torch float64 autograd of the same
expression, what fp32 costs (`own`), the tie rule, skipped queries, a descent in float64, the argument contract of the Python
layer and of the C entries, and the kernels' resources."""
import ctypes
import os

import numpy as np
import pytest
import torch

import occloss_ref as LR
import occupancy_ref as OR
from kernel_resources import kernel_resources

CASES = {'k3': dict(B=2, kinds=(1, 0, 0), Q=257, seed=11), 'k16': dict(B=2, kinds=(1, 0) * 8, Q=257, seed=12)}
TAUS = (0.02, 0.05, 0.1)
GRADS = ((1.0, 0.0), (0.0, 1.0), (0.3, 2.0))


def _autograd(params, kinds, queries, labels, tau, g):
    """(out [2], dparams) of the loss composed from torch float64 ops, differentiated by autograd."""
    p = torch.from_numpy(np.asarray(params)).double().requires_grad_(True)
    m = OR.prim_m(p, kinds, torch.from_numpy(np.asarray(queries)), torch.float64)          # [B,Q,K]
    z = -(m - 1) / tau
    l = torch.logsumexp(z, -1)
    y = torch.from_numpy(LR.labels_float(labels)).double()
    bce = (l.clamp(min=0) + torch.log1p(torch.exp(-l.abs()))) - y * l          # torch's softplus is linear above 20: e^-20 off
    ov = torch.relu(torch.sigmoid(z).sum(-1) - 1) ** 2
    out = torch.stack([bce.mean(), ov.mean()])
    (out * torch.tensor(g, dtype=torch.float64)).sum().backward()
    return out.detach().numpy(), p.grad.numpy()


@pytest.mark.parametrize('tau', TAUS)
@pytest.mark.parametrize('name', sorted(CASES))
def test_analytic_gradient_equals_float64_autograd_and_own_error_is_small(name, tau):
    c = CASES[name]
    params, queries, labels = LR.case(c['B'], c['kinds'], c['Q'], c['seed'])
    frac = float(labels.mean())
    assert 0.0 < frac < 1.0, frac                                              # both branches of the cross-entropy
    f = LR.forward(params, c['kinds'], queries, labels, tau)
    assert f['n_skipped'] == 0 and (f['s'] > 1).any() and (f['s'] < 1).any()    # and both of the overlap term
    for g in GRADS:
        want_out, want_grad = _autograd(params, c['kinds'], queries, labels, tau, g)
        got = LR.backward(params, c['kinds'], queries, labels, tau, g, fwd=f)
        e_out = float((np.abs(f['out'] - want_out) / (1 + np.abs(want_out))).max())
        e_grad = float(np.abs(got - want_grad).max() / np.abs(want_grad).max())
        print('%s tau %.2f g %s: restatement against autograd, losses %.2e  gradient %.2e (losses %s)' % (name, tau, g, e_out, e_grad, want_out))
        assert e_out <= 1e-12 and e_grad <= 1e-10, (g, e_out, e_grad)
    own = LR.errors(params, c['kinds'], queries, labels, tau, (0.3, 2.0))
    print('%s tau %.2f: labels %.3f inside; own (fp32 against float64) losses %.2e  per query %.2e  gradient %.2e'
          % (name, tau, frac, *own))
    assert own[0] <= 1e-5 and own[2] <= 1e-4                                    # fp32 itself stays far inside the 1e-4 bar


def test_cuboid_ties_take_the_lowest_axis_and_sign_of_zero_is_zero():
    kinds = (LR.CUBOID,)
    params = np.array([[[0.2, 0.2, 0.2, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]]], np.float32)      # q3 = 0: the identity
    labels = np.zeros((1, 1), np.uint8)
    tie = LR.backward(params, kinds, np.array([[0.1, 0.1, 0.05]], np.float32), labels, 0.05)[0, 0]
    assert tie[0] != 0 and tie[1] == 0 and tie[2] == 0                          # x~ = (0.5, 0.5, 0.25): axis 0 of the two
    assert tie[7] != 0 and tie[8] == 0 and tie[9] == 0
    tie = LR.backward(params, kinds, np.array([[0.05, -0.1, 0.1]], np.float32), labels, 0.05)[0, 0]
    assert tie[0] == 0 and tie[1] != 0 and tie[2] == 0 and tie[8] < 0           # y before z, and its sign: x~_y < 0, so moving t up moves the point out
    centre = LR.backward(params, kinds, np.zeros((1, 3), np.float32), labels, 0.05, (1.0, 1.0))
    assert not centre.any()                                                     # x~ = 0: sign(0) = 0, no gradient at all


def test_skipped_queries_add_exactly_zero_and_are_counted():
    c = CASES['k3']
    params, queries, labels = LR.case(3, c['kinds'], 70, 3, shared=False)
    labels = labels.astype(np.float32)
    queries[0, 5, 1] = np.nan
    queries[1, 7, 0] = np.inf
    labels[0, 9] = np.nan
    params[2, :, 0] = 0.0                                                       # every m of sample 2 is inf or a NaN
    f = LR.forward(params, c['kinds'], queries, labels, 0.05)
    want = np.zeros((3, 70), bool)
    want[0, 5] = want[1, 7] = want[0, 9] = True
    want[2] = True
    assert np.array_equal(f['skipped'], want) and f['n_skipped'] == 73
    assert not f['bce'][want].any() and not f['ov'][want].any() and np.isfinite(f['out']).all()
    g = LR.backward(params, c['kinds'], queries, labels, 0.05, (0.3, 2.0), fwd=f)
    assert np.isfinite(g).all() and not g[2].any() and g[0].any() and g[1].any()
    # the same numbers from the queries that are left, sample by sample, with the divisor kept at B Q
    total, grads = np.zeros(2), np.zeros_like(g)
    for b in range(2):
        keep = ~want[b]
        fb = LR.forward(params[b:b + 1], c['kinds'], queries[b:b + 1, keep], labels[b:b + 1, keep], 0.05)
        scale = keep.sum() / (3 * 70)
        total += fb['out'] * scale
        grads[b] = LR.backward(params[b:b + 1], c['kinds'], queries[b:b + 1, keep], labels[b:b + 1, keep], 0.05, (0.3, 2.0), fwd=fb)[0] * scale
    assert np.abs(total - f['out']).max() <= 1e-14 and np.abs(grads - g).max() <= 1e-12 * np.abs(g).max()


def test_one_primitive_has_its_own_logit():
    params, queries, labels = LR.case(2, (0,), 65, 4)
    for kinds in ((0,), (1,)):
        for dt in (np.float64, np.float32):
            f = LR.forward(params, kinds, queries, labels, 0.25, dt)
            assert np.array_equal(f['lse'], f['z'][..., 0]) and np.array_equal(f['s'], LR.sigmoid(f['z'][..., 0]))


def test_descent_in_float64_lowers_the_loss_and_raises_the_iou():
    start, kinds, queries, labels = LR.descent_case()
    assert 0.0 < labels.mean() < 1.0
    p = start.astype(np.float64)
    first = LR.forward(p, kinds, queries, labels, 0.05)['out'][0]
    iou0 = LR.iou(p, kinds, queries, labels)
    for _ in range(200):
        p = p - 0.02 * LR.backward(p, kinds, queries, labels, 0.05)
    last, iou1 = LR.forward(p, kinds, queries, labels, 0.05)['out'][0], LR.iou(p, kinds, queries, labels)
    print('descent: loss %.4f -> %.4f, IoU %.3f -> %.3f' % (first, last, iou0, iou1))
    assert last < first and iou1 > iou0


# ---- the Python layer

def test_ops_contract_is_checked_before_any_launch():
    import vpn_amd
    from vpn_amd import OccupancyLoss, ops
    prm, kinds, q, lab = torch.zeros(2, 3, 10), [1, 0, 0], torch.zeros(5, 3), torch.zeros(2, 5, dtype=torch.uint8)
    for fn, args in ((ops.primitive_occupancy_loss, (lab,)), (ops.primitive_soft_occupancy, ())):
        name = fn.__name__
        with pytest.raises(ValueError, match=name + r': params must be float32 \[B,K,10\]'):
            fn(prm[0], kinds, q, *args, 0.05)
        with pytest.raises(ValueError, match=name + ': 2 kinds for 3 primitives'):
            fn(prm, kinds[:2], q, *args, 0.05)
        with pytest.raises(ValueError, match=name + r': queries must be float32 \[Q,3\] or \[B,Q,3\]'):
            fn(prm, kinds, q.double(), *args, 0.05)
        with pytest.raises(ValueError, match='unknown primitive kind'):
            fn(prm, [1, 0, 2], q, *args, 0.05)
        for tau in (0.0, -1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError, match='tau must be finite and > 0'):
                fn(prm, kinds, q, *args, tau)
        with pytest.raises(ValueError, match='GPU only'):                         # host tensors have no path
            fn(prm, kinds, q, *args, 0.05)
    for bad in (lab[:, :4], lab[0], lab.int(), lab.double(), None):
        with pytest.raises(ValueError, match=r'labels must be uint8 or float32 \[2,5\]'):
            ops.primitive_occupancy_loss(prm, kinds, q, bad)
    with pytest.raises(ValueError, match='GPU only'):
        OccupancyLoss(1.0, 0.1)(prm, kinds, q, lab)
    loss = OccupancyLoss()
    assert loss.weights == (1.0, 0.0) and loss.tau == 0.05 and loss.last is None and loss.last_skipped is None
    for name in ('OccupancyLossFunction', 'primitive_occupancy_loss', 'primitive_soft_occupancy', 'occloss_plan'):
        assert getattr(vpn_amd, name) is getattr(ops, name), name
    assert vpn_amd.OccupancyLoss is OccupancyLoss


# ---- the C entries and the kernels

def test_entries_were_added_without_an_abi_change_and_refuse_bad_arguments():
    import vpn_amd._lib as lib
    from vpn_amd import ops
    L = lib.lib()
    assert L.vpn_abi_version() == lib.ABI_VERSION == 9
    for name in ('vpn_occloss_plan', 'vpn_occloss_workspace', 'vpn_occloss_fwd', 'vpn_occloss_bwd'):
        assert name in lib.SIGNATURES and hasattr(L, name), name
    big, kmax = lib.CONSTANTS['VPN_OCCUPANCY_MAX_ITEMS'] + 1, lib.CONSTANTS['VPN_MAX_PRIMS']
    tile, qpl, groups = lib.CONSTANTS['VPN_OCCUPANCY_TILE'], lib.CONSTANTS['VPN_OCCLOSS_MAX_QPL'], lib.CONSTANTS['VPN_OCCLOSS_MIN_GROUPS']
    assert (tile, qpl, groups) == (256, 8, 256)
    # the plan: the largest slice of 256 * (8, 4, 2, 1) queries that still gives 256 workgroups, a function of (B, Q) alone
    assert ops.occloss_plan(2, 257) == (2, 256) and ops.occloss_plan(1, 1) == (1, 256)
    assert ops.occloss_plan(64, 32768) == (16, 2048) and ops.occloss_plan(64, 8193) == (5, 2048)
    assert ops.occloss_plan(8, 32768) == (32, 1024) and ops.occloss_plan(128, 513) == (2, 512) and ops.occloss_plan(128, 512) == (2, 256)
    sq = ctypes.c_int(0)
    assert L.vpn_occloss_plan(3, 700, None) == 3
    for bad in ((0, 1), (1, 0), (-1, 5)):
        assert L.vpn_occloss_plan(*bad, ctypes.byref(sq)) == -1, bad
    assert L.vpn_occloss_plan(65536, 1, ctypes.byref(sq)) == -2 and L.vpn_occloss_plan(1, big, ctypes.byref(sq)) == -2 and sq.value == 0
    # the workspace: four floats a forward workgroup, or 4 K 12 floats a slice of the backward, whichever is more
    ws = L.vpn_occloss_workspace
    assert ws(2, 3, 257) == 2 * 2 * 4 * 3 * 12 * 4 and ws(1, 1, 1) == 4 * 12 * 4 and ws(64, 16, 32768) == 64 * 16 * 4 * 16 * 12 * 4
    assert ws(0, 1, 1) == 0 and ws(1, 0, 1) == 0 and ws(1, 1, 0) == 0 and ws(65536, 1, 1) == 0 and ws(1, kmax + 1, 1) == 0 and ws(1, 1, big) == 0
    # sizes and limits are looked at before any pointer is followed: host buffers stand in for device memory
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd16 = ctypes.c_void_p(p.value + 8)
    assert p.value % 16 == 0

    def fwd(params=p, kinds=p, queries=p, labels=p, B=1, K=2, Q=4, tau=0.05, work=p, nbytes=32768, lse=p, s=p, out=p, skipped=p):
        return L.vpn_occloss_fwd(params, kinds, queries, 1, labels, 1, B, K, Q, tau, work, nbytes, lse, s, out, skipped, None)

    def bwd(grad=p, params=p, kinds=p, queries=p, labels=p, lse=p, s=p, B=1, K=2, Q=4, tau=0.05, work=p, nbytes=32768, dparams=p):
        return L.vpn_occloss_bwd(grad, params, kinds, queries, 1, labels, 0, lse, s, B, K, Q, tau, work, nbytes, dparams, None)

    sizes = (dict(B=0), dict(K=0), dict(Q=0), dict(Q=-2))
    taus = (dict(tau=0.0), dict(tau=-0.05), dict(tau=float('nan')), dict(tau=float('inf')))
    for bad in (dict(params=None), dict(kinds=None), dict(queries=None), dict(labels=None), dict(work=None), dict(lse=None),
                dict(s=None), dict(lse=None, s=None, out=None), dict(out=None), dict(out=None, labels=None, work=None),
                dict(nbytes=ws(1, 2, 4) // 100), dict(nbytes=15), dict(work=odd16)) + sizes + taus:
        assert fwd(**bad) == -1, bad
    for bad in (dict(grad=None), dict(params=None), dict(kinds=None), dict(queries=None), dict(labels=None), dict(lse=None),
                dict(s=None), dict(work=None), dict(dparams=None), dict(nbytes=ws(1, 2, 4) - 1), dict(work=odd16)) + sizes + taus:
        assert bwd(**bad) == -1, bad
    for too in (dict(B=65536), dict(Q=big), dict(K=kmax + 1)):
        assert fwd(**too) == -2 and bwd(**too) == -2, too
    assert not any(buf)                                                       # nothing was written


def test_kernels_use_no_scratch_and_no_atomics():
    from kernel_resources import load_build
    b = load_build()
    assert 'occloss.hip' in b.SOURCES and b.PER_FILE['occloss.hip'] == ['-ffp-contract=off']
    rows = kernel_resources('occloss.hip')
    kernels = ('occl_fwd_kernel', 'occl_fwd_finish_kernel', 'occl_bwd_kernel', 'occl_bwd_finish_kernel')
    for k in kernels:
        hits = [v for name, v in rows.items() if k in name]
        assert len(hits) == 1, (k, list(rows))
        assert hits[0]['ScratchSize'] == 0, (k, hits[0])
    assert len(rows) == len(kernels), list(rows)
    src = open(os.path.join(b.CSRC, 'occloss.hip')).read()
    assert 'atomic' not in src.split('#include', 1)[1]
