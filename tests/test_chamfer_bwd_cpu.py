"""CPU tests of tests/chamfer_bwd_ref.py: the float64 statement of the Chamfer backward against the oracle's autograd, the
element-wise bar against fp32 evaluations of the closed form in shuffled orders (they must stay within HALF the bar, or the
bar is wrong) and against three injected faults (each must break it, or the bar sees nothing), and every property the case
builders claim, the launch path included (limits read from include/vpn_hip.h and the kernels' sources)."""
import os
import re

import numpy as np
import pytest
import torch

import chamfer_bwd_ref as C
from conftest import ROOT
from oracle import vpn_oracle as O

CASES = C.cases()
NO_NAN = [n for n, c in CASES.items() if not c['meta']['nan']]


def _neighbours(case):
    return C.neighbours(case, O.chamfer_nn_ieee)


def _source_constants():
    """CB_MAX_POINTS, CB_LDS_DEFAULT (csrc/chamfer.hip), SCB_BLOCK (csrc/sampler.hip), VPN_FUSED_BWD_MAX_GT (the header), read
    with the binding's own header parser, not copied."""
    import vpn_amd._lib as lib
    csrc = os.path.join(ROOT, 'volumetric-primitives-net_amd', 'csrc')
    out = {'VPN_FUSED_BWD_MAX_GT': lib.CONSTANTS['VPN_FUSED_BWD_MAX_GT']}
    for name, fname, pattern in (('CB_MAX_POINTS', 'chamfer.hip', r'constexpr\s+int\s+CB_MAX_POINTS\s*=\s*(\d+)\s*;'),
                                 ('CB_LDS_DEFAULT', 'chamfer.hip', r'constexpr\s+size_t\s+CB_LDS_DEFAULT\s*=\s*(\d+)\s*;'),
                                 ('SCB_BLOCK', 'sampler.hip', r'#\s*define\s+SCB_BLOCK\s+(\d+)')):
        with open(os.path.join(csrc, fname)) as f:
            found = re.findall(pattern, lib._header_code(f.read()))
        assert len(found) == 1, (name, found)
        out[name] = int(found[0])
    return out


# ----------------------------------------------------------------------------- the statement is the oracle's gradient
@pytest.mark.parametrize('name', [n for n in NO_NAN if n.startswith(('ragged', 'hub')) and 'translated' not in n])
def test_statement_equals_float64_autograd(name):
    """The closed form with the float64 oracle's own arg-minima (torch.min: lowest index on a tie) equals the float64
    autograd of O.chamfer_loss(each_batch=True), both gradients, to 1e-12 of the largest element."""
    case = CASES[name]
    p1, p2 = (torch.from_numpy(case[k]).double() for k in ('p1', 'p2'))
    _, i1, _, i2 = O.chamfer_nn(p1, p2)
    a, b = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    (O.chamfer_loss(a, b, each_batch=True, w1=case['w1'], w2=case['w2']) * torch.from_numpy(case['gl']).double()).sum().backward()
    (g1, _, _), (g2, _, _) = C.both(case, i1.numpy(), i2.numpy())
    for got, ref in ((g1, a.grad.numpy()), (g2, b.grad.numpy())):
        assert np.isfinite(ref).all()
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (name, np.abs(got - ref).max(), np.abs(ref).max())


def test_statement_nan_rows_and_missing_neighbours():
    """A coincident pair: NaN in the query's row and the target's row, nowhere else.  An index outside the other cloud:
    that row NaN, nothing scattered from it, every other row as without the point."""
    case = CASES['coincident']
    i1, i2 = _neighbours(case)
    (g1, _, _), (g2, _, _) = C.both(case, i1, i2)
    for g, rows in ((g1, case['meta']['nan_p1']), (g2, case['meta']['nan_p2'])):
        nan = np.isnan(g).any(2)
        assert np.isnan(g[nan]).all() and all(sorted(np.nonzero(r)[0].tolist()) == rows for r in nan), nan.nonzero()
    case = CASES['ragged_63x65']
    i1, i2 = _neighbours(case)
    j1 = i1.copy()
    j1[0, 5] = 0x7fffffff
    j1[1, 6] = -1
    (g1, _, _), (g2, n2, _) = C.both(case, i1, i2)
    (h1, _, _), (h2, m2, _) = C.both(case, j1, i2)
    assert np.isnan(h1[0, 5]).all() and np.isnan(h1[1, 6]).all() and np.isnan(h1).sum() == 6
    h1[0, 5], h1[1, 6] = g1[0, 5], g1[1, 6]
    assert np.array_equal(h1, g1)
    assert np.isfinite(h2).all() and m2.sum() == n2.sum() - 2 and m2[0, i1[0, 5]] == n2[0, i1[0, 5]] - 1


# ----------------------------------------------------------------------------- the bar
def _held(got, ref, n, S, fraction=1.0):
    """Largest |got - ref| / bar over the elements that are not NaN in the reference (0/0 where bar and error are both 0 counts
    as held), after checking that got is NaN in exactly the reference's NaN rows."""
    nan = np.isnan(ref).any(2)
    assert np.array_equal(np.isnan(got).any(2), nan)
    err, lim = np.abs(got.astype(np.float64) - ref)[~nan], C.bar(n, S)[~nan] * fraction
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where((err == 0) & (lim == 0), 0.0, err / lim)
    return float(ratio.max()) if ratio.size else 0.0


@pytest.mark.parametrize('name', list(CASES))
def test_fp32_evaluations_stay_within_half_the_bar(name):
    """The closed form in fp32 numpy, the forward's fp32 distance, each row's terms added in 8 seeded random orders: every
    element within HALF the bar, on every case.  A failure here faults the bar, not a kernel."""
    case = CASES[name]
    i1, i2 = _neighbours(case)
    (g1, n1, S1), (g2, n2, S2) = C.both(case, i1, i2)
    rng = np.random.RandomState(2024)
    worst = 0.0
    for _ in range(8):
        e1 = C.evaluate32(case['p1'], case['p2'], i1, i2, case['gl'], case['w1'], case['w2'], rng)
        e2 = C.evaluate32(case['p2'], case['p1'], i2, i1, case['gl'], case['w2'], case['w1'], rng)
        worst = max(worst, _held(e1, g1, n1, S1, 0.5), _held(e2, g2, n2, S2, 0.5))
    print('%s: worst |fp32 - float64| / (bar / 2) = %.3f' % (name, worst))
    assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize('fault', ['dropped_term', 'index_plus_one', 'stale_row'])
def test_injected_fault_breaks_the_bar(fault):
    """Each of three subtly wrong evaluations, on its own, exceeds the bar in at least one element (and the unharmed
    evaluation of the same case does not): one scatter term of the hub row missing; idx + 1 for one point (its old dist);
    one unreferenced row left at a stale value, here its neighbour row's."""
    case = CASES[{'dropped_term': 'hub1_700x64', 'index_plus_one': 'ragged_63x65', 'stale_row': 'unreferenced'}[fault]]
    i1, i2 = _neighbours(case)
    (g1, n1, S1), (g2, n2, S2) = C.both(case, i1, i2)
    args2 = (case['p2'], case['p1'], i2, i1, case['gl'], case['w2'], case['w1'])
    good = C.evaluate32(*args2)
    assert _held(good, g2, n2, S2) <= 0.5
    if fault == 'dropped_term':
        h = case['meta']['hub_rows'][0]
        f = np.float32
        e = 123                                                    # point e of p1 has the hub as its nearest neighbour
        assert i1[0, e] == h
        d = C.forward_dist32(case['p1'], case['p2'], i1)[0, e]
        bad = good.copy()
        bad[0, h] = bad[0, h] - ((case['gl'][0] * f(case['w1'])) / f(case['N'])) / d * (case['p2'][0, h] - case['p1'][0, e])
    elif fault == 'index_plus_one':
        j2 = i2.copy()
        j2[0, 7] = (j2[0, 7] + 1) % case['N']
        bad = C.evaluate32(case['p2'], case['p1'], j2, i1, case['gl'], case['w2'], case['w1'],
                           dist_a=C.forward_dist32(case['p2'], case['p1'], i2))
    else:
        r = case['meta']['unref_p2'][3]
        assert n2[0, r] == 0
        bad = good.copy()
        bad[0, r] = good[0, r - 1]
    assert _held(bad, g2, n2, S2) > 1.0, fault


# ----------------------------------------------------------------------------- what the builders claim
@pytest.mark.parametrize('name', list(CASES))
def test_case_meta_holds(name):
    case, meta = CASES[name], CASES[name]['meta']
    k = _source_constants()
    i1, i2 = _neighbours(case)
    (g1, n1, S1), (g2, n2, S2) = C.both(case, i1, i2)
    N, M = case['N'], case['M']
    assert meta['path'] == C.path_of(N, M, k['CB_MAX_POINTS'], k['CB_LDS_DEFAULT']), (name, meta['path'])
    assert not (N > k['CB_MAX_POINTS'] and M > k['CB_MAX_POINTS'])
    assert max(np.abs(case['p1']).max(), np.abs(case['p2']).max()) <= 2000.0
    assert (n1.sum(1) == M).all() and (n2.sum(1) == N).all()
    if not meta['nan']:
        d1 = np.linalg.norm(case['p1'].astype(np.float64) - np.take_along_axis(case['p2'].astype(np.float64), i1[..., None], 1), axis=2)
        d2 = np.linalg.norm(case['p2'].astype(np.float64) - np.take_along_axis(case['p1'].astype(np.float64), i2[..., None], 1), axis=2)
        assert min(d1.min(), d2.min()) >= 1e-6, (name, d1.min(), d2.min())
        assert np.isfinite(g1).all() and np.isfinite(g2).all()
    if 'hub_rows' in meta:
        rows = meta['hub_rows']
        assert (n2[:, rows].sum(1) == meta['hub_total']).all() and (n2[:, rows] > 0).all(), n2[:, rows]
        if len(rows) == 2:
            assert (n2[:, rows] >= meta['hub_total'] // 4).all(), n2[:, rows]
        assert (n2 == 0).sum() == n2.size - n2.shape[0] * len(rows)
    if 'unref_p2' in meta:
        assert len(meta['unref_p2']) > 0 and (n2[:, meta['unref_p2']] == 0).all()
    if 'cancel_row' in meta:
        r = meta['cancel_row']
        assert (n1[:, r] == 3).all()
        assert (np.abs(g1[:, r]).max(1) < 1e-2 * S1[:, r].max(1)).all(), (g1[:, r], S1[:, r])
    if 'close_p1' in meta:
        sel = d1[:, meta['close_p1']]
        assert (sel >= 1e-6).all() and (sel <= 1.1e-6).all() and (i1[:, meta['close_p1']] == np.array(meta['close_p2'])).all()
    if 'zero' in meta:
        assert (case['w1'], case['w2'])[meta['zero'] - 1] == 0.0
        own, other = ((g1, n1), (g2, n2)) if meta['zero'] == 1 else ((g2, n2), (g1, n1))
        assert (own[0][own[1] == 0] == 0).all() and (own[1] == 0).any()          # rows that hold the zero-weight term alone
    if name.startswith('ragged'):
        assert (case['gl'] == 0).any() and (case['gl'] < 0).any() and len(case['gl']) == 3
    assert any((n == 0).any() for n in (n1, n2)) or N == 1 or M == 1


def test_case_list_covers_the_issue():
    """Every shape and kind of case the tests were asked to hold, by name; each side of every size rule is there."""
    k = _source_constants()
    names = set(CASES)
    for N, M in C.RAGGED:
        assert 'ragged_%dx%d' % (N, M) in names
    edge = k['CB_LDS_DEFAULT'] // 12                                  # the most points whose gradient fits the default limit
    assert {(edge, 40), (edge + 1, 40), (40, edge + 1)} == set(C.LDS_RAISE)
    top = k['CB_MAX_POINTS']
    assert {(top, 33), (33, top)} == set(C.LDS_MAX) and {(top + 1, 33), (33, top + 1), (top + 1, 700)} == set(C.GLOBAL_MIN)
    assert {(700, 64), (top + 1, 33), (33, top + 1)} == set(C.HUBS)
    for extra in ('hub2_700x64', 'unreferenced', 'cancel', 'close', 'zero_w1', 'zero_w2', 'coincident', 'hub1_%dx33_translated' % (top + 1)):
        assert extra in names, extra
    # a shape that needs the raised limit is never the first LDS-path shape of the list (the process-wide marks)
    paths = [c['meta']['path'] for c in CASES.values()]
    assert paths.index('lds') < paths.index('lds_raised')
    # the fused kernel's sizes: a multiple and a non-multiple of its block, more than one 8-pass round, its largest M
    blk = k['SCB_BLOCK']
    assert max(C.FUSED_M) == k['VPN_FUSED_BWD_MAX_GT'] and k['VPN_FUSED_BWD_MAX_GT'] % blk == 0
    assert any(m % blk for m in C.FUSED_M) and any(m > 8 * blk and m % blk for m in C.FUSED_M)


@pytest.mark.parametrize('M', [300, 7680])
def test_fused_hub_batch_fills_the_match_lists(M):
    """In the hub batch every GT point's nearest predicted point (float64 sampler, dense search) lies on primitive 0; in the
    even batch every primitive gets its share."""
    import pose_domain_ref as P
    k = _source_constants()
    K, n = C.FUSED_K, C.FUSED_N
    for hub_batch in (True, False):
        params, kinds, gt, gl = C.fused_batch(torch.Generator().manual_seed(5), M, hub_batch)
        u = torch.rand(params.shape[0], K, n, 3, generator=torch.Generator().manual_seed(6))
        pts = P.sample(params.double(), kinds, u, P.face_counts(params, kinds, n))
        _, _, _, i2 = O.chamfer_nn(pts, gt.double())
        owner = i2 // n
        if hub_batch:
            assert (owner == 0).all()
            # wave w of the workgroup of primitive 0 looks at ceil(M / block) * 64 entries, all below M when M is a multiple
            if M % k['SCB_BLOCK'] == 0:
                assert (M + k['SCB_BLOCK'] - 1) // k['SCB_BLOCK'] * 64 * (k['SCB_BLOCK'] // 64) == M
        else:
            counts = torch.stack([(owner == p).sum(1) for p in range(K)], 1)
            assert (counts >= M // (2 * K)).all(), counts
