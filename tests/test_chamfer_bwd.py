"""GPU tests of the Chamfer backward on every launch path, against the float64 statement of tests/chamfer_bwd_ref.py, element
by element at the derived bar (n_r + 8) 2^-23 S_r and norm-wise at 1e-4:

  * vpn_chamfer_bwd at the C ABI on every case of the reference file -- the LDS kernel below and above the 64 KB it may ask
    for without a raised limit, at its largest cloud, the two-kernel global path at its smallest, in both roles of the clouds
    -- into outputs pre-filled with NaN (written, not accumulated), as both gradients and as either alone;
  * the raised limit requested by the first LDS-path call of a fresh process;
  * ChamferDistanceLoss and HotPathLossFunction's fallback branch (M > VPN_FUSED_BWD_MAX_GT) on the global path;
  * vpn_sample_chamfer_bwd with full match lists, M off the block size, more than one 8-pass round and M at its limit;
  * a NaN point in either cloud.
The LDS and the global path add with float atomics in arbitrary order: no bit-equality between two runs is asked of them.

Measured on an MI355X (the file: 61 tests in 5.3 s), worst over all cases, call forms and the module-level runs of a path:
    path                                   |got - ref| / bar    norm-wise
    LDS kernel, default limit              0.27                 4.7e-07
    LDS kernel, limit raised above 64 KB   0.28                 8.9e-07
    global path (direct + scatter)         0.31                 1.6e-06 .. 2.8e-06 from run to run (a 12289-term row)
    fused kernel, per primitive            against float64 4.4e-06 (bar 1e-4), against the unfused pair 2.9e-06 (bar 1e-5);
                                           the hot-path fallback against float64 1.1e-05 .. 1.9e-05 (bar 1e-4)
What the tests found, by reading, before any backward ran on such input: the filtered scan's index of a NaN query
(0x7fffffff) was read through by all four backward kernels (test_nan_point_in_either_cloud's docstring)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT                      # first: it puts the repository root on sys.path (this file also runs as a script)
import chamfer_bwd_ref as C
import pose_domain_ref as P
from oracle import vpn_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NO_NEIGHBOUR = 0x7fffffff


@pytest.fixture(scope='module')
def vpn():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU (no CPU fallback exists)')
    import vpn_amd
    vpn_amd._lib.lib()
    return vpn_amd


def g(t):
    return (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)


# ----------------------------------------------------------------------------- holding a gradient to the statement
def held(label, got, ref, n, S):
    """Prints, then asserts: got is NaN in exactly the rows the statement says; every other element within the bar; the
    tensor within 1e-4 norm-wise.  Returns (worst |got - ref| / bar, norm-wise error)."""
    got = got.detach().cpu().numpy().astype(np.float64)
    nan = np.isnan(ref).any(2)
    err, lim = np.abs(got - ref)[~nan], C.bar(n, S)[~nan]
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where((err == 0) & (lim == 0), 0.0, err / lim)
    worst = float(ratio.max()) if ratio.size else 0.0
    top = float(np.abs(ref[~nan]).max()) if ratio.size else 0.0
    norm = float(err.max() / top) if top > 0 else (0.0 if not ratio.size or err.max() == 0 else np.inf)
    print('BWD %-44s |got-ref|/bar %.3f  norm-wise %.2e  rows %d (NaN %d, n_r max %d)' % (label, worst, norm, nan.size, nan.sum(), n.max()))
    assert np.array_equal(np.isnan(got).any(2), nan), label + ': NaN rows differ from the statement'
    assert worst <= 1.0, '%s: |got - ref| / bar = %.3f' % (label, worst)
    assert norm <= C.NORM_BAR, '%s: norm-wise %.2e' % (label, norm)
    return worst, norm


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def chamfer_bwd(case, nn, want1=True, want2=True):
    """vpn_chamfer_bwd at the C ABI into outputs full of NaN; (grad_p1 | None, grad_p2 | None)."""
    from vpn_amd import _lib
    p1, p2, gl = g(case['p1']), g(case['p2']), g(case['gl'])
    d1, i1, d2, i2 = nn
    B, N, M = p1.shape[0], p1.shape[1], p2.shape[1]
    g1 = torch.full_like(p1, float('nan')) if want1 else None
    g2 = torch.full_like(p2, float('nan')) if want2 else None
    _lib.call('vpn_chamfer_bwd', p1, p2, d1, i1, d2, i2, gl, B, N, M, case['w1'], case['w2'], g1, g2, _lib.stream())
    return g1, g2


def check_case(vpn, case, dense=True):
    """The three call forms of one case, held; returns the worst (ratio, norm-wise)."""
    nn = vpn.chamfer_nn(g(case['p1']), g(case['p2']))
    i1, i2 = nn[1].cpu().numpy().astype(np.int64), nn[3].cpu().numpy().astype(np.int64)
    if dense:
        r1, r2 = C.neighbours(case, O.chamfer_nn_ieee)
        assert np.array_equal(i1, r1) and np.array_equal(i2, r2), case['name'] + ': neighbours differ from the dense CPU search'
    (ref1, n1, S1), (ref2, n2, S2) = C.both(case, i1, i2)
    b1, b2 = chamfer_bwd(case, nn)
    a1, none2 = chamfer_bwd(case, nn, want2=False)
    none1, a2 = chamfer_bwd(case, nn, want1=False)
    assert none1 is None and none2 is None
    figures = [held(case['name'] + ' grad_p1 (both)', b1, ref1, n1, S1), held(case['name'] + ' grad_p2 (both)', b2, ref2, n2, S2),
               held(case['name'] + ' grad_p1 alone', a1, ref1, n1, S1), held(case['name'] + ' grad_p2 alone', a2, ref2, n2, S2)]
    # rows without a scatter term see no atomic: the same bits whichever call wrote them
    for both_, alone, n in ((b1, a1, n1), (b2, a2, n2)):
        rows = torch.from_numpy(n == 0).to(DEV)
        assert same_bits(both_[rows], alone[rows]), case['name'] + ': rows with n_r = 0 differ between the call forms'
    return max(f[0] for f in figures), max(f[1] for f in figures)


# ----------------------------------------------------------------------------- C ABI, every case
@pytest.mark.parametrize('name', C.case_names())
def test_chamfer_bwd_against_statement(vpn, name):
    """In the order of the case list: the first LDS-path shapes of the process fit the default limit, the raised one comes
    later (test_first_lds_call_of_a_process_needs_the_raised_limit has it the other way round)."""
    check_case(vpn, C.cases()[name])


def _child():
    """A fresh process whose FIRST LDS-path call needs the raised limit, followed by one that does not and one at the top."""
    import vpn_amd
    vpn_amd._lib.lib()
    out = {}
    for name in ('lds_raise_5462x40', 'ragged_63x65', 'lds_max_33x12288'):
        out[name] = check_case(vpn_amd, C.cases()[name])
    print('CHILD ' + json.dumps(out))


def test_first_lds_call_of_a_process_needs_the_raised_limit():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--first-call-raised'], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith('CHILD ')]
    assert len(line) == 1 and len(json.loads(line[0][6:])) == 3, r.stdout


# ----------------------------------------------------------------------------- module level
@pytest.mark.parametrize('each_batch', [False, True])
@pytest.mark.parametrize('name', ['global_min_12289x700', 'global_min_33x12289', 'hub1_12289x33', 'hub1_33x12289'])
def test_chamfer_loss_module_on_the_global_path(vpn, name, each_batch):
    """ChamferDistanceLoss with both clouds requiring grad: its backward hands vpn_chamfer_bwd uninitialised outputs."""
    case = dict(C.cases()[name])
    B = len(case['gl'])
    if not each_batch:
        case['gl'] = np.full(B, 1.0 / B, np.float32)             # the mean over the batch (exact: B = 2)
    a, b = g(case['p1']).requires_grad_(True), g(case['p2']).requires_grad_(True)
    loss = vpn.ChamferDistanceLoss()(a, b, each_batch=each_batch, w1=case['w1'], w2=case['w2'])
    ((loss * g(case['gl'])).sum() if each_batch else loss).backward()
    _, i1, _, i2 = vpn.chamfer_nn(a, b)
    (ref1, n1, S1), (ref2, n2, S2) = C.both(case, i1.cpu().numpy(), i2.cpu().numpy())
    label = '%s module each_batch=%s' % (name, each_batch)
    held(label + ' grad_p1', a.grad, ref1, n1, S1)
    held(label + ' grad_p2', b.grad, ref2, n2, S2)


HOT_K, HOT_N, HOT_SEED = 4, 64, 5


def _hot_case(gen, M):
    params, kinds, gt, _ = C.fused_batch(gen, M, False)
    B = params.shape[0]
    u = O.philox_uniforms(HOT_SEED, 0, B, HOT_K, HOT_N)
    gl = torch.full((B,), 1.0 / B)
    pts = P.sample(params, kinds, u, P.face_counts(params, kinds, HOT_N))
    _, i1, _, i2 = O.chamfer_nn(pts, gt)
    r64 = P.chamfer_sampler_ref(params, kinds, u, gt, i1, i2, gl, 0.7, 1.3)
    r32 = P.chamfer_sampler_ref(params, kinds, u, gt, i1, i2, gl, 0.7, 1.3, torch.float32)
    return (params, kinds, gt, gl, u), r64, _group_max(r32, r64)


def _group_max(ga, gb):
    return {k: float(e.max()) for k, e in P.param_group_errors(ga, gb).items()}


def _hold(label, errs, bar=P.BAR):
    msg = label + ': ' + '  '.join('%s %.2e' % (k, e) for k, e in errs.items())
    print('FUSED ' + msg)
    assert all(e <= bar for e in errs.values()), msg


@pytest.mark.parametrize('M', [7681, 12289])
def test_hot_path_fallback_against_float64(vpn, M):
    """HotPathLossFunction beyond the fused backward's limit (vpn_chamfer_bwd, LDS path at 7681 and global path at 12289, then
    vpn_sample_bwd), image weights 0: grad_params per primitive against the statement's loss through the float64 sampler
    (P.chamfer_sampler_ref with the GPU's neighbours), on a draw chosen by the fp32 oracle alone (P.conditioned)."""
    (params, kinds, gt, gl, u), _, _ = P.conditioned(lambda gen: _hot_case(gen, M), 7000 + M)
    B, H, W = params.shape[0], 32, 32
    kt = vpn.kinds_tensor(kinds, torch.device(DEV))
    cam = g(torch.tensor([[1.0, 0.0, 0.0]]).expand(B, 3).contiguous())
    sil = torch.zeros(B, 1, H, W, device=DEV)
    pg = g(params).requires_grad_(True)
    out = vpn.HotPathLossFunction.apply(pg, kt, cam, g(gt), sil, None, HOT_N, HOT_SEED, 0, H, W, 0.05, 0.1, 2.0, 1.0, 0.0, 0.0, 0.7, 1.3)
    out[2].backward()
    pts = vpn.Sampling.sample_primitives(g(params), kt, HOT_N, seed=HOT_SEED)
    _, i1, _, i2 = vpn.chamfer_nn(pts, g(gt))
    r64 = P.chamfer_sampler_ref(params, kinds, u, gt, i1.cpu(), i2.cpu(), gl, 0.7, 1.3)
    _hold('hot path fallback M=%d against float64' % M, _group_max(pg.grad.cpu(), r64))


# ----------------------------------------------------------------------------- the fused kernel
W1, W2 = 0.7, 1.3


def _fused_conditioned(M, hub_batch):
    """The first draw on which the fp32 ORACLE's gradient is within REF_BAR / 20 of float64 per primitive: the selection of
    test_pose_domain._thin_conditioned (the margin the 1e-5 bar between the fused and the unfused kernels presumes) at half
    its figure, because the unfused pair adds up to M / K = 1920 scatter terms per primitive with LDS atomics in an order that
    changes from run to run, and so does its distance from float64.  The choice looks at the CPU oracle only."""
    K, n = C.FUSED_K, C.FUSED_N
    for s in range(3100 + M, 3100 + M + 64):
        gen = torch.Generator().manual_seed(s)
        params, kinds, gt, gl = C.fused_batch(gen, M, hub_batch)
        u = torch.rand(params.shape[0], K, n, 3, generator=gen)
        pts = P.sample(params, kinds, u, P.face_counts(params, kinds, n))
        _, i1, _, i2 = O.chamfer_nn(pts, gt)
        g64 = P.chamfer_sampler_ref(params, kinds, u, gt, i1, i2, gl, W1, W2)
        g32 = P.chamfer_sampler_ref(params, kinds, u, gt, i1, i2, gl, W1, W2, torch.float32)
        if max(_group_max(g32, g64).values()) <= P.REF_BAR / 20:
            return params, kinds, gt, gl, u
    raise AssertionError('no draw on which the fp32 oracle stays within %.1e of float64' % (P.REF_BAR / 20))


@pytest.mark.parametrize('hub_batch', [True, False])
@pytest.mark.parametrize('M', C.FUSED_M)
def test_fused_backward_full_lists_and_odd_sizes(vpn, M, hub_batch):
    """vpn_sample_chamfer_bwd, K = 4, n = 64: in the hub batch every GT point's nearest predicted point lies on primitive 0, so
    the match lists of that workgroup's waves fill (to their capacity exactly at M = 7680); M = 129 is no multiple of the
    block, 1025 needs more than one 8-pass round.  Per primitive against float64 at 1e-4, against the unfused pair at 1e-5,
    and two runs bit-equal (asserted inside _fused_backward)."""
    from test_pose_domain import _fused_backward
    params, kinds, gt, gl, u = _fused_conditioned(M, hub_batch)
    n = C.FUSED_N
    fused, unfused, i1, i2 = _fused_backward(vpn, g(params), vpn.kinds_tensor(kinds, torch.device(DEV)), g(u), 0, n, g(gt), g(gl), W1, W2)
    if hub_batch:
        assert bool((i2 // n == 0).all()), 'the hub batch does not fill the match lists of primitive 0'
    t64 = P.chamfer_sampler_ref(params, kinds, u, gt, i1, i2, gl, W1, W2)
    label = 'fused backward M=%d %s' % (M, 'hub' if hub_batch else 'even')
    _hold(label + ' against float64', _group_max(fused, t64))
    _hold(label + ' unfused against float64', _group_max(unfused, t64))
    _hold(label + ' against unfused', _group_max(fused, unfused), bar=1e-5)


def test_fused_backward_rejects_one_point_too_many(vpn):
    """M = VPN_FUSED_BWD_MAX_GT + 1: VPN_E_TOOBIG from the C ABI before anything is launched (the output keeps its NaN); the
    op takes the two-kernel branch instead (test_hot_path_fallback_against_float64 at the same M)."""
    from vpn_amd import _lib, ops
    M = _lib.CONSTANTS['VPN_FUSED_BWD_MAX_GT'] + 1
    assert M == 7681 and ops.FUSED_BWD_MAX_GT == M - 1
    params, kinds, gt, gl = C.fused_batch(torch.Generator().manual_seed(1), M, False)
    B, K, n = params.shape[0], C.FUSED_K, C.FUSED_N
    kt = vpn.kinds_tensor(kinds, torch.device(DEV))
    pts = vpn.Sampling.sample_primitives(g(params), kt, n, seed=3)
    d1, i1, d2, i2 = vpn.chamfer_nn(pts, g(gt))
    out = torch.full((B, K, 10), float('nan'), device=DEV)
    pr, gtd, gld = g(params), g(gt), g(gl)
    rc = _lib.lib().vpn_sample_chamfer_bwd(_lib.ptr(pr), _lib.ptr(kt), None, 3, None, 0, B, K, n, _lib.ptr(pts), _lib.ptr(gtd), M,
                                           _lib.ptr(d1), _lib.ptr(i1), _lib.ptr(d2), _lib.ptr(i2), _lib.ptr(gld), W1, W2,
                                           _lib.ptr(out), _lib.stream())
    assert rc == _lib.CONSTANTS['VPN_E_TOOBIG'], rc
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ----------------------------------------------------------------------------- NaN points
def _true_neighbours(p, q, idx):
    """For the finite points of p [B,N,3]: idx is in range and its fp32 distance is the smallest to any finite point of q."""
    for b in range(p.shape[0]):
        fin = np.isfinite(p[b]).all(1)
        d = p[b][:, None, :] - q[b][None, :, :]
        d = np.sqrt(((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2]))
        if not ((idx[b][fin] >= 0) & (idx[b][fin] < q.shape[1])).all():
            return False
        if not np.array_equal(d[fin, idx[b][fin]], np.nanmin(d[fin], 1)):
            return False
    return True


NAN_SHAPES = [(300, 200), (1025, 1023), (12289, 33), (33, 12289)]
# auto never takes the filtered scan below 512 x 512 pairs, and the scan is not asked for there
NAN_RUNS = [(s, m) for s in NAN_SHAPES for m in ('auto', 'brute', 'mfma16') if m != 'mfma16' or s[0] * s[1] >= 512 * 512]


@pytest.mark.parametrize('shape,mode', NAN_RUNS, ids=['%dx%d-%s' % (s[0], s[1], m) for s, m in NAN_RUNS])
def test_nan_point_in_either_cloud(vpn, shape, mode):
    """One all-NaN point per cloud (sample 0), neighbours from the forward in each scan `auto` can resolve to ('brute' below
    512 x 512 pairs, 'mfma16' from there on; both are also forced at every shape they accept).

    What the forward returns, read from csrc/chamfer.hip and confirmed by running the forward alone:
      * brute force: a query with a NaN coordinate never lowers its running minimum (every comparison with NaN is false):
        dist = inf, idx = 0 -- in range.  An infinite query: dist = inf, idx = 0 as well.  A NaN target is never selected
        (fminf drops it), every finite query keeps its true neighbour.
      * the fp16-filtered scan: dist = inf, idx = 0x7fffffff for a query with a NaN coordinate (one or all three) -- OUT of
        range; an infinite query gets dist = inf and some index in range (0, 1, 9 seen).  chamfer_bwd_lds_kernel,
        chamfer_bwd_direct_kernel, chamfer_bwd_scatter_kernel and sample_chamfer_bwd_kernel used to read (and the first
        three to add) through that index; the first three now test it against the cloud's size: the point's own row is NaN,
        the pair scatters nothing (the fused kernel clamps it: test_fused_backward_primitive_of_nan_points).  Finite queries
        keep a true nearest neighbour among the finite targets.
    So: the NaN point's own row is NaN; with brute force row 0 of the other cloud, which it was pointed at, is NaN too
    (0 * NaN); every other row is held to the bar."""
    N, M = shape
    case = C.nan_points(N, M)
    d1, i1, d2, i2 = nn = vpn.chamfer_nn(g(case['p1']), g(case['p2']), mode=mode)
    h1, h2 = i1.cpu().numpy().astype(np.int64), i2.cpu().numpy().astype(np.int64)
    q1, q2 = case['meta']['nan_p1'][0], case['meta']['nan_p2'][0]
    print('NAN %s %s: query p1[0,%d] -> idx %d dist %s; query p2[0,%d] -> idx %d dist %s' % (
        shape, mode, q1, h1[0, q1], float(d1[0, q1]), q2, h2[0, q2], float(d2[0, q2])))
    filtered = mode == 'mfma16' or (mode == 'auto' and N * M >= 512 * 512)
    assert h1[0, q1] == h2[0, q2] == (NO_NEIGHBOUR if filtered else 0)
    assert _true_neighbours(case['p1'], case['p2'], h1) and _true_neighbours(case['p2'], case['p1'], h2)
    (ref1, n1, S1), (ref2, n2, S2) = C.both(case, h1, h2)
    nan1, nan2 = np.isnan(ref1).any(2), np.isnan(ref2).any(2)
    assert nan1[0, q1] and nan2[0, q2] and nan1.sum() == nan2.sum() == (1 if filtered else 2) and not nan1[1].any()
    b1, b2 = chamfer_bwd(case, nn)
    held('%s %s grad_p1' % (case['name'], mode), b1, ref1, n1, S1)
    held('%s %s grad_p2' % (case['name'], mode), b2, ref2, n2, S2)


def test_fused_backward_primitive_of_nan_points(vpn):
    """A NaN translation makes the 64 points of primitive (0, 1) NaN; at K n M = 256 x 1025 pairs the forward is the filtered
    scan, which gives them idx1 = 0x7fffffff.  sample_chamfer_bwd_kernel clamps the index and reads nothing outside the GT
    cloud: that primitive's gradient is NaN (through the points' own coordinates), the others of its sample are finite, sample 1 has the bits of the run without the NaN, and the unfused pair
    (vpn_chamfer_bwd + vpn_sample_bwd) shows the same NaN pattern."""
    from test_pose_domain import _fused_backward
    M, n = 1025, C.FUSED_N
    gen = torch.Generator().manual_seed(77)
    params, kinds, gt, gl = C.fused_batch(gen, M, False)
    u = torch.rand(params.shape[0], C.FUSED_K, n, 3, generator=gen)
    kt = vpn.kinds_tensor(kinds, torch.device(DEV))
    clean, _, _, _ = _fused_backward(vpn, g(params), kt, g(u), 0, n, g(gt), g(gl), W1, W2)
    bad = params.clone()
    bad[0, 1, 7:10] = float('nan')
    # _fused_backward compares its two runs with torch.equal, which no NaN passes: the same calls here, compared by bits
    from vpn_amd import _lib
    B, K = bad.shape[0], C.FUSED_K
    pb, ud, gtd, gld = g(bad), g(u), g(gt), g(gl)
    pts = vpn.Sampling.sample_primitives(pb, kt, n, u=ud)
    d1, i1, d2, i2 = vpn.chamfer_nn(pts, gtd)
    gp = torch.full_like(pts, float('nan'))
    _lib.call('vpn_chamfer_bwd', pts, gtd, d1, i1, d2, i2, gld, B, K * n, M, W1, W2, gp, None, _lib.stream())
    unfused = torch.empty_like(pb)
    _lib.call('vpn_sample_bwd', pb, kt, ud, 0, None, 0, B, K, n, gp, unfused, _lib.stream())
    runs = []
    for _ in range(2):
        out = torch.empty_like(pb)
        _lib.call('vpn_sample_chamfer_bwd', pb, kt, ud, 0, None, 0, B, K, n, pts, gtd, M, d1, i1, d2, i2, gld, W1, W2, out, _lib.stream())
        runs.append(out)
    fused, i1, i2 = runs[0], i1.cpu(), i2.cpu()
    assert bool(torch.isnan(runs[0]).equal(torch.isnan(runs[1]))) and same_bits(runs[0][1], runs[1][1])
    assert bool((i1[0, n:2 * n] == NO_NEIGHBOUR).all()) and int((i1 == NO_NEIGHBOUR).sum()) == n
    assert bool(((i2 >= 0) & (i2 < C.FUSED_K * n)).all()) and not bool((i2[0] // n == 1).any())
    for name, out in (('fused', fused), ('unfused', unfused)):
        nan = torch.isnan(out).any(2).cpu()
        assert bool(torch.isnan(out[0, 1]).all()) and int(nan.sum()) == 1, (name, nan)
    assert same_bits(fused[1], clean[1])


if __name__ == '__main__':
    assert sys.argv[1:] == ['--first-call-raised'], sys.argv
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    _child()
