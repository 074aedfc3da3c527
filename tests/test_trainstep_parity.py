"""TrainStepLossFunction (BASELINE config C5) and the kernels around it, pinned the way the hot path is: the one-launch
backward `vpn_trainstep_bwd` (sample_chamfer_bwd_kernel<true>: view-centred Chamfer, object-centred Chamfer through the
camera matrix, raster finish, VP-diversity, EMD) on mixed kinds and on the shapes at which it takes another path, term by
term, block by block (v, q, t), under an upstream gradient that is not 1 and with the options of the step; the VP-diversity
neighbours (vpdiv_fwd_kernel, both merge routes) and the reduction (trainstep_finalize_kernel) through the C ABI.

References: the fp32 oracle (oracle.train_step) at the project's 1e-4 bar, and the float64 restatement with the oracle's
discrete decisions (tests/trainstep_ref.py) for the element-wise rule of _raster_case in tests/test_gpu_parity.py.
tests/test_trainstep_ref_cpu.py holds the oracle itself within 5e-5 of float64 for every step used here, so no escape
clause is needed."""
import pytest
import torch

from conftest import elem_rel_err, rel_err
import trainstep_ref as R
from oracle import vpn_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
RTOL = 1e-4            # north_star: fp32 parity with the oracle
ELEM_TOL = 1e-3        # the element-wise rule of tests/test_gpu_parity.py::_raster_case
SAME_ARITH = 1e-5      # the project's bar between two launch paths over the same arithmetic


@pytest.fixture(scope='module')
def vpn():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU (no CPU fallback exists)')
    import vpn_amd
    vpn_amd._lib.lib()
    return vpn_amd


def g(t):
    return t.to(DEV)


def _step(vpn, case, kn, w, opts=None, seed=R.SEED, advance=False, params=None, backward=lambda total: total.backward()):
    """One TrainStepLossFunction step of a case -> (losses [6] on the host, gradient [B,K,10] on the host)."""
    opts = dict(opts or {})
    opts.pop('grad_scale', None)
    B, K, n, M, Mc, H, W, _ = R.CASES[case]
    inputs = R.batch(case)
    p = g(inputs[0] if params is None else params).clone().requires_grad_(True)
    kinds = vpn.kinds_tensor(R.kinds_of(kn, K), torch.device(DEV))
    assert vpn._lib.lib().vpn_hotpath_fused_features(B, K, n, M) == 1, 'the case must be a shape the step takes'
    out = vpn.TrainStepLossFunction.apply(p, kinds, *[g(x) for x in inputs[1:]], n, seed, opts.get('sample_base', 0), H, W, w,
                                          0.005, 50, advance, opts.get('cd_w1', 1.0), opts.get('cd_w2', 1.0),
                                          opts.get('sil_mse', False))
    backward(out[5])
    torch.cuda.synchronize()
    return torch.stack([o.detach() for o in out]).cpu(), p.grad.cpu()


def _references(vpn, step_id):
    """The references of a step.  Where the EMD term is on, their auction assigns the cloud the sampler KERNEL draws for the
    step (see oracle.train_step: the auction is chaotic under the rounding that separates two samplers); the assignment
    is the oracle's own, so the kernel's auction has to reproduce it."""
    _, case, kn, w, opts = R.STEP_BY_ID[step_id]
    if not w[4]:
        return R.references(step_id)
    B, K, n = R.CASES[case][:3]
    with torch.no_grad():
        pts = vpn.Sampling.sample_primitives(g(R.batch(case)[0]), R.kinds_of(kn, K), n, seed=R.SEED,
                                             sample_base=opts.get('sample_base', 0)).cpu()
    return R.references_for(step_id, emd_points=pts)


def _check_grad(tag, mine, g32, g64, weights):
    """Per block: identically zero where the reference is; <= 1e-4 of the fp32 oracle; element-wise against float64 no worse
    than 1e-3 nor than 4x the fp32 oracle itself (test_gpu_parity.py::_raster_case, without its escape clause)."""
    zero = R.zero_blocks(weights)
    for name, sl in R.BLOCKS:
        m, r32, r64 = mine[..., sl], g32[..., sl], g64[..., sl]
        if name in zero:
            assert int(torch.count_nonzero(r64)) == 0 and int(torch.count_nonzero(m)) == 0, (tag, name)
            continue
        e = rel_err(m, r32)
        ee_gpu, ee_cpu = elem_rel_err(m, r64), elem_rel_err(r32, r64)
        print('%s %s: rel_err vs fp32 oracle %.2e | elem_rel_err vs float64 %.2e (oracle %.2e)' % (tag, name, e, ee_gpu, ee_cpu))
        assert e <= RTOL, (tag, name, e)
        assert ee_gpu <= max(ELEM_TOL, 4 * ee_cpu), (tag, name, ee_gpu, ee_cpu)


# ----------------------------------------------------------------------------- the step against both references
PARITY_STEPS = [s for s in R.STEP_IDS if 'scale' not in s and 'hot' not in s]


@pytest.mark.parametrize('step_id', PARITY_STEPS)
def test_trainstep_parity(vpn, step_id):
    """Mixed kinds, every path of the backward kernel (cases A to E of trainstep_ref.CASES), each of the five terms alone
    (a zero weight also drives the NULL-pointer and render = False branches) and the options cd_w1 != cd_w2, sil_mse,
    sample_base != 0."""
    _, case, kn, w, opts = R.STEP_BY_ID[step_id]
    l32, g32, _, g64 = _references(vpn, step_id)
    got, grad = _step(vpn, case, kn, w, opts)
    print(step_id, 'losses', got.tolist(), 'oracle', l32.tolist())
    assert torch.allclose(got, l32, rtol=1e-4, atol=1e-6), (got, l32)
    _check_grad(step_id, grad, g32, g64, w)


# ----------------------------------------------------------------------------- upstream gradient
def _upstream_checks(vpn, tag, run, ref_scaled):
    """run(backward) -> gradient.  A power-of-two factor commutes with every rounding in the kernel: bit-equal; 0.3 agrees
    with 0.3 x the unscaled gradient to the same-arithmetic bar per block, and with the references under grad_scale = 0.3."""
    g1 = run(lambda total: total.backward())
    gm4 = run(lambda total: (total * -4.0).backward())
    assert torch.equal(gm4, -4.0 * g1), (tag, rel_err(gm4, -4.0 * g1))
    g03 = run(lambda total: total.backward(torch.tensor(0.3, device=DEV)))
    want = g1.double() * float(torch.tensor(0.3, dtype=torch.float32))
    for name, sl in R.BLOCKS:
        e = rel_err(g03[..., sl], want[..., sl])
        print('%s %s: 0.3 upstream vs 0.3 x gradient %.2e' % (tag, name, e))
        assert e <= SAME_ARITH, (tag, name, e)
    _, g32, _, g64 = _references(vpn, ref_scaled)
    _check_grad(tag + ' x0.3', g03, g32, g64, R.STEP_BY_ID[ref_scaled][3])


def test_trainstep_upstream_gradient(vpn):
    """The kernel multiplies the upstream gradient into seven separately written coefficients (both Chamfer directions of
    both clouds, EMD, both VP-diversity directions, the raster finish): loss scaling and gradient accumulation rely on each."""
    _upstream_checks(vpn, 'step', lambda bw: _step(vpn, 'A', 'mixed', R.W_ALL, backward=bw)[1], 'A-mixed-scale')


def test_hot_path_upstream_gradient(vpn):
    """The same three checks on HotPathLossFunction (the <false> variant of the kernel): its total, w_cd Chamfer + w_sil
    silhouette under the view-centred camera, is the step of weights W_HOT."""
    B, K, n, M, Mc, H, W, _ = R.CASES['A']
    params, gt_view, _, gt_sil = R.batch('A')[:4]
    kinds = vpn.kinds_tensor(R.kinds_of('mixed', K), torch.device(DEV))
    cam = g(torch.tensor([[1.0, 0.0, 0.0]]).expand(B, 3).contiguous())
    cfg = vpn.config

    def run(backward, losses=None):
        p = g(params).clone().requires_grad_(True)
        out = vpn.HotPathLossFunction.apply(p, kinds, cam, g(gt_view), g(gt_sil), None, n, R.SEED, 0, H, W, cfg.RASTER_SIGMA,
                                            cfg.RASTER_GAMMA, cfg.RASTER_Z_FAR, R.W_HOT[0], R.W_HOT[2], 0.0)
        backward(out[2])
        torch.cuda.synchronize()
        if losses is not None:
            losses.append(float(out[2].detach()))
        return p.grad.cpu()
    l32, g32, _, g64 = R.references('A-mixed-hot')
    total = []
    g1 = run(lambda t: t.backward(), total)
    assert abs(total[0] - float(l32[5])) <= 1e-4 * abs(float(l32[5])) + 1e-6, (total, l32)
    _check_grad('hot', g1, g32, g64, R.W_HOT)
    _upstream_checks(vpn, 'hot', run, 'A-mixed-hot-scale')


# ----------------------------------------------------------------------------- thin primitive, device seed
@pytest.mark.parametrize('kn', ['spheres', 'mixed'])
def test_trainstep_advance_seed_thin_primitive(vpn, kn):
    """tests/test_gpu_parity.py::test_hot_path_advance_seed for the step, which passes no uniforms and reads the seed its
    sampler launch kept in the loss workspace: a THIN primitive (a sphere, or the first cuboid of the mixed kinds) makes the
    backward redraw the Philox uniforms, so a backward that read the advanced counter would redraw other points."""
    params = R.batch('A')[0].clone()
    params[0, 0, :3] = torch.tensor([1e-5, 0.05, 0.04])
    ref_l, ref_g = _step(vpn, 'A', kn, R.W_ALL, seed=R.SEED, params=params)
    assert bool(torch.isfinite(ref_g).all()) and bool(torch.isfinite(ref_l).all())
    counter = torch.full((1,), R.SEED, dtype=torch.int64, device=DEV)
    l1, g1 = _step(vpn, 'A', kn, R.W_ALL, seed=counter, advance=True, params=params)
    assert int(counter.item()) == R.SEED + 1
    assert torch.equal(l1, ref_l) and torch.equal(g1, ref_g)
    l2, g2 = _step(vpn, 'A', kn, R.W_ALL, seed=counter, advance=True, params=params)     # the next step draws other points
    assert int(counter.item()) == R.SEED + 2 and not torch.equal(l2, l1)
    assert rel_err(g2[0, 0], g1[0, 0]) > 1e-3                                            # ... the thin primitive's gradient with them
    ref2_l, ref2_g = _step(vpn, 'A', kn, R.W_ALL, seed=R.SEED + 1, params=params)
    assert torch.equal(l2, ref2_l) and torch.equal(g2, ref2_g)


def test_trainstep_ground_truth_limit(vpn):
    """One ground-truth point beyond the backward launch's match lists: a Python exception from forward(), before any
    launch, not an error out of the backward after the forward has run (and never a fault)."""
    import vpn_amd.ops as ops
    B, K, n, M, Mc, H, W, _ = R.CASES['A']
    inputs = R.batch('A')
    Mbig = ops.FUSED_BWD_MAX_GT + 1
    assert Mbig == 7681 and K * n == 512
    gen = torch.Generator().manual_seed(1)
    gt_big = torch.rand(B, Mbig, 3, generator=gen) - 0.5
    p = g(inputs[0]).clone().requires_grad_(True)
    kinds = vpn.kinds_tensor(R.kinds_of('mixed', K), torch.device(DEV))
    with pytest.raises(ValueError, match='ground-truth points'):
        vpn.TrainStepLossFunction.apply(p, kinds, g(gt_big), *[g(x) for x in inputs[2:]], n, R.SEED, 0, H, W, R.W_D)
    torch.cuda.synchronize()
    # the limit itself is taken
    gt_max = gt_big[:, :ops.FUSED_BWD_MAX_GT].contiguous()
    out = vpn.TrainStepLossFunction.apply(p, kinds, g(gt_max), *[g(x) for x in inputs[2:]], n, R.SEED, 0, H, W, R.W_D)
    out[5].backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0


# ----------------------------------------------------------------------------- VP-diversity neighbours
def _vpdiv_both_routes(vpn, centres, gt):
    """vpn_vpdiv_fwd the way ops.py calls it, through both merge routes -> ((d1, i1, d2, i2) of vpdiv_merge_kernel,
    (d1, i1, d2, i2) of the merge inside vpn_trainstep_finalize)."""
    L = vpn._lib
    B, K, _ = centres.shape
    M = gt.shape[1]
    params = torch.zeros(B, K, 10)
    params[..., 7:10] = centres
    params, gtd = g(params), g(gt.contiguous())
    s = L.stream()
    routes = []
    for merged_by_finalize in (False, True):
        d1 = torch.full((B, K), -1.0, device=DEV)
        i1 = torch.full((B, K), -1, dtype=torch.int32, device=DEV)
        d2 = torch.full((B, M), -1.0, device=DEV)
        i2 = torch.full((B, M), -1, dtype=torch.int32, device=DEV)
        nbytes = L.lib().vpn_vpdiv_workspace(B, K)
        assert nbytes == B * 8 * K * 8
        dws = torch.empty((nbytes // 8,), dtype=torch.int64, device=DEV)
        if not merged_by_finalize:
            L.call('vpn_vpdiv_fwd', params, gtd, B, K, M, d1, i1, d2, i2, dws, s)
        else:
            L.call('vpn_vpdiv_fwd', params, gtd, B, K, M, None, None, d2, i2, dws, s)
            hot = torch.zeros(4, device=DEV)
            fws = torch.empty((L.lib().vpn_trainstep_workspace(B) // 4,), device=DEV)
            out = torch.empty(6, device=DEV)
            L.call('vpn_trainstep_finalize', hot, None, None, None, None, d2, B, K, M, 0, K, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0,
                   fws, dws, d1, i1, out, s)
        torch.cuda.synchronize()
        routes.append((d1.cpu(), i1.cpu(), d2.cpu(), i2.cpu()))
    return routes


def _vpdiv_check(vpn, centres, gt):
    m1, j1, m2, j2 = O.chamfer_nn_ieee(centres, gt)
    a, b = _vpdiv_both_routes(vpn, centres, gt)
    for d1, i1, d2, i2 in (a, b):
        assert torch.equal(i1.long(), j1) and torch.equal(i2.long(), j2)
        assert torch.equal(d1, m1) and torch.equal(d2, m2)              # bit-equal: correctly rounded sqrt on both sides
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('shape', [(1, 1, 1),            # one of everything: slices 1 to 7 are empty
                                   (2, 5, 9),            # per = 2: slices 5 to 7 are empty
                                   (2, 7, 1030),         # K does not divide 256, ragged last slice
                                   (1, 100, 300),        # nsl = 2 sub-slices with idle lanes
                                   (1, 300, 257),        # K >= 256: the second k0 trip
                                   (2, 64, 2048)])
def test_vpdiv_neighbours(vpn, shape):
    B, K, M = shape
    gen = torch.Generator().manual_seed(100 + K)
    centres = 0.35 * (torch.rand(B, K, 3, generator=gen) * 2 - 1)
    gt = torch.rand(B, M, 3, generator=gen) - 0.5
    _vpdiv_check(vpn, centres, gt)


def test_vpdiv_lattice_ties(vpn):
    """Centres and ground truth on the lattice of multiples of 0.25 in [-0.5, 0.5]^3 (125 sites for 200 points: duplicates):
    many distances are exactly equal, the lowest index must win in both directions (the 2-ulp `near` path decides)."""
    B, K, M = 2, 12, 200
    gen = torch.Generator().manual_seed(12)
    centres = torch.randint(-2, 3, (B, K, 3), generator=gen).float() * 0.25
    gt = torch.randint(-2, 3, (B, M, 3), generator=gen).float() * 0.25
    centres[:, 5] = centres[:, 2]                                        # duplicate centres too
    m1, j1, m2, j2 = O.chamfer_nn_ieee(centres, gt)
    s = torch.from_numpy(__import__('numpy').sqrt(((centres[:, :, None] - gt[:, None]) ** 2).sum(-1).numpy()))
    assert int((s == m1[..., None]).sum(-1).max()) > 1 and int((s == m2[:, None, :]).sum(1).max()) > 1    # ties exist both ways
    _vpdiv_check(vpn, centres, gt)


# ----------------------------------------------------------------------------- the reduction alone
@pytest.mark.parametrize('B', [1, 64, 65, 130])
@pytest.mark.parametrize('absent', [None, 'emd', 'cn', 'dv'])
def test_trainstep_finalize_alone(vpn, B, absent):
    """vpn_trainstep_finalize on synthetic positive arrays against a float64 evaluation of the formulas in the header
    comment of trainstep_finalize_kernel (lane l adds the samples l, l + 64, ...: B = 64, 65 and 130 fill one, start a
    second and start a third trip).  1e-6 relative covers B N <= 12480 fp32 additions of same-sign values in a tree
    order; two runs are bit-equal."""
    L = vpn._lib
    N, M, Mc, K = 96, 70, 45, 7
    gen = torch.Generator().manual_seed(B)
    pos = lambda *shape: torch.rand(*shape, generator=gen) + 0.05
    hot, emd, cn1, cn2, dv1, dv2 = pos(4), pos(B, N), pos(B, N), pos(B, Mc), pos(B, K), pos(B, M)
    wts = torch.tensor([0.9, 0.7, 1.3, 0.1, 1.1, 0.5, 2.0], dtype=torch.float32)     # view, can, sil, div, emd, cd_w1, cd_w2
    w = wts.double().tolist()
    has = {name: absent != name for name in ('emd', 'cn', 'dv')}
    d = lambda t: t.double()
    ref = [w[0] * d(hot[3]),
           w[1] * (w[5] * d(cn1).mean() + w[6] * d(cn2).mean()) if has['cn'] else torch.zeros((), dtype=torch.float64),
           w[2] * d(hot[0]),
           w[3] * (0.5 * d(dv1).mean() + 1.0 * d(dv2).mean()) if has['dv'] else torch.zeros((), dtype=torch.float64),
           w[4] * torch.sqrt(d(emd)).mean() if has['emd'] else torch.zeros((), dtype=torch.float64)]
    ref = torch.stack(ref + [sum(ref)])
    dev = [g(t) for t in (hot, emd, cn1, cn2, dv1, dv2)]
    fws = torch.empty((L.lib().vpn_trainstep_workspace(B) // 4,), device=DEV)
    assert fws.numel() == B * 8

    def run():
        out = torch.full((6,), -1.0, device=DEV)
        L.call('vpn_trainstep_finalize', dev[0], dev[1] if has['emd'] else None, dev[2] if has['cn'] else None,
               dev[3] if has['cn'] else None, dev[4] if has['dv'] else None, dev[5] if has['dv'] else None, B, N, M, Mc, K,
               *[float(x) for x in wts], fws, None, None, None, out, L.stream())
        torch.cuda.synchronize()
        return out.cpu()
    got, again = run(), run()
    err = ((got.double() - ref).abs() / ref.abs().clamp_min(1e-30)).tolist()
    print('finalize B=%d absent=%s: relative errors %s' % (B, absent, ['%.1e' % e for e in err]))
    for i in range(6):
        if float(ref[i]) == 0.0:
            assert float(got[i]) == 0.0, (i, got)
        else:
            assert err[i] <= 1e-6, (i, err[i], got, ref)
    assert torch.equal(got, again)
