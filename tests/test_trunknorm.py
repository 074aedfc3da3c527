"""GPU tests of the trunk's norm / add / ReLU op (csrc/trunknorm.hip, ops.BatchNormActFunction, ResNet18(fused_norm);
DESIGN.md 4.18).

Reference: the float64 restatement tests/trunknorm_ref.py on the CPU.  Yardstick: ATen's own fp32 CPU result on the same
inputs.  For every output T (y, dx, d_residual, d_gamma, d_beta, running_mean, running_var) with
e(T) = max|T - T64| / max|T64| the op must keep e_kernel(T) <= max(4 e_aten(T), 4 * 2^-24): the factor 4 covers a
different but fixed fp32 summation order.  Where ReLU is on, elements whose float64 pre-activation lies within 1e-4 of
zero are left out (a rounding may flip their mask): their upstream gradient is zero for the op, the yardstick and the
reference alike, so neither their own dx nor the channel sums depend on the flip; their share is asserted <= 0.1 %."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import trunknorm_ref as R

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -24
MOMENTUM, EPS = 0.1, 1e-5


def _ops():
    from vpn_amd import ops
    return ops


def _one_pass_max():
    import vpn_amd._lib as lib
    return lib.CONSTANTS['VPN_BN_ONE_PASS_MAX']


def e(t, t64):
    return float((t.double().cpu() - t64).abs().max() / t64.abs().max().clamp_min(1e-300))


def hold(name, got, ref64, aten, margin=4.0, report=None):
    ek, ea = e(got, ref64), e(aten, ref64)
    bound = max(margin * ea, margin * FLOOR)
    print('%-14s e_kernel %.3e  e_aten %.3e  bound %.3e' % (name, ek, ea, bound))
    if report is not None:
        report.append((name, ek / max(ea, FLOOR)))
    assert ek <= bound, (name, ek, ea, bound)


@functools.lru_cache(maxsize=None)
def inputs(shape, kind='normal', seed=11):
    """Seeded fp32 inputs on the CPU, shared by every test of a shape and never written to."""
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = torch.randn(shape, generator=g)
    if kind == 'shifted':                       # the cancellation case: E[x^2] - E[x]^2 loses every digit of the variance
        x = 10 + 0.05 * x
    rm = 0.1 * torch.randn(C, generator=g) + (10 if kind == 'shifted' else 0)
    rv = (1 + 0.2 * torch.rand(C, generator=g)) * (0.0025 if kind == 'shifted' else 1)
    return dict(x=x, res=torch.randn(shape, generator=g), dy=torch.randn(shape, generator=g),
                w=1 + 0.3 * torch.randn(C, generator=g), b=0.3 * torch.randn(C, generator=g), rm=rm, rv=rv)


@functools.lru_cache(maxsize=None)
def expected(shape, kind, relu, residual, training):
    """(the gradient actually sent back, the float64 reference, ATen's fp32 CPU result), each a dict of outputs."""
    c = inputs(shape, kind)
    d = {k: v.double() for k, v in c.items()}
    res64 = d['res'] if residual else None
    y, pre, mean, invstd, rm2, rv2, _n = R.forward(d['x'], d['w'], d['b'], d['rm'], d['rv'], torch.tensor(0), res64, training,
                                                   MOMENTUM, EPS, relu)
    dy = c['dy']
    if relu:
        near = pre.abs() < 1e-4
        share = float(near.double().mean())
        assert share <= 1e-3, share
        dy = torch.where(near, torch.zeros_like(dy), dy)
    dx, dw, db, dres = R.backward(dy.double(), d['x'], y, d['w'], mean, invstd, training, relu, bool(residual))
    ref = dict(y=y, dx=dx, dw=dw, db=db, dres=dres, rm=rm2, rv=rv2)
    # ATen, fp32, CPU
    x = c['x'].clone().requires_grad_(True)
    w, b = c['w'].clone().requires_grad_(True), c['b'].clone().requires_grad_(True)
    res = c['res'].clone().requires_grad_(True) if residual else None
    rm, rv = c['rm'].clone(), c['rv'].clone()
    out = F.batch_norm(x, rm, rv, w, b, training, MOMENTUM, EPS)
    if residual:
        out = out + res
    if relu:
        out = torch.relu(out)
    out.backward(dy)
    aten = dict(y=out.detach(), dx=x.grad, dw=w.grad, db=b.grad, dres=res.grad if residual else None, rm=rm, rv=rv)
    return dy, ref, aten


def run_op(c, dy, relu, residual, training, x_dev=None, needs=(True, True, True, True)):
    """The op on the GPU -> dict of outputs (device tensors)."""
    ops = _ops()
    dev = torch.device('cuda:0')
    x = (c['x'].to(dev) if x_dev is None else x_dev).requires_grad_(needs[0])
    w, b = c['w'].to(dev).requires_grad_(needs[1]), c['b'].to(dev).requires_grad_(needs[2])
    res = c['res'].to(dev).requires_grad_(needs[3]) if residual else None
    rm, rv, nbt = c['rm'].to(dev), c['rv'].to(dev), torch.zeros((), dtype=torch.int64, device=dev)
    y = ops.BatchNormActFunction.apply(x, w, b, rm, rv, nbt, res, training, MOMENTUM, EPS, relu)
    y.backward(dy.to(dev))
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, db=b.grad, dres=res.grad if residual else None, rm=rm, rv=rv, nbt=nbt)


def check(got, ref, aten, training):
    for k in ('y', 'dx', 'dw', 'db', 'dres', 'rm', 'rv'):
        if ref[k] is None:
            assert got[k] is None, k
            continue
        hold(k, got[k], ref[k], aten[k])
    assert int(got['nbt']) == int(training)


def _shapes():
    # around VPN_BN_ONE_PASS_MAX = 8192; test_threshold_shapes_straddle_the_constant holds them to the header's value
    return [(2, 3, 5, 7),        # odd H W: element path
            (3, 64, 4, 4),       # N = 48 < one wave
            (2, 8, 64, 64),      # N = 8192: vector path, the largest one-launch slab
            (5, 6, 33, 31),      # ragged, B not a power of two
            (2, 5, 16, 16),      # N = 512: the largest slab one wave owns
            (1, 4, 19, 27),      # N = 513: the smallest a whole workgroup owns
            (1, 3, 90, 91),      # N = 8190, just below the threshold, H W no multiple of 4
            (2, 3, 64, 65),      # N = 8320, just above: two launches, vector path, a short last slice
            (3, 2, 53, 53)]      # N = 8427, above, odd H W: two launches, element path


COMBOS = [(1, 0), (1, 1), (0, 0), (0, 1)]


def test_threshold_shapes_straddle_the_constant():
    m = _one_pass_max()
    assert _ops().TRUNKNORM_ONE_PASS_MAX == m
    n = [s[0] * s[2] * s[3] for s in _shapes()]
    assert max(v for v in n if v <= m) == m and m - 2 in n and min(v for v in n if v > m) <= m + 128 and sum(v > m for v in n) >= 2


@pytest.mark.parametrize('relu,residual', COMBOS)
@pytest.mark.parametrize('shape', _shapes())
def test_training_forward_backward(shape, relu, residual):
    dy, ref, aten = expected(shape, 'normal', relu, residual, True)
    check(run_op(inputs(shape), dy, relu, residual, True), ref, aten, True)


@pytest.mark.parametrize('relu,residual', COMBOS)
def test_cancellation_case(relu, residual):
    """x ~ 10 + 0.05 randn: a sum-of-squares variance has no correct digit left here."""
    shape = (2, 8, 64, 64)
    dy, ref, aten = expected(shape, 'shifted', relu, residual, True)
    check(run_op(inputs(shape, 'shifted'), dy, relu, residual, True), ref, aten, True)


@pytest.mark.parametrize('relu,residual', [(1, 1), (0, 0)])
@pytest.mark.parametrize('shape', [(2, 8, 64, 64), (2, 3, 64, 66)])
def test_misaligned_view_and_channels_last(shape, relu, residual):
    dev = torch.device('cuda:0')
    dy, ref, aten = expected(shape, 'normal', relu, residual, True)
    c = inputs(shape)
    flat = torch.empty(c['x'].numel() + 1, device=dev)
    view = flat[1:].view(shape)                       # storage offset 1: 4 bytes past a 16-byte boundary
    view.copy_(c['x'])
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    check(run_op(c, dy, relu, residual, True, x_dev=view.detach()), ref, aten, True)
    cl = c['x'].to(dev).contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    got = run_op(c, dy, relu, residual, True, x_dev=cl)
    check(got, ref, aten, True)
    assert got['dx'].shape == cl.shape


@pytest.mark.parametrize('shape', [(5, 6, 33, 31), (2, 8, 64, 64), (2, 3, 64, 65)])
def test_three_steps_then_eval(shape):
    """Three training steps through nn.BatchNorm2d on the CPU against the op on the GPU, then eval mode both ways.  The
    shapes have thousands of elements: a tensor of a few hundred cannot leave out one element within the 0.1 % share."""
    import vpn_amd
    dev = torch.device('cuda:0')
    C = shape[1]
    c = inputs(shape)
    bn32, bn64, bng = nn.BatchNorm2d(C), nn.BatchNorm2d(C).double(), nn.BatchNorm2d(C).to(dev)
    for bn in (bn32, bn64, bng):
        with torch.no_grad():
            bn.weight.copy_(c['w'])
            bn.bias.copy_(c['b'])
    g = torch.Generator().manual_seed(5)
    for step in range(3):
        x = torch.randn(shape, generator=g) * (1 + step) + step
        y32, y64 = bn32(x).detach(), bn64(x.double()).detach()
        if step == 1:
            with torch.no_grad():                     # the no-grad path: the statistics are still updated
                y = vpn_amd.batch_norm_act(x.to(dev), bng, relu=False)
            assert not y.requires_grad
            hold('no_grad y', y, y64, y32)
        else:
            y = vpn_amd.batch_norm_act(x.to(dev), bng, relu=True)
            hold('y', y.detach(), torch.relu(y64), torch.relu(y32))
    assert int(bng.num_batches_tracked) == 3 == int(bn32.num_batches_tracked)
    hold('running_mean', bng.running_mean, bn64.running_mean, bn32.running_mean)
    hold('running_var', bng.running_var, bn64.running_var, bn32.running_var)
    # eval mode, all three on the same running statistics (the float64 ones rounded to fp32: one set of inputs)
    rm, rv = bn64.running_mean.float(), bn64.running_var.float()
    for bn in (bn32, bn64, bng):
        with torch.no_grad():
            bn.running_mean.copy_(rm)
            bn.running_var.copy_(rv)
    for bn in (bn32, bn64, bng):
        bn.eval()
    rm0, rv0 = bng.running_mean.clone(), bng.running_var.clone()
    for relu, residual in COMBOS:
        x64 = c['x'].double().requires_grad_(True)
        r64 = c['res'].double().requires_grad_(True)
        pre = bn64(x64) + (r64 if residual else 0)
        near = (pre.detach().abs() < 1e-4) if relu else torch.zeros_like(pre, dtype=torch.bool)
        assert float(near.double().mean()) <= 1e-3
        dy = torch.where(near, torch.zeros_like(c['dy']), c['dy'])
        (torch.relu(pre) if relu else pre).backward(dy.double())
        x32, r32 = c['x'].clone().requires_grad_(True), c['res'].clone().requires_grad_(True)
        o32 = bn32(x32) + (r32 if residual else 0)
        o32 = torch.relu(o32) if relu else o32
        o32.backward(dy)
        xg, rg = c['x'].to(dev).requires_grad_(True), c['res'].to(dev).requires_grad_(True)
        og = vpn_amd.batch_norm_act(xg, bng, residual=rg if residual else None, relu=bool(relu))
        og.backward(dy.to(dev))
        hold('eval y', og.detach(), (torch.relu(pre) if relu else pre).detach(), o32.detach())
        hold('eval dx', xg.grad, x64.grad, x32.grad)
        hold('eval dw', bng.weight.grad, bn64.weight.grad, bn32.weight.grad)
        hold('eval db', bng.bias.grad, bn64.bias.grad, bn32.bias.grad)
        if residual:
            hold('eval dres', rg.grad, r64.grad, r32.grad)
        for bn in (bn32, bn64, bng):
            bn.zero_grad()
    assert int(bng.num_batches_tracked) == 3 and torch.equal(bng.running_mean, rm0) and torch.equal(bng.running_var, rv0)


@pytest.mark.parametrize('shape', [(5, 6, 33, 31), (2, 3, 64, 65)])
def test_frozen_affine_and_input_without_grad(shape):
    c = inputs(shape)
    dy = inputs(shape)['dy']
    full = run_op(c, dy, 1, 1, True)
    frozen = run_op(c, dy, 1, 1, True, needs=(True, False, False, True))
    assert frozen['dw'] is None and frozen['db'] is None
    assert torch.equal(frozen['dx'], full['dx']) and torch.equal(frozen['dres'], full['dres'])
    no_dx = run_op(c, dy, 1, 1, True, needs=(False, True, True, False))
    assert no_dx['dx'] is None and no_dx['dres'] is None
    assert torch.equal(no_dx['dw'], full['dw']) and torch.equal(no_dx['db'], full['db'])
    only_res = run_op(c, dy, 0, 1, True, needs=(False, False, False, True))      # no ReLU: the residual's gradient is dy itself
    assert torch.equal(only_res['dres'], dy.to('cuda:0')) and only_res['dx'] is None


@pytest.mark.parametrize('shape', [(3, 64, 4, 4), (2, 8, 64, 64), (3, 2, 53, 53)])
def test_two_identical_calls_are_bit_equal(shape):
    c = inputs(shape)
    a, b = run_op(c, c['dy'], 1, 1, True), run_op(c, c['dy'], 1, 1, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('shape', [(2, 8, 64, 64), (2, 3, 64, 65)])
def test_no_sync_and_graph_replay_equals_eager(shape):
    ops = _ops()
    dev = torch.device('cuda:0')
    c = {k: v.to(dev) for k, v in inputs(shape).items()}
    x, res = c['x'].clone().requires_grad_(True), c['res'].clone().requires_grad_(True)
    w, b = c['w'].clone().requires_grad_(True), c['b'].clone().requires_grad_(True)

    def step(rm, rv, nbt):
        # only detached results leave (a kept autograd graph would tie the leaves' accumulators to the stream they were made on)
        y = ops.BatchNormActFunction.apply(x, w, b, rm, rv, nbt, res, True, MOMENTUM, EPS, True)
        return (y.detach(),) + torch.autograd.grad((y * c['dy']).sum(), [x, w, b, res])

    def buffers():
        return c['rm'].clone(), c['rv'].clone(), torch.zeros((), dtype=torch.int64, device=dev)

    step(*buffers())
    eb = buffers()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        eager = step(*eb)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for _ in range(2):
        eager = step(*eb)
    gb = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*gb)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(*gb)
    for t, t0 in zip(gb, buffers()):                 # the warm-up step is undone: the replays start where the eager steps did
        t.copy_(t0)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(gb[2]) == 3 == int(eb[2])
    assert torch.equal(gb[0], eb[0]) and torch.equal(gb[1], eb[1])
    for p, q in zip(captured, eager):
        assert torch.equal(p, q)


def test_whole_trunk_against_the_float64_cpu_trunk():
    """ResNet18(fused_norm=True) on the GPU, training mode, B = 4 at 64 x 64 (layer4 is 2 x 2: N = 16): the four maps and
    every parameter gradient against the float64 CPU trunk, ATen's fp32 CPU trunk as yardstick, margin 8 (20
    normalisations compound, and tiny-N statistics amplify a difference of order).
    Measured on an MI355X: worst ratio e_kernel / max(e_aten, 2^-24) = 2.76, at bn1.running_mean."""
    from vpn_amd.modules.network import ResNet18, _trunk_maps, VPNetOneRes
    dev = torch.device('cuda:0')
    torch.manual_seed(3)
    plain = ResNet18()
    state = {k: v.clone() for k, v in plain.state_dict().items()}
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(4, 3, 64, 64, generator=g)
    ws = [torch.randn(4, ch, 64 // s, 64 // s, generator=g) for ch, s in ((64, 4), (128, 8), (256, 16), (512, 32))]

    def run(model, dtype, device):
        model.load_state_dict(state, strict=True)
        model = model.to(device=device, dtype=dtype).train()
        maps = _trunk_maps(model, imgs.to(device=device, dtype=dtype))
        sum((m * w.to(device=device, dtype=dtype)).sum() for m, w in zip(maps, ws)).backward()
        grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
        return [m.detach() for m in maps], grads, {k: v for k, v in model.state_dict().items() if 'running' in k}

    m64, g64, s64 = run(ResNet18(), torch.float64, 'cpu')
    m32, g32, s32 = run(ResNet18(), torch.float32, 'cpu')
    fused = ResNet18(fused_norm=True)
    mg, gg, sg = run(fused, torch.float32, dev)
    assert set(gg) == set(g64) and len(gg) == 60            # all but fc.weight / fc.bias
    assert all(int(v) == 1 for k, v in fused.state_dict().items() if k.endswith('num_batches_tracked'))
    report = []
    for i in range(4):
        hold('map %d' % i, mg[i], m64[i], m32[i], 8.0, report)
    for k in g64:
        hold(k, gg[k], g64[k], g32[k], 8.0, report)
    for k in s64:
        hold(k, sg[k], s64[k], s32[k], 8.0, report)
    print('worst ratio e_kernel / max(e_aten, 2^-24): %.2f at %s' % max((r, n) for n, r in report))
    # the model takes the fused trunk through its trunk= argument
    net = VPNetOneRes(vp_num=4, is_dropout=False, trunk=fused).to(dev).train()
    params, maps, feats = net.forward_packed(imgs.to(dev))
    assert params.shape == (4, 4, 10) and len(maps) == 4
    params.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in net.resnet.parameters() if p.grad is not None)
    assert net.resnet.conv1.weight.grad is not None
