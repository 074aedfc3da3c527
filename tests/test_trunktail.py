"""GPU tests of the trunk's tail (the tt_ kernels of csrc/trunknorm.hip, ops.BatchNormMeanFunction, ResNet18(fused_tail);
DESIGN.md 4.22): the last norm / add / ReLU site that also writes the global average pool m and takes m's gradient.

y, the saved and the running statistics and the counter must equal BatchNormActFunction's bit for bit.  m and the
gradients are held as tests/test_trunknorm.py holds its outputs: reference the float64 restatement tests/trunktail_ref.py
on the CPU, yardstick ATen's own fp32 CPU composition (batch_norm, add, ReLU, mean((2, 3))) on the same inputs,
e_kernel <= max(4 e_aten, 4 * 2^-24).  Where ReLU is on, elements whose float64 pre-activation lies within 1e-4 of zero are
left out: their dy is set to -fl32(dm[b,c] / HW), so that their upstream gradient is zero for the op, the yardstick and the
reference alike; their share is asserted <= 0.1 %."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import trunknorm_ref as N
import trunktail_ref as R
from test_trunknorm import inputs, hold, MOMENTUM, EPS, COMBOS

pytestmark = pytest.mark.gpu

SHAPES = [(8, 512, 4, 4),      # the real site
          (3, 64, 4, 4),       # N below a wave
          (2, 3, 5, 7),        # odd sizes, element path
          (2, 5, 16, 16),      # N = 512, the largest one-wave slab
          (1, 4, 19, 27),      # N = 513, B = 1
          (2, 8, 64, 64),      # N = 8192, rows of 4096
          (5, 6, 33, 31),      # ragged
          (1, 3, 90, 91),      # N = 8190
          (2, 3, 64, 65),      # two launches, vector path
          (3, 2, 53, 53),      # two launches, rows longer than a slice
          (40, 2, 15, 15),     # two launches, about nine rows per slice, rows straddling slice ends
          (4, 3, 1, 1)]        # HW = 1


def _ops():
    from vpn_amd import ops
    return ops


def _dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def case(shape):
    """test_trunknorm.inputs(shape) plus dm [B,C] from a generator of its own; shared and never written to."""
    c = dict(inputs(shape))
    c['dm'] = torch.randn(shape[:2], generator=torch.Generator().manual_seed(12))
    return c


@functools.lru_cache(maxsize=None)
def expected(shape, relu, residual, training):
    """(the dy actually sent back, the float64 reference, ATen's fp32 CPU result), the last two dicts of outputs."""
    c = case(shape)
    d = {k: v.double() for k, v in c.items()}
    HW = shape[2] * shape[3]
    y, m, pre, mean, invstd, rm2, rv2, _n = R.forward(d['x'], d['w'], d['b'], d['rm'], d['rv'], torch.tensor(0),
                                                      d['res'] if residual else None, training, MOMENTUM, EPS, relu)
    dy = c['dy']
    up = R.upstream(dy.double(), d['dm'], shape)
    if relu:
        near = pre.abs() < 1e-4
        share = float(near.double().mean())
        assert share <= 1e-3, share
        q = (c['dm'] / HW)[:, :, None, None].expand(shape)              # fl32(dm / HW), the op's and ATen's own term
        dy = torch.where(near, -q, dy)
        up = torch.where(near, torch.zeros_like(up), up)
    dx, dw, db, dres = N.backward(up, d['x'], y, d['w'], mean, invstd, training, relu, bool(residual))
    ref = dict(y=y, m=m, dx=dx, dw=dw, db=db, dres=dres, rm=rm2, rv=rv2)
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
    avg = out.mean((2, 3))
    torch.autograd.backward([out, avg], [dy, c['dm']])
    aten = dict(y=out.detach(), m=avg.detach(), dx=x.grad, dw=w.grad, db=b.grad, dres=res.grad if residual else None, rm=rm, rv=rv)
    return dy, ref, aten


def run_op(c, dy, dm, relu, residual, training, x_dev=None, needs=(True, True, True, True), tail=True):
    """The op on the GPU -> dict of outputs (device tensors).  dy or dm None: that output takes no part in the backward.
    tail=False: BatchNormActFunction on the same inputs (dm is then not used)."""
    ops = _ops()
    dev = _dev()
    x = (c['x'].to(dev) if x_dev is None else x_dev).requires_grad_(needs[0])
    w, b = c['w'].to(dev).requires_grad_(needs[1]), c['b'].to(dev).requires_grad_(needs[2])
    res = c['res'].to(dev).requires_grad_(needs[3]) if residual else None
    rm, rv, nbt = c['rm'].to(dev), c['rv'].to(dev), torch.zeros((), dtype=torch.int64, device=dev)
    if tail:
        y, m = ops.BatchNormMeanFunction.apply(x, w, b, rm, rv, nbt, res, training, MOMENTUM, EPS, relu)
        outs = [(t, g.to(dev)) for t, g in ((y, dy), (m, dm)) if g is not None]
    else:
        y, m = ops.BatchNormActFunction.apply(x, w, b, rm, rv, nbt, res, training, MOMENTUM, EPS, relu), None
        outs = [(y, dy.to(dev))]
    saved = [t for t in y.grad_fn.saved_tensors[-2:]] if y.grad_fn is not None else None
    torch.autograd.backward([t for t, _ in outs], [g for _, g in outs])
    return dict(y=y.detach(), m=None if m is None else m.detach(), dx=x.grad, dw=w.grad, db=b.grad,
                dres=res.grad if residual else None, rm=rm, rv=rv, nbt=nbt, saved=saved)


GRADS = ('dx', 'dw', 'db', 'dres')


def same(a, b, keys):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('relu,residual', COMBOS)
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_forward_and_backward_with_both_gradients(shape, training, relu, residual):
    dy, ref, aten = expected(shape, relu, residual, training)
    c = case(shape)
    got = run_op(c, dy, c['dm'], relu, residual, training)
    act = run_op(c, dy, None, relu, residual, training, tail=False)
    same(got, act, ('y', 'rm', 'rv', 'nbt'))                     # what vpn_bn_act_fwd writes, bit for bit
    assert torch.equal(got['saved'][0], act['saved'][0]) and torch.equal(got['saved'][1], act['saved'][1])
    assert int(got['nbt']) == int(training) and got['m'].shape == shape[:2]
    for k in ('m', 'dx', 'dw', 'db', 'dres', 'rm', 'rv'):
        if ref[k] is None:
            assert got[k] is None, k
            continue
        hold(k, got[k], ref[k], aten[k])


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('shape', [(8, 512, 4, 4), (2, 8, 64, 64), (40, 2, 15, 15)])
def test_exact_rows(shape, training):
    """weight = bias = 0 without ReLU and an integer-valued residual in [-8, 8]: y is the residual, every row sum is exact
    in any order, so m is the float64 row sum / HW rounded once.  A wrong row boundary cannot pass."""
    ops = _ops()
    dev = _dev()
    c = case(shape)
    B, C, H, W = shape
    res = torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(13)).float()
    zero = torch.zeros(C, device=dev)
    y, m = ops.BatchNormMeanFunction.apply(c['x'].to(dev), zero, zero, c['rm'].to(dev), c['rv'].to(dev), None, res.to(dev), training,
                                           MOMENTUM, EPS, False)
    assert torch.equal(y.cpu(), res)
    assert torch.equal(m.cpu(), (res.double().sum((2, 3)) / (H * W)).float())


@pytest.mark.parametrize('relu,residual', COMBOS)
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_one_gradient_alone(shape, training, relu, residual):
    """No gradient for m: BatchNormActFunction's backward bit for bit.  No gradient for y: the call with dy = zeros."""
    c = case(shape)
    only_y = run_op(c, c['dy'], None, relu, residual, training)
    act = run_op(c, c['dy'], None, relu, residual, training, tail=False)
    same(only_y, act, GRADS)
    only_m = run_op(c, None, c['dm'], relu, residual, training)
    zeros = run_op(c, torch.zeros(shape), c['dm'], relu, residual, training)
    same(only_m, zeros, GRADS)
    assert only_m['dx'] is not None and (only_m['dx'].numel() < 100 or bool(only_m['dx'].abs().max() > 0))


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('shape', [(8, 512, 4, 4), (5, 6, 33, 31), (2, 3, 64, 65)])
def test_frozen_affine_and_inputs_without_grad(shape, training):
    c = case(shape)
    dy, dm = c['dy'], c['dm']
    full = run_op(c, dy, dm, 1, 1, training)
    frozen = run_op(c, dy, dm, 1, 1, training, needs=(True, False, False, True))
    assert frozen['dw'] is None and frozen['db'] is None
    same(frozen, full, ('dx', 'dres'))
    no_dx = run_op(c, dy, dm, 1, 1, training, needs=(False, True, True, False))
    assert no_dx['dx'] is None and no_dx['dres'] is None
    same(no_dx, full, ('dw', 'db'))
    no_res = run_op(c, dy, dm, 1, 1, training, needs=(True, True, True, False))
    assert no_res['dres'] is None
    same(no_res, full, ('dx', 'dw', 'db'))
    only_res = run_op(c, dy, dm, 0, 1, training, needs=(False, False, False, True))      # no ReLU: d_residual is the upstream gradient
    HW = shape[2] * shape[3]
    assert only_res['dx'] is None and torch.equal(only_res['dres'].cpu(), dy + (dm / HW)[:, :, None, None])
    only_res_y = run_op(c, dy, None, 0, 1, training, needs=(False, False, False, True))   # ... and dy itself without m's
    assert torch.equal(only_res_y['dres'].cpu(), dy)


@pytest.mark.parametrize('shape', [(8, 512, 4, 4), (2, 8, 64, 64), (3, 2, 53, 53), (40, 2, 15, 15)])
def test_two_identical_calls_are_bit_equal(shape):
    c = case(shape)
    a, b = run_op(c, c['dy'], c['dm'], 1, 1, True), run_op(c, c['dy'], c['dm'], 1, 1, True)
    same(a, b, ('y', 'm', 'rm', 'rv', 'nbt') + GRADS)


@pytest.mark.parametrize('shape', [(2, 8, 64, 64), (2, 3, 64, 65)])
def test_no_sync_and_graph_replay_equals_eager(shape):
    ops = _ops()
    dev = _dev()
    c = {k: v.to(dev) for k, v in case(shape).items()}
    x, res = c['x'].clone().requires_grad_(True), c['res'].clone().requires_grad_(True)
    w, b = c['w'].clone().requires_grad_(True), c['b'].clone().requires_grad_(True)

    def step(rm, rv, nbt):
        # only detached results leave (a kept autograd graph would tie the leaves' accumulators to the stream they were made on)
        y, m = ops.BatchNormMeanFunction.apply(x, w, b, rm, rv, nbt, res, True, MOMENTUM, EPS, True)
        return (y.detach(), m.detach()) + torch.autograd.grad((y * c['dy']).sum() + (m * c['dm']).sum(), [x, w, b, res])

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


@pytest.mark.parametrize('relu,residual', [(1, 1), (0, 0)])
@pytest.mark.parametrize('shape', [(2, 8, 64, 64), (2, 3, 64, 66)])
def test_misaligned_view_and_channels_last(shape, relu, residual):
    dev = _dev()
    dy, ref, aten = expected(shape, relu, residual, True)
    c = case(shape)

    def check(got):
        for k in ('y', 'm', 'dx', 'dw', 'db', 'dres', 'rm', 'rv'):
            if ref[k] is not None:
                hold(k, got[k], ref[k], aten[k])
    flat = torch.empty(c['x'].numel() + 1, device=dev)
    view = flat[1:].view(shape)                       # storage offset 1: 4 bytes past a 16-byte boundary
    view.copy_(c['x'])
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    check(run_op(c, dy, c['dm'], relu, residual, True, x_dev=view.detach()))
    cl = c['x'].to(dev).contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    got = run_op(c, dy, c['dm'], relu, residual, True, x_dev=cl)
    check(got)
    assert got['dx'].shape == cl.shape
    same(got, run_op(c, dy, c['dm'], relu, residual, True), ('y', 'm') + GRADS)      # the same values as from a contiguous x


def test_functional_form_reads_the_module():
    import vpn_amd
    dev = _dev()
    shape = (2, 3, 64, 65)
    c = case(shape)
    bn1, bn2 = nn.BatchNorm2d(3, eps=1e-3, momentum=0.3).to(dev), nn.BatchNorm2d(3, eps=1e-3, momentum=0.3).to(dev)
    x, res = c['x'].to(dev), c['res'].to(dev)
    for mode in ('train', 'eval'):
        getattr(bn1, mode)()
        getattr(bn2, mode)()
        for residual, relu in ((None, True), (res, True), (res, False)):
            y, m = vpn_amd.batch_norm_act_mean(x, bn1, residual=residual, relu=relu)
            y2 = vpn_amd.batch_norm_act(x, bn2, residual=residual, relu=relu)
            assert torch.equal(y, y2) and m.shape == (2, 3)
            y64 = y.detach().double().cpu()
            hold('m', m.detach(), y64.mean((2, 3)), y.detach().cpu().mean((2, 3)))
    assert int(bn1.num_batches_tracked) == 3 == int(bn2.num_batches_tracked)
    assert torch.equal(bn1.running_var, bn2.running_var) and torch.equal(bn1.running_mean, bn2.running_mean)


def test_whole_trunk_with_and_without_the_fused_tail():
    """ResNet18(fused_norm=True, fused_tail=True) against the same trunk without fused_tail, both with their convolutions on
    csrc/trunkconv.hip and csrc/trunkstride.hip (bit-equal from run to run), from one state_dict, training, B = 4 at
    64 x 64; the loss is taken on the four maps and on the features.  The maps and all running statistics are bit-equal;
    the features and every parameter gradient are held against the float64 CPU trunk with ATen's fp32 CPU trunk as
    yardstick, margin 8 as in test_whole_trunk_against_the_float64_cpu_trunk.
    Measured on an MI355X: worst ratio e_kernel / max(e_aten, 2^-24) = 1.00, at layer4.1.bn2.bias."""
    from vpn_amd.modules.network import ResNet18, _trunk_features
    dev = _dev()
    torch.manual_seed(3)
    state = {k: v.clone() for k, v in ResNet18().state_dict().items()}
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(4, 3, 64, 64, generator=g)
    ws = [torch.randn(4, ch, 64 // s, 64 // s, generator=g) for ch, s in ((64, 4), (128, 8), (256, 16), (512, 32))]
    wf = torch.randn(4, 512, generator=g)

    def run(model, dtype, device):
        model.load_state_dict(state, strict=True)
        model = model.to(device=device, dtype=dtype).train()
        maps, feats = _trunk_features(model, imgs.to(device=device, dtype=dtype))
        assert feats.shape == (4, 512)
        loss = sum((m * w.to(device=device, dtype=dtype)).sum() for m, w in zip(maps, ws)) + (feats * wf.to(device=device, dtype=dtype)).sum()
        loss.backward()
        return ([m.detach() for m in maps], feats.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None},
                {k: v for k, v in model.state_dict().items() if 'running' in k or 'tracked' in k})

    conv = dict(hip_conv=True, hip_conv_strided=True)
    tail = ResNet18(fused_norm=True, fused_tail=True, **conv)
    mt, ft, gt, st = run(tail, torch.float32, dev)
    mn, fn, gn, sn = run(ResNet18(fused_norm=True, **conv), torch.float32, dev)
    assert all(torch.equal(a, b) for a, b in zip(mt, mn)) and set(gt) == set(gn) and len(gt) == 60
    assert all(torch.equal(st[k], sn[k]) for k in sn)
    assert all(int(v) == 1 for k, v in tail.state_dict().items() if k.endswith('num_batches_tracked'))
    _m64, f64, g64, _s64 = run(ResNet18(), torch.float64, 'cpu')
    _m32, f32, g32, _s32 = run(ResNet18(), torch.float32, 'cpu')
    report = []
    hold('features', ft, f64, f32, 8.0, report)
    for k in g64:
        hold(k, gt[k], g64[k], g32[k], 8.0, report)
    print('worst ratio e_kernel / max(e_aten, 2^-24): %.2f at %s' % max((r, n) for n, r in report))
    # the classifier's forward takes the same path
    with torch.no_grad():
        tail.eval()
        logits = tail(imgs.to(dev))
    assert logits.shape == (4, 1000) and bool(torch.isfinite(logits).all())


class _PoolThatMustNotRun(nn.AdaptiveAvgPool2d):
    def forward(self, x):
        raise AssertionError('avgpool was called')


def test_models_take_the_features_from_the_trunk():
    from vpn_amd.modules.network import ResNet18, VPNetOneRes, VPNetTwoRes, SDNet
    dev = _dev()
    torch.manual_seed(5)
    imgs = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(6)).to(dev)

    def trunk(tail):
        return ResNet18(fused_norm=True, fused_tail=tail, hip_conv=True, hip_conv_strided=True)

    one = VPNetOneRes(vp_num=4, is_dropout=False, trunk=trunk(True)).to(dev).train()
    ref = VPNetOneRes(vp_num=4, is_dropout=False, trunk=trunk(False)).to(dev).train()
    ref.load_state_dict(one.state_dict(), strict=True)
    one.avgpool = _PoolThatMustNotRun(1)
    one.resnet.avgpool = _PoolThatMustNotRun(1)
    params, maps, feats = one.forward_packed(imgs)
    params_r, maps_r, feats_r = ref.forward_packed(imgs)
    assert feats.shape == (2, 512) and params.shape == (2, 4, 10)
    assert torch.equal(maps[3], maps_r[3]) and all(torch.equal(a, b) for a, b in zip(maps, maps_r))
    hold('features', feats.detach(), maps_r[3].detach().double().cpu().mean((2, 3)), feats_r.detach().cpu())      # yardstick: ATen's pool
    (params.sum() + maps[3].sum()).backward()              # the GCN's case: the map has a gradient of its own
    assert one.resnet.conv1.weight.grad is not None and bool(torch.isfinite(one.resnet.conv1.weight.grad).all())

    two = VPNetTwoRes(vp_num=4, is_dropout=False, trunk=(trunk(True), trunk(True))).to(dev).train()
    two.avgpool = _PoolThatMustNotRun(1)
    out = two.forward_packed(imgs)
    assert out.shape == (2, 4, 10)
    out.sum().backward()                                   # VPNet without the GCN: no gradient reaches the map
    assert all(bool(torch.isfinite(p.grad).all()) for p in two.parameters() if p.grad is not None)
    assert two.volume_resnet.conv1.weight.grad is not None and two.transform_resnet.conv1.weight.grad is not None

    sd = SDNet(vertex_num=12, trunk=trunk(True)).to(dev).train()
    sd._model.avgpool = nn.Sequential(_PoolThatMustNotRun(1))
    off = sd(imgs)
    assert off.shape == (2, 12, 3) and bool(torch.isfinite(off).all())
