"""GPU tests of the stem's pool op (the tp_ kernels of csrc/trunknorm.hip, ops.BatchNormPoolFunction, ResNet18(fused_pool);
DESIGN.md 4.21).

Forward: bit for bit the composition it replaces, F.max_pool2d(batch_norm_act(x, relu=True), 3, 2, 1) on the GPU, indices and
every statistic included.  Backward: the float64 restatement tests/trunkpool_ref.py on the CPU as reference and ATen's own
fp32 CPU composition as yardstick, with the helper and the margin 4 of tests/test_trunknorm.py: for dx, d_weight, d_bias
e_kernel(T) <= max(4 e_aten(T), 4 * 2^-24).  A window whose float64 top two pre-activations lie within 1e-4 of each other
while the maximum is positive, or whose float64 maximum lies within 1e-4 of zero, is left out (a rounding may move its
routing or its mask): its dp is zero for the op, the yardstick and the reference alike; the share of such windows is
asserted <= 0.1 %, and everywhere else idx is compared exactly."""
import functools

import pytest
import torch
import torch.nn.functional as F

import trunkpool_ref as R
from test_trunknorm import EPS, MOMENTUM, hold, inputs

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 5, 7),        # odd sizes, element path, windows cut at both borders
          (3, 64, 4, 4),       # N below a wave
          (2, 4, 8, 8),        # vector path
          (2, 5, 16, 16),      # N = 512: the largest slab one wave owns
          (1, 4, 19, 27),      # N = 513
          (2, 2, 64, 64),      # N = 8192: the largest one-launch slab
          (1, 3, 90, 91),      # N = 8190, just below
          (2, 3, 64, 65),      # N = 8320, just above: two launches, a short last slice
          (3, 2, 53, 53),      # N = 8427, odd H W
          (3, 2, 40, 40),      # batch rows crossing slices, windows straddling slice ends
          (2, 64, 32, 32),     # the stem's channel count
          (2, 2, 2, 3)]        # PH = 1
TIES = [(2, 3, 12, 14), (2, 2, 80, 72)]      # one launch, elements; two launches, 16-byte accesses


def _ops():
    from vpn_amd import ops
    return ops


def _dev():
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def case(shape, ties=False):
    """The inputs of tests/test_trunknorm.py (seed 11, kind normal) and dp on the pooled shape; never written to.  ties: x is
    a half-size map with every pixel repeated 2 x 2, so that every window holds equal maxima."""
    c = dict(inputs(shape))
    g = torch.Generator().manual_seed(12)
    B, C, H, W = shape
    if ties:
        c['x'] = torch.randn((B, C, H // 2, W // 2), generator=g).repeat_interleave(2, 2).repeat_interleave(2, 3).contiguous()
    c['dp'] = torch.randn((B, C) + R.out_size(H, W), generator=g)
    return c


@functools.lru_cache(maxsize=None)
def expected(shape, training, ties=False):
    """(dp with the left-out windows zeroed, those windows, the float64 reference, ATen's fp32 CPU result)."""
    c = case(shape, ties)
    d = {k: v.double() for k, v in c.items()}
    p, idx, pre, mean, invstd, _rm, _rv, _n = R.forward(d['x'], d['w'], d['b'], d['rm'], d['rv'], torch.tensor(0), training,
                                                        MOMENTUM, EPS)
    t = R.taps(pre)
    top = t.max(dim=-1).values
    # the runner-up; with exact ties the largest value below the maximum (equal taps are routed by position, not by rounding)
    second = torch.where(t == top.unsqueeze(-1), torch.full_like(t, float('-inf')), t).max(dim=-1).values if ties else \
        t.topk(2, dim=-1).values[..., 1]
    near = (((top - second) < 1e-4) & (top > 0)) | (top.abs() < 1e-4)
    share = float(near.double().mean())
    print('left-out windows: %.2e' % share)
    assert share <= 1e-3, share
    dp = torch.where(near, torch.zeros_like(c['dp']), c['dp'])
    dx, dw, db = R.backward(dp.double(), d['x'], p, idx, d['w'], mean, invstd, training)
    ref = dict(p=p, idx=idx, dx=dx, dw=dw, db=db)
    x, w, b = c['x'].clone().requires_grad_(True), c['w'].clone().requires_grad_(True), c['b'].clone().requires_grad_(True)
    out = F.max_pool2d(torch.relu(F.batch_norm(x, c['rm'].clone(), c['rv'].clone(), w, b, training, MOMENTUM, EPS)), 3, 2, 1)
    out.backward(dp)
    return dp, near, ref, dict(p=out.detach(), dx=x.grad, dw=w.grad, db=b.grad)


def run_op(c, dp, training, needs=(True, True, True), x_dev=None):
    """The op on the GPU -> dict of outputs (device tensors); idx and the statistics are the tensors it saved."""
    dev = _dev()
    x = (c['x'].to(dev) if x_dev is None else x_dev).requires_grad_(needs[0])
    w, b = c['w'].to(dev).requires_grad_(needs[1]), c['b'].to(dev).requires_grad_(needs[2])
    rm, rv, nbt = c['rm'].to(dev), c['rv'].to(dev), torch.zeros((), dtype=torch.int64, device=dev)
    p = _ops().BatchNormPoolFunction.apply(x, w, b, rm, rv, nbt, training, MOMENTUM, EPS)
    _x, _p, idx, _w, stat_a, stat_b = p.grad_fn.saved_tensors
    p.backward(dp.to(dev))
    return dict(p=p.detach(), idx=idx, stat_a=stat_a, stat_b=stat_b, dx=x.grad, dw=w.grad, db=b.grad, rm=rm, rv=rv, nbt=nbt)


def run_composition(c, training, x_dev=None):
    """F.max_pool2d(batch_norm_act(x, relu=True), 3, 2, 1) on the GPU: what the op replaces."""
    dev = _dev()
    x = (c['x'].to(dev) if x_dev is None else x_dev).requires_grad_(True)
    rm, rv, nbt = c['rm'].to(dev), c['rv'].to(dev), torch.zeros((), dtype=torch.int64, device=dev)
    y = _ops().BatchNormActFunction.apply(x, c['w'].to(dev), c['b'].to(dev), rm, rv, nbt, None, training, MOMENTUM, EPS, True)
    _x, _y, _w, stat_a, stat_b = y.grad_fn.saved_tensors
    p, flat = F.max_pool2d(y.detach(), 3, 2, 1, return_indices=True)
    return dict(p=p, idx=R.taps_from_flat(flat.cpu(), x.shape[2], x.shape[3]), stat_a=stat_a, stat_b=stat_b, rm=rm, rv=rv, nbt=nbt)


def assert_forward_equal(got, comp):
    assert torch.equal(got['p'], comp['p'])
    assert got['idx'].dtype == torch.uint8 and torch.equal(got['idx'].cpu(), comp['idx'])
    for k in ('stat_a', 'stat_b', 'rm', 'rv', 'nbt'):
        assert torch.equal(got[k], comp[k]), k


def check_backward(got, near, ref, aten):
    keep = ~near
    assert torch.equal(got['idx'].cpu()[keep], ref['idx'][keep])
    for k in ('dx', 'dw', 'db'):
        hold(k, got[k], ref[k], aten[k])


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_forward_is_the_composition_bit_for_bit(shape, training):
    c = case(shape)
    got, comp = run_op(c, c['dp'], training), run_composition(c, training)
    assert_forward_equal(got, comp)
    assert int(got['nbt']) == int(training) and got['p'].shape[2:] == _ops().pool_out_size(*shape[2:])


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('shape', [(2, 4, 8, 8), (5, 2, 44, 48)])
def test_misaligned_view_and_channels_last(shape, training):
    dev = _dev()
    c = case(shape)
    flat = torch.empty(c['x'].numel() + 1, device=dev)
    view = flat[1:].view(shape)                       # storage offset 1: 4 bytes past a 16-byte boundary
    view.copy_(c['x'])
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert_forward_equal(run_op(c, c['dp'], training, x_dev=view.detach()), run_composition(c, training, x_dev=view.detach()))
    dp, near, ref, aten = expected(shape, training)
    check_backward(run_op(c, dp, training, x_dev=view.detach()), near, ref, aten)
    cl = c['x'].to(dev).contiguous(memory_format=torch.channels_last)
    got = run_op(c, dp, training, x_dev=cl)
    check_backward(got, near, ref, aten)
    assert got['dx'].shape == cl.shape


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('shape', TIES)
def test_exact_ties(shape, training):
    c = case(shape, True)
    dp, near, ref, aten = expected(shape, training, True)
    got = run_op(c, dp, training)
    assert_forward_equal(got, run_composition(c, training))
    tied = R.taps(torch.relu(c['x']))
    # a window holds four half-size pixels on 1, 2, 2 and 4 taps (fewer at the borders): unless the single tap wins, it ties
    assert float(((tied == tied.max(dim=-1, keepdim=True).values).sum(-1) > 1).double().mean()) > 0.7
    check_backward(got, near, ref, aten)


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_backward_against_the_restatement(shape, training):
    dp, near, ref, aten = expected(shape, training)
    got = run_op(case(shape), dp, training)
    hold('p', got['p'], ref['p'], aten['p'])
    check_backward(got, near, ref, aten)


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('shape', [(1, 4, 19, 27), (2, 3, 64, 65), (2, 2, 64, 64)])
def test_frozen_affine_and_input_without_grad(shape, training):
    c = case(shape)
    full = run_op(c, c['dp'], training)
    frozen = run_op(c, c['dp'], training, needs=(True, False, False))
    assert frozen['dw'] is None and frozen['db'] is None and torch.equal(frozen['dx'], full['dx'])
    no_dx = run_op(c, c['dp'], training, needs=(False, True, True))
    assert no_dx['dx'] is None and torch.equal(no_dx['dw'], full['dw']) and torch.equal(no_dx['db'], full['db'])
    only_b = run_op(c, c['dp'], training, needs=(False, False, True))
    assert only_b['dx'] is None and only_b['dw'] is None and torch.equal(only_b['db'], full['db'])


def test_saved_bytes():
    """One training call at (2, 64, 32, 32) keeps x, p (a quarter), idx (a sixteenth) and [C] vectors: below 1.5 x the bytes
    of x; the composition keeps x, y and the pool's int64 indices: above 2 x."""
    dev = _dev()
    shape = (2, 64, 32, 32)
    c = case(shape)
    x_bytes = c['x'].numel() * 4

    def saved(fn):
        seen = {}

        def pack(t):
            seen[(t.data_ptr(), t.numel(), t.dtype)] = t.numel() * t.element_size()
            return t
        x = c['x'].to(dev).requires_grad_(True)
        w, b = c['w'].to(dev).requires_grad_(True), c['b'].to(dev).requires_grad_(True)
        rm, rv, nbt = c['rm'].to(dev), c['rv'].to(dev), torch.zeros((), dtype=torch.int64, device=dev)
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = fn(x, w, b, rm, rv, nbt)
        return sum(seen.values()), out

    fused, _ = saved(lambda x, w, b, rm, rv, nbt: _ops().BatchNormPoolFunction.apply(x, w, b, rm, rv, nbt, True, MOMENTUM, EPS))
    comp, _ = saved(lambda x, w, b, rm, rv, nbt: F.max_pool2d(
        _ops().BatchNormActFunction.apply(x, w, b, rm, rv, nbt, None, True, MOMENTUM, EPS, True), 3, 2, 1))
    print('saved bytes / bytes of x: fused %.3f, composition %.3f' % (fused / x_bytes, comp / x_bytes))
    assert fused < 1.5 * x_bytes and comp > 2 * x_bytes


@pytest.mark.parametrize('shape', [(3, 64, 4, 4), (2, 2, 64, 64), (3, 2, 53, 53)])
def test_two_identical_calls_are_bit_equal(shape):
    c = case(shape)
    a, b = run_op(c, c['dp'], True), run_op(c, c['dp'], True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('shape', [(2, 2, 64, 64), (2, 3, 64, 65)])
def test_no_sync_and_graph_replay_equals_eager(shape):
    ops = _ops()
    dev = _dev()
    c = {k: v.to(dev) for k, v in case(shape).items()}
    x = c['x'].clone().requires_grad_(True)
    w, b = c['w'].clone().requires_grad_(True), c['b'].clone().requires_grad_(True)

    def step(rm, rv, nbt):
        # only detached results leave (a kept autograd graph would tie the leaves' accumulators to the stream they were made on)
        p = ops.BatchNormPoolFunction.apply(x, w, b, rm, rv, nbt, True, MOMENTUM, EPS)
        return (p.detach(),) + torch.autograd.grad((p * c['dp']).sum(), [x, w, b])

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


def test_functional_form_reads_the_module():
    import vpn_amd
    dev = _dev()
    c = case((2, 3, 64, 65))
    bn1, bn2 = torch.nn.BatchNorm2d(3).to(dev), torch.nn.BatchNorm2d(3).to(dev)
    x = c['x'].to(dev)
    for mode in ('train', 'eval'):
        getattr(bn1, mode)()
        getattr(bn2, mode)()
        assert torch.equal(vpn_amd.batch_norm_relu_pool(x, bn1), F.max_pool2d(vpn_amd.batch_norm_act(x, bn2, relu=True), 3, 2, 1))
    assert int(bn1.num_batches_tracked) == 1 and torch.equal(bn1.running_var, bn2.running_var)


def test_whole_trunk_with_and_without_the_fused_pool():
    """ResNet18(fused_norm=True, fused_pool=True) against ResNet18(fused_norm=True) from one state_dict, training, B = 4 at
    64 x 64: the four maps and every gradient bit-equal but conv1.weight, bn1.weight, bn1.bias (the stem's g is summed in
    another order than ATen's pool backward sums it); those three against the float64 CPU trunk with ATen's fp32 CPU trunk
    as yardstick, margin 8 as in test_whole_trunk_against_the_float64_cpu_trunk.  Both trunks run their convolutions on
    csrc/trunkconv.hip and csrc/trunkstride.hip, which are bit-equal from run to run: with the library's convolutions two
    runs of the SAME trunk already differ from layer2 on, so bit equality would say nothing about the pool.
    Measured on an MI355X: worst ratio e_kernel / max(e_aten, 2^-24) = 9.3e-4, at bn1.weight."""
    from vpn_amd.modules.network import ResNet18, _trunk_maps
    dev = _dev()
    torch.manual_seed(3)
    state = {k: v.clone() for k, v in ResNet18().state_dict().items()}
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(4, 3, 64, 64, generator=g)
    ws = [torch.randn(4, ch, 64 // s, 64 // s, generator=g) for ch, s in ((64, 4), (128, 8), (256, 16), (512, 32))]

    def run(model, dtype, device):
        model.load_state_dict(state, strict=True)
        model = model.to(device=device, dtype=dtype).train()
        maps = _trunk_maps(model, imgs.to(device=device, dtype=dtype))
        sum((m * w.to(device=device, dtype=dtype)).sum() for m, w in zip(maps, ws)).backward()
        return ([m.detach() for m in maps], {k: p.grad for k, p in model.named_parameters() if p.grad is not None},
                {k: v for k, v in model.state_dict().items() if 'running' in k or 'tracked' in k})

    conv = dict(hip_conv=True, hip_conv_strided=True)
    mp, gp, sp = run(ResNet18(fused_norm=True, fused_pool=True, **conv), torch.float32, dev)
    mn, gn, sn = run(ResNet18(fused_norm=True, **conv), torch.float32, dev)
    stem = ('conv1.weight', 'bn1.weight', 'bn1.bias')
    assert all(torch.equal(a, b) for a, b in zip(mp, mn)) and set(gp) == set(gn) and len(gp) == 60
    assert all(torch.equal(sp[k], sn[k]) for k in sn)
    for k in gn:
        if k not in stem:
            assert torch.equal(gp[k], gn[k]), k
    _m64, g64, _s64 = run(ResNet18(), torch.float64, 'cpu')
    _m32, g32, _s32 = run(ResNet18(), torch.float32, 'cpu')
    report = []
    for k in stem:
        hold(k, gp[k], g64[k], g32[k], 8.0, report)
    print('worst ratio e_kernel / max(e_aten, 2^-24): %.2e at %s' % max((r, n) for n, r in report))
