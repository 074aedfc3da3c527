"""GPU tests of the trunk's strided convolutions (csrc/trunkstride.hip, ops.Conv2dFunction, vpn_amd.conv2d,
ResNet18(hip_conv_strided)).  Shapes are (B, C_in, C_out, H, W, R, stride, pad).

Reference: the float64 restatement tests/trunkstride_ref.py on the CPU.
  * exact: integer-valued inputs (x in -3..3, w and dy in -2..2): every partial sum is an integer below 2^24 in magnitude
    whatever the order, so y, dx and dw must EQUAL the float64 result.  The output buffers hold NaN before the call: an
    element the kernels forgot to write (the dx of an input pixel that no output reads) is caught;
  * rounded: seeded normal inputs; per element |T - T64| <= 2 K 2^-24 A with A the same product of |x|, |w|, |dy| in
    float64 and K the reduction length (R R C_in, R R C_out, B OH OW): the chain bound DESIGN.md 4.19 derives;
  * the 3x3 / stride 1 / padding 1 case is bit-equal to vpn_amd.conv3x3: the summation order is the documented one;
  * the whole trunk with hip_conv and hip_conv_strided reaches no library convolution, holds the float64 trunk within
    max(8 e_plain, 8 x 2^-24) and repeats bit for bit.
Measured on an MI355X: the worst fraction of the chain bound and the whole-trunk ratio are in DESIGN.md 4.20."""
import functools

import pytest
import torch
import torch.nn.functional as F

import trunkstride_ref as R

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -24

SMALL = [
    (1, 1, 1, 1, 1, 1, 2, 0),          # one pixel
    (1, 1, 1, 1, 1, 3, 2, 1),          # image smaller than the kernel
    (1, 2, 3, 2, 2, 7, 2, 3),          # OH = 1 with most taps in the padding
    (2, 3, 5, 9, 11, 7, 2, 3),         # odd everything
    (2, 5, 7, 6, 5, 3, 2, 1),          # even H, odd W
    (2, 5, 7, 5, 6, 3, 2, 1),          # odd H, even W
    (2, 6, 7, 8, 8, 1, 2, 0),          # last row and column unread, so dx is exactly 0 there
    (1, 3, 64, 16, 16, 7, 2, 3),       # K = 147, nine chunks plus a tail of 3
    (1, 4, 65, 16, 16, 3, 2, 1),       # N = 64 and M = 65, at the tile edges
    (3, 19, 33, 7, 9, 3, 3, 0),        # stride 3
    (2, 5, 7, 5, 3, 3, 1, 1),          # stride 1
    (2, 5, 7, 5, 3, 1, 1, 0),          # stride 1
]


def trunk_sites(B, side):
    """The seven stride-2 convolutions of the ResNet-18 trunk for a side x side image."""
    out = [(B, 3, 64, side, side, 7, 2, 3)]
    for i, c in enumerate((64, 128, 256)):
        s = side // (4 << i)
        out += [(B, c, 2 * c, s, s, 3, 2, 1), (B, c, 2 * c, s, s, 1, 2, 0)]
    return out


SITES = trunk_sites(2, 64)
STEM = (4, 3, 64, 128, 128, 7, 2, 3)          # the real stem: 256 tiles, unsplit
# not in the sites at B = 2: a weight gradient that is unsplit by its tile count (16 x 29) AND walks more than one chunk (K = 18)
WIDE = (2, 37, 1024, 6, 6, 7, 2, 3)
SHAPES = SMALL + SITES + [STEM, WIDE]
_ids = lambda s: '-'.join(map(str, s))          # noqa: E731


def _ops():
    from vpn_amd import ops
    return ops


def _splits(shape):
    ops = _ops()
    return {p: ops.conv2d_splits(*shape, p) for p in (ops.CONV_FWD, ops.CONV_DX, ops.CONV_DW)}


def _mnk(shape, product):
    ops = _ops()
    B, Ci, Co, H, W, k, st, p = shape
    OH, OW = R.out_size(H, W, k, st, p)
    return {ops.CONV_FWD: (Co, B * OH * OW, k * k * Ci), ops.CONV_DX: (Ci, B * H * W, k * k * Co),
            ops.CONV_DW: (Co, k * k * Ci, B * OH * OW)}[product]


def test_shapes_reach_both_regimes_of_every_product():
    """From the host rule (ops.conv2d_splits, held to the library's own vpn_conv2d_splits), not by assumption."""
    import vpn_amd._lib as lib
    ops, L, c = _ops(), lib.lib(), lib.CONSTANTS
    tile, tk, target = c['VPN_CONV_TILE'], c['VPN_CONV_TILE_K'], c['VPN_CONV_SPLIT_TARGET']
    assert len(SITES) == 7 and len(set(SHAPES)) == len(SHAPES) == 21
    for s in SHAPES:
        for p, S in _splits(s).items():
            assert L.vpn_conv2d_splits(*s, p) == S, (s, p)
    for p in (ops.CONV_FWD, ops.CONV_DX, ops.CONV_DW):
        got = {_splits(s)[p] for s in SHAPES}
        assert 1 in got and max(got) == c['VPN_CONV_MAX_SPLIT'], (p, got)

        def tiles_k(s):
            M, N, K = _mnk(s, p)
            return -(-M // tile) * -(-N // tile), K
        # unsplit because there are tiles enough, not only because K is one chunk; split with more than one tile as well
        assert any(tiles_k(s)[0] >= target and tiles_k(s)[1] > tk and _splits(s)[p] == 1 for s in SHAPES), p
        assert any(tiles_k(s)[0] > 1 and _splits(s)[p] > 1 for s in SHAPES), p
    assert _splits(STEM)[ops.CONV_FWD] == 1 and -(-_mnk(STEM, ops.CONV_FWD)[1] // tile) == 256
    # every kernel size is reached in both regimes
    for k in (1, 3, 7):
        got = {S for s in SHAPES if s[5] == k for S in _splits(s).values()}
        assert 1 in got and max(got) > 1, (k, got)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """Seeded inputs on the CPU with the float64 results, shared by every test of a shape and never written to."""
    B, Ci, Co, H, W, k, st, p = shape
    OH, OW = R.out_size(H, W, k, st, p)
    g = torch.Generator().manual_seed(13)
    if kind == 'int':
        x = torch.randint(-3, 4, (B, Ci, H, W), generator=g).float()
        w = torch.randint(-2, 3, (Co, Ci, k, k), generator=g).float()
        dy = torch.randint(-2, 3, (B, Co, OH, OW), generator=g).float()
    else:
        x, w, dy = torch.randn(B, Ci, H, W, generator=g), torch.randn(Co, Ci, k, k, generator=g), torch.randn(B, Co, OH, OW, generator=g)
    y64 = R.forward(x, w, st, p)
    dx64, dw64 = R.backward(dy, x, w, st, p)
    return dict(x=x, w=w, dy=dy, y=y64, dx=dx64, dw=dw64, stride=st, pad=p)


def run_op(c, x_dev=None, w_dev=None, needs=(True, True)):
    """The op on the GPU -> (y, dx, dw), device tensors; a gradient that was not asked for is None."""
    ops = _ops()
    dev = torch.device('cuda:0')
    x = (c['x'].to(dev) if x_dev is None else x_dev).requires_grad_(needs[0])
    w = (c['w'].to(dev) if w_dev is None else w_dev).requires_grad_(needs[1])
    y = ops.Conv2dFunction.apply(x, w, c['stride'], c['pad'])
    if any(needs):
        y.backward(c['dy'].to(dev))
    return y.detach(), x.grad, w.grad


def run_entries(c, shape, want=(True, True)):
    """The two C entries on buffers that hold NaN before the call -> (y, dx, dw); a gradient that is not wanted is passed as
    NULL and its NaN-filled buffer is returned as it was left."""
    from vpn_amd import _lib
    ops = _ops()
    dev = torch.device('cuda:0')
    x, w, dy = c['x'].to(dev), c['w'].to(dev), c['dy'].to(dev)
    y, dx, dw = (torch.full(t.shape, float('nan'), device=dev) for t in (c['y'], c['dx'], c['dw']))
    ws, nbytes = ops._conv2d_ws(shape, ops.CONV_FWD, dev)
    _lib.call('vpn_conv2d_fwd', x, w, y, *shape, ws, nbytes, _lib.stream())
    products = (ops.CONV_DX if want[0] else 0) | (ops.CONV_DW if want[1] else 0)
    ws, nbytes = ops._conv2d_ws(shape, products, dev)          # sized for the wanted products alone
    _lib.call('vpn_conv2d_bwd', dy, x, w, dx if want[0] else None, dw if want[1] else None, *shape, ws, nbytes, _lib.stream())
    return y, dx, dw


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_exact_on_integer_inputs(shape):
    c = case(shape, 'int')
    assert 3 * 2 * max(_mnk(shape, p)[2] for p in (1, 2, 4)) < 2 ** 24        # every partial sum, in any order, is an exact integer
    for got3 in (run_entries(c, shape), run_op(c)):
        for name, got in zip(('y', 'dx', 'dw'), got3):
            assert got.shape == c[name].shape and got.dtype == torch.float32
            bad = int((~(got.double().cpu() == c[name])).sum())          # a NaN left behind is counted
            assert bad == 0, (name, bad, float((got.double().cpu() - c[name]).abs().max()))
    B, Ci, Co, H, W, k, st, p = shape
    if (k, st, p) == (1, 2, 0) and H % 2 == 0 and H > 1:          # the unread last row and column: written, and as +0.0
        dx = run_entries(c, shape)[1]
        assert int(dx[:, :, H - 1, :].ne(0).sum()) == 0 and int(dx[:, :, :, W - 1].ne(0).sum()) == 0
        assert not bool(torch.signbit(dx[:, :, H - 1, :]).any())


_FRACTIONS = []


def _e(t, t64):
    return float((t.double().cpu() - t64).abs().max() / t64.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_rounded_within_the_fma_chain_bound(shape):
    c = case(shape, 'normal')
    st, p = c['stride'], c['pad']
    A = dict(y=R.forward(c['x'].abs(), c['w'].abs(), st, p))
    A['dx'], A['dw'] = R.backward(c['dy'].abs(), c['x'].abs(), c['w'].abs(), st, p)
    K = dict(y=_mnk(shape, 1)[2], dx=_mnk(shape, 2)[2], dw=_mnk(shape, 4)[2])
    y, dx, dw = run_op(c)
    for name, got in (('y', y), ('dx', dx), ('dw', dw)):
        err = (got.double().cpu() - c[name]).abs()
        bound = 2.0 * K[name] * FLOOR * A[name]
        # where A is 0 (an input pixel that no output reads) the result must be exactly 0
        worst = float((err / bound.clamp_min(1e-300)).max())
        print('%-2s K %6d  e_op %.3e  worst |T - T64| / bound %.4f' % (name, K[name], _e(got, c[name]), worst))
        _FRACTIONS.append((worst, name, shape))
        assert bool((err <= bound).all()), (name, worst)


def test_report_the_worst_fraction_of_the_bound():
    """Printed for DESIGN.md 4.20, not asserted here (every case above asserts its own)."""
    if _FRACTIONS:
        print('worst |T - T64| / (2 K 2^-24 A): %.4f for %s at %s' % max(_FRACTIONS))


@pytest.mark.parametrize('shape', [(2, 5, 7, 5, 3), (2, 64, 64, 16, 16), (1, 2, 2, 128, 128), (1, 114, 1024, 3, 6)], ids=_ids)
def test_bit_equal_to_conv3x3_at_stride_1_padding_1(shape):
    """conv2d(x, w, 1, 1) with a 3x3 weight against conv3x3(x, w): one split and one unsplit shape per product."""
    import vpn_amd
    ops = _ops()
    dev = torch.device('cuda:0')
    B, Ci, Co, H, W = shape
    g = torch.Generator().manual_seed(17)
    x0, w0, dy = torch.randn(B, Ci, H, W, generator=g).to(dev), torch.randn(Co, Ci, 3, 3, generator=g).to(dev), torch.randn(B, Co, H, W, generator=g).to(dev)
    out = []
    for f in (lambda x, w: vpn_amd.conv2d(x, w, 1, 1), vpn_amd.conv3x3):
        x, w = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        y = f(x, w)
        y.backward(dy)
        out.append((y.detach(), x.grad, w.grad))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    for p in (ops.CONV_FWD, ops.CONV_DX, ops.CONV_DW):
        assert ops.conv2d_splits(*shape, 3, 1, 1, p) == ops.conv3x3_splits(*shape, p)


def test_the_bit_equal_shapes_cover_both_regimes_of_every_product():
    ops = _ops()
    shapes = [(2, 5, 7, 5, 3), (2, 64, 64, 16, 16), (1, 2, 2, 128, 128), (1, 114, 1024, 3, 6)]
    for p in (ops.CONV_FWD, ops.CONV_DX, ops.CONV_DW):
        got = {ops.conv3x3_splits(*s, p) for s in shapes}
        assert 1 in got and max(got) > 1, (p, got)


@pytest.mark.parametrize('shape', [(2, 5, 7, 6, 5, 3, 2, 1), SITES[0], SITES[5], SITES[6]], ids=_ids)
def test_gradients_that_are_not_needed_are_skipped(shape):
    c = case(shape, 'normal')
    y, dx, dw = run_op(c)
    y1, dx1, dw1 = run_op(c, needs=(False, True))               # the stem: its input needs no gradient
    assert dx1 is None and torch.equal(dw1, dw) and torch.equal(y1, y)
    y2, dx2, dw2 = run_op(c, needs=(True, False))               # a frozen weight
    assert dw2 is None and torch.equal(dx2, dx) and torch.equal(y2, y)
    y3, dx3, dw3 = run_op(c, needs=(False, False))
    assert dx3 is None and dw3 is None and torch.equal(y3, y) and not y3.requires_grad
    # the entries themselves: a NULL product's buffer is not touched, and the call runs in a workspace sized for the other
    # product alone (were the unwanted one computed all the same, it would have nowhere to put its partial results)
    _, ex, ew = run_entries(c, shape, want=(True, False))
    assert torch.equal(ex, dx) and bool(torch.isnan(ew).all())
    _, ex, ew = run_entries(c, shape, want=(False, True))
    assert torch.equal(ew, dw) and bool(torch.isnan(ex).all())
    _, ex, ew = run_entries(c, shape, want=(False, False))
    assert bool(torch.isnan(ex).all()) and bool(torch.isnan(ew).all())


@pytest.mark.parametrize('shape', [(2, 8, 8, 64, 64, 3, 2, 1), (2, 3, 5, 64, 66, 7, 2, 3), (3, 19, 33, 7, 9, 1, 2, 0)], ids=_ids)
def test_misaligned_view_and_channels_last(shape):
    dev = torch.device('cuda:0')
    c = case(shape, 'normal')
    st, p = c['stride'], c['pad']
    y, dx, dw = run_op(c)

    def misaligned(t):
        flat = torch.empty(t.numel() + 1, device=dev)
        view = flat[1:].view(t.shape)                     # storage offset 1: 4 bytes past a 16-byte boundary
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view.detach()

    for got in (run_op(c, x_dev=misaligned(c['x'])), run_op(c, w_dev=misaligned(c['w'])),
                run_op(c, x_dev=misaligned(c['x']), w_dev=misaligned(c['w']))):
        assert torch.equal(got[0], y) and torch.equal(got[1], dx) and torch.equal(got[2], dw)
    xl = c['x'].to(dev).contiguous(memory_format=torch.channels_last)
    wl = c['w'].to(dev).contiguous(memory_format=torch.channels_last)
    assert not xl.is_contiguous() and (not wl.is_contiguous() or shape[5] == 1)
    got = run_op(c, x_dev=xl, w_dev=wl)
    assert torch.equal(got[0], y) and torch.equal(got[1], dx) and torch.equal(got[2], dw)
    assert got[1].shape == xl.shape and got[2].shape == wl.shape
    # a channels-last upstream gradient and a strided slice as input
    ops = _ops()
    wide = torch.zeros(shape[0], shape[1], shape[3], shape[4] + 3, device=dev)
    wide[..., 1:-2] = c['x'].to(dev)
    xs = wide[..., 1:-2].requires_grad_(True)
    ws = c['w'].to(dev).requires_grad_(True)
    assert not xs.is_contiguous()
    ys = ops.Conv2dFunction.apply(xs, ws, st, p)
    ys.backward(c['dy'].to(dev).contiguous(memory_format=torch.channels_last))
    assert torch.equal(ys.detach(), y) and torch.equal(xs.grad, dx) and torch.equal(ws.grad, dw)


@pytest.mark.parametrize('shape', [(3, 19, 33, 7, 9, 3, 3, 0), SITES[0], SITES[3], SITES[6]], ids=_ids)
def test_two_identical_calls_are_bit_equal(shape):
    c = case(shape, 'normal')
    a, b = run_op(c), run_op(c)
    for p, q in zip(a, b):
        assert torch.equal(p, q)


@pytest.mark.parametrize('shape', [(3, 19, 33, 7, 9, 3, 3, 0), SITES[0], SITES[4], SITES[5]], ids=_ids)
def test_no_sync_and_graph_replay_equals_eager(shape):
    ops = _ops()
    dev = torch.device('cuda:0')
    B, Ci, Co, H, W, k, st, p = shape
    OH, OW = R.out_size(H, W, k, st, p)
    g = torch.Generator().manual_seed(21)
    feeds = [(torch.randn(B, Ci, H, W, generator=g).to(dev), torch.randn(Co, Ci, k, k, generator=g).to(dev),
              torch.randn(B, Co, OH, OW, generator=g).to(dev)) for _ in range(3)]
    x = feeds[0][0].clone().requires_grad_(True)
    w = feeds[0][1].clone().requires_grad_(True)
    dy = feeds[0][2].clone()

    def step():
        # only detached results leave (a kept autograd graph would tie the leaves' accumulators to the stream they were made on)
        y = ops.Conv2dFunction.apply(x, w, st, p)
        return (y.detach(),) + torch.autograd.grad((y * dy).sum(), [x, w])

    def feed(i):
        with torch.no_grad():
            x.copy_(feeds[i][0])
            w.copy_(feeds[i][1])
            dy.copy_(feeds[i][2])

    step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    eager = []
    for i in range(3):
        feed(i)
        eager.append([t.clone() for t in step()])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for i in range(3):
        feed(i)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, eager[i]):
            assert torch.equal(a, b), i


# ---- the whole trunk

def _hold(name, got, ref64, plain, report):
    ek, ep = _e(got, ref64), _e(plain, ref64)
    bound = max(8.0 * ep, 8.0 * FLOOR)
    print('%-44s e_new %.3e  e_plain %.3e  bound %.3e' % (name, ek, ep, bound))
    report.append((ek / max(ep, FLOOR), name))
    assert ek <= bound, (name, ek, ep, bound)


def _trunk_fixture():
    from vpn_amd.modules.network import ResNet18
    torch.manual_seed(3)
    state = {k: v.clone() for k, v in ResNet18().state_dict().items()}
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(2, 3, 64, 64, generator=g)
    ws = [torch.randn(2, ch, 64 // s, 64 // s, generator=g) for ch, s in ((64, 4), (128, 8), (256, 16), (512, 32))]
    return state, imgs, ws


def _run_trunk(model, state, imgs, ws, dtype, device):
    from vpn_amd.modules.network import _trunk_maps
    model.load_state_dict(state, strict=True)
    model = model.to(device=device, dtype=dtype).train()
    x = imgs.to(device=device, dtype=dtype).requires_grad_(True)
    maps = _trunk_maps(model, x)
    sum((m * w.to(device=device, dtype=dtype)).sum() for m, w in zip(maps, ws)).backward()
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    grads['input'] = x.grad
    return [m.detach() for m in maps], grads


STRIDED_WEIGHTS = sorted([(64, 3, 7, 7)] + [t for c in (64, 128, 256) for t in ((2 * c, c, 3, 3), (2 * c, c, 1, 1))])


def test_whole_trunk_against_the_float64_cpu_trunk(monkeypatch):
    """ResNet18(hip_conv=True, hip_conv_strided=True), and the same with fused_norm=True, on the GPU, training mode, B = 2 at
    64 x 64, loaded from one state_dict: the four stage outputs, the input gradient and all 60 parameter gradients against
    the float64 CPU trunk.  Yardstick: the plain fp32 trunk (library convolutions) on the same GPU, measured here; bound
    max(8 e_plain, 8 x 2^-24) as tests/test_trunkconv.py sets it.  While the new trunks run, nn.Conv2d.forward and
    F.conv2d raise: no library convolution is reached."""
    from vpn_amd.modules import network
    from vpn_amd.modules.network import ResNet18
    dev = torch.device('cuda:0')
    state, imgs, ws = _trunk_fixture()
    calls3, calls2 = [], []
    real3, real2 = _ops().Conv3x3Function, _ops().Conv2dFunction

    class Counting3:
        @staticmethod
        def apply(x, weight):
            calls3.append(tuple(weight.shape))
            return real3.apply(x, weight)

    class Counting2:
        @staticmethod
        def apply(x, weight, stride, padding):
            calls2.append(tuple(weight.shape))
            return real2.apply(x, weight, stride, padding)
    monkeypatch.setattr(network, 'Conv3x3Function', Counting3)
    monkeypatch.setattr(network, 'Conv2dFunction', Counting2)

    m64, g64 = _run_trunk(ResNet18(), state, imgs, ws, torch.float64, 'cpu')
    mp, gp = _run_trunk(ResNet18(), state, imgs, ws, torch.float32, dev)
    assert calls3 == [] and calls2 == []
    assert len(g64) == 61            # 60 parameter gradients (all but fc.weight / fc.bias) and the input

    def library(*a, **k):
        raise AssertionError('a library convolution was reached')
    report = []
    for label, kwargs in (('conv + strided', dict(hip_conv=True, hip_conv_strided=True)),
                          ('fused_norm + conv + strided', dict(fused_norm=True, hip_conv=True, hip_conv_strided=True))):
        del calls3[:], calls2[:]
        with monkeypatch.context() as mk:
            mk.setattr(torch.nn.Conv2d, 'forward', library)
            mk.setattr(F, 'conv2d', library)
            mg, gg = _run_trunk(ResNet18(**kwargs), state, imgs, ws, torch.float32, dev)
        assert len(calls3) == 13 and sorted(set(calls3)) == [(c, c, 3, 3) for c in (64, 128, 256, 512)]
        assert sorted(calls2) == STRIDED_WEIGHTS and len(calls2) == 7
        assert set(gg) == set(g64)
        for i in range(4):
            _hold('%s: map %d' % (label, i), mg[i], m64[i], mp[i], report)
        for k in g64:
            _hold('%s: %s' % (label, k), gg[k], g64[k], gp[k], report)
    print('worst ratio e_new / max(e_plain, 2^-24): %.2f at %s' % max(report))
    # the strided keyword alone: exactly its seven
    del calls3[:], calls2[:]
    _run_trunk(ResNet18(hip_conv_strided=True), state, imgs, ws, torch.float32, dev)
    assert calls3 == [] and sorted(calls2) == STRIDED_WEIGHTS


def test_whole_trunk_repeats_bit_for_bit():
    """fused_norm + hip_conv + hip_conv_strided, forward and backward twice from the same state and inputs: every map and
    every gradient torch.equal."""
    from vpn_amd.modules.network import ResNet18
    dev = torch.device('cuda:0')
    state, imgs, ws = _trunk_fixture()
    runs = [_run_trunk(ResNet18(fused_norm=True, hip_conv=True, hip_conv_strided=True), state, imgs, ws, torch.float32, dev)
            for _ in range(2)]
    (ma, ga), (mb, gb) = runs
    assert len(ga) == 61 and set(ga) == set(gb)
    differ = ['map %d' % i for i in range(4) if not torch.equal(ma[i], mb[i])] + [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert differ == [], differ
