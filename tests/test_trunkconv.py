"""GPU tests of the trunk's 3x3 convolution (csrc/trunkconv.hip, ops.Conv3x3Function, ResNet18(hip_conv)).

Reference: the float64 restatement tests/trunkconv_ref.py on the CPU.
  * exact: integer-valued inputs (x in -3..3, w and dy in -2..2): every partial sum is an integer below 2^24 in magnitude
    whatever the order, so y, dx and dw must EQUAL the float64 result;
  * rounded: seeded normal inputs; per element |T - T64| <= 2 K 2^-24 A with A the same product of |x|, |w|, |dy| in
    float64 and K the reduction length (9 C_in, 9 C_out, B H W): a chain of K fused multiply-adds rounds at most K times and
    merging partial sums adds fewer than K further additions.  Derived, not tuned; e = max|T - T64| / max|T64| is printed
    next to ATen's fp32 CPU figure.
The shapes are built from the published VPN_CONV_* constants: C_out, 9 C_in, B H W and the slice count at every constant's
edges (9 C_in moves in steps of 9: the nearest multiples on both sides of T - 1 .. T + 1), the tile count at the split target's
edges, and the four trunk sites at B = 2.
Measured on an MI355X: worst e_op / max(e_aten, 2^-24) over the shapes and the whole-trunk ratio: DESIGN.md 4.19."""
import functools

import pytest
import torch
import torch.nn.functional as F

import trunkconv_ref as R

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -24


def _ops():
    from vpn_amd import ops
    return ops


def _constants():
    import vpn_amd._lib as lib
    return {k: lib.CONSTANTS[k] for k in ('VPN_CONV_TILE', 'VPN_CONV_TILE_K', 'VPN_CONV_SPLIT_TARGET', 'VPN_CONV_MAX_SPLIT')}


def _hw(n):
    """(H, W) with H W = n, as square as n allows (a prime n: one row)."""
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return h, n // h


BASE = [(1, 1, 1, 1, 1), (2, 5, 7, 5, 3), (3, 19, 33, 7, 9), (1, 3, 130, 2, 67), (2, 70, 6, 1, 33), (2, 6, 70, 33, 1)]
TRUNK = [(2, 64, 64, 32, 32), (2, 128, 128, 16, 16), (2, 256, 256, 8, 8), (2, 512, 512, 4, 4)]


@functools.lru_cache(maxsize=None)
def _shapes():
    """(B, C_in, C_out, H, W) of every case; the other dimensions of an edge shape are 2 (two taps rows, a tail everywhere)."""
    c = _constants()
    tile, tk, target, smax = c['VPN_CONV_TILE'], c['VPN_CONV_TILE_K'], c['VPN_CONV_SPLIT_TARGET'], c['VPN_CONV_MAX_SPLIT']
    out = list(BASE) + list(TRUNK)
    for T in sorted(set(c.values())):
        for v in (T - 1, T, T + 1):
            out.append((1, 2, v, 2, 2))                                   # C_out
            out.append((1,) + (2, 2) + _hw(v))                            # B H W
        for ci in sorted({max(1, (T - 1) // 9), -(-T // 9), -(-(T + 1) // 9)}):
            out.append((1, ci, 2, 2, 2))                                  # 9 C_in on both sides of T
    # the slice count at the edges of every constant it can reach (one tile: S = min(chunks, MAX_SPLIT)); chunks = n
    for T in sorted(set(c.values())):
        for n in (T - 1, T, T + 1):
            if n < 2 or n > smax + 1:
                continue
            ch = next(v for v in range(1, 16 * n) if -(-9 * v // tk) == n)        # 9 v elements: n chunks
            out.append((1, ch, 2, 2, 2))                                  # forward
            out.append((1, 2, ch, 2, 2))                                  # data gradient
            out.append((1, 2, 2) + _hw(tk * n))                           # weight gradient
    # the tile count at the split target's edges: pixels for the forward and the data gradient, weights for the weight gradient
    for tiles in (target - 1, target, target + 1):
        out.append((1, 2, 2) + _hw(tiles * tile))
    out.append((1, -(-(tile * (target // 16) + 1) // 9), 16 * tile, 3, 6))         # 16 x (target / 16 + 1) tiles of dw
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


def _splits(shape):
    ops = _ops()
    return {p: ops.conv3x3_splits(*shape, p) for p in (ops.CONV_FWD, ops.CONV_DX, ops.CONV_DW)}


def test_shapes_sit_at_the_constants_and_reach_both_regimes():
    """From the host rule (ops.conv3x3_splits, held to the library's own vpn_conv3x3_splits), not by assumption."""
    import vpn_amd._lib as lib
    ops, c, shapes = _ops(), _constants(), _shapes()
    L = lib.lib()
    for s in shapes:
        for p, S in _splits(s).items():
            assert L.vpn_conv3x3_splits(*s, p) == S, (s, p)
    for p in (ops.CONV_FWD, ops.CONV_DX, ops.CONV_DW):
        got = {_splits(s)[p] for s in shapes}
        assert 1 in got and max(got) == c['VPN_CONV_MAX_SPLIT'], (p, got)
        for T in c.values():                              # the slice counts around every constant they can reach
            for n in (T - 1, T, T + 1):
                if 2 <= n <= c['VPN_CONV_MAX_SPLIT']:
                    assert n in got, (p, n, sorted(got))
        # unsplit because there are tiles enough, not only because K is one chunk
        tile, tk = c['VPN_CONV_TILE'], c['VPN_CONV_TILE_K']
        def tiles_k(s):
            B, Ci, Co, H, W = s
            M, N, K = {ops.CONV_FWD: (Co, B * H * W, 9 * Ci), ops.CONV_DX: (Ci, B * H * W, 9 * Co), ops.CONV_DW: (Co, 9 * Ci, B * H * W)}[p]
            return -(-M // tile) * -(-N // tile), K
        assert any(tiles_k(s)[0] >= c['VPN_CONV_SPLIT_TARGET'] and tiles_k(s)[1] > tk and _splits(s)[p] == 1 for s in shapes), p
        assert any(tiles_k(s)[0] == c['VPN_CONV_SPLIT_TARGET'] - 1 and _splits(s)[p] == 2 for s in shapes) or p == ops.CONV_DW
    for T in c.values():
        assert {T - 1, T, T + 1} <= {s[2] for s in shapes} and {T - 1, T, T + 1} <= {s[0] * s[3] * s[4] for s in shapes}, T
        nine = {9 * s[1] for s in shapes}
        assert any(T - 9 <= v < T for v in nine) and any(T < v <= T + 9 for v in nine) and (T % 9 != 0 or T in nine), T
    assert all(s in shapes for s in BASE + TRUNK)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """Seeded inputs on the CPU with the float64 results, shared by every test of a shape and never written to."""
    B, Ci, Co, H, W = shape
    g = torch.Generator().manual_seed(13)
    if kind == 'int':
        x = torch.randint(-3, 4, (B, Ci, H, W), generator=g).float()
        w = torch.randint(-2, 3, (Co, Ci, 3, 3), generator=g).float()
        dy = torch.randint(-2, 3, (B, Co, H, W), generator=g).float()
    else:
        x, w, dy = torch.randn(B, Ci, H, W, generator=g), torch.randn(Co, Ci, 3, 3, generator=g), torch.randn(B, Co, H, W, generator=g)
    y64 = R.forward(x, w)
    dx64, dw64 = R.backward(dy, x, w)
    return dict(x=x, w=w, dy=dy, y=y64, dx=dx64, dw=dw64)


def run_op(c, x_dev=None, w_dev=None, needs=(True, True)):
    """The op on the GPU -> (y, dx, dw), device tensors; a gradient that was not asked for is None."""
    ops = _ops()
    dev = torch.device('cuda:0')
    x = (c['x'].to(dev) if x_dev is None else x_dev).requires_grad_(needs[0])
    w = (c['w'].to(dev) if w_dev is None else w_dev).requires_grad_(needs[1])
    y = ops.Conv3x3Function.apply(x, w)
    if any(needs):
        y.backward(c['dy'].to(dev))
    return y.detach(), x.grad, w.grad


@pytest.mark.parametrize('shape', _shapes(), ids=lambda s: '-'.join(map(str, s)))
def test_exact_on_integer_inputs(shape):
    c = case(shape, 'int')
    B, Ci, Co, H, W = shape
    assert 3 * 2 * max(9 * Ci, 9 * Co, B * H * W) < 2 ** 24        # every partial sum, in any order, is an exact integer
    y, dx, dw = run_op(c)
    for name, got in (('y', y), ('dx', dx), ('dw', dw)):
        assert got.shape == c[name].shape and got.dtype == torch.float32
        bad = int((got.double().cpu() != c[name]).sum())
        assert bad == 0, (name, bad, float((got.double().cpu() - c[name]).abs().max()))


_RATIOS = []


def _e(t, t64):
    return float((t.double().cpu() - t64).abs().max() / t64.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize('shape', _shapes(), ids=lambda s: '-'.join(map(str, s)))
def test_rounded_within_the_fma_chain_bound(shape):
    B, Ci, Co, H, W = shape
    c = case(shape, 'normal')
    A = dict(y=R.forward(c['x'].abs(), c['w'].abs()))
    A['dx'], A['dw'] = R.backward(c['dy'].abs(), c['x'].abs(), c['w'].abs())
    K = dict(y=9 * Ci, dx=9 * Co, dw=B * H * W)
    # ATen, fp32, CPU: the yardstick that is printed, not asserted
    xa, wa = c['x'].clone().requires_grad_(True), c['w'].clone().requires_grad_(True)
    ya = F.conv2d(xa, wa, None, 1, 1)
    ya.backward(c['dy'])
    aten = dict(y=ya.detach(), dx=xa.grad, dw=wa.grad)
    y, dx, dw = run_op(c)
    for name, got in (('y', y), ('dx', dx), ('dw', dw)):
        err = (got.double().cpu() - c[name]).abs()
        bound = 2.0 * K[name] * FLOOR * A[name]
        e_op, e_aten = _e(got, c[name]), _e(aten[name], c[name])
        worst = float((err / bound.clamp_min(1e-300)).max())
        print('%-2s K %6d  e_op %.3e  e_aten %.3e  worst |T - T64| / bound %.4f' % (name, K[name], e_op, e_aten, worst))
        _RATIOS.append((e_op / max(e_aten, FLOOR), name, shape))
        assert bool((err <= bound).all()), (name, worst)


def test_report_the_worst_ratio_to_aten():
    """Printed for DESIGN.md 4.19, not asserted: e_op / max(e_aten, 2^-24) over every shape and product above."""
    if _RATIOS:
        print('worst e_op / max(e_aten, 2^-24): %.2f for %s at %s' % max(_RATIOS))


@pytest.mark.parametrize('shape', [(3, 19, 33, 7, 9), (2, 64, 64, 32, 32), (1, 114, 1024, 3, 6)])
def test_gradients_that_are_not_needed_are_skipped(shape):
    c = case(shape, 'normal')
    y, dx, dw = run_op(c)
    y1, dx1, dw1 = run_op(c, needs=(False, True))               # the input needs no gradient
    assert dx1 is None and torch.equal(dw1, dw) and torch.equal(y1, y)
    y2, dx2, dw2 = run_op(c, needs=(True, False))               # a frozen weight
    assert dw2 is None and torch.equal(dx2, dx) and torch.equal(y2, y)
    y3, dx3, dw3 = run_op(c, needs=(False, False))
    assert dx3 is None and dw3 is None and torch.equal(y3, y) and not y3.requires_grad


@pytest.mark.parametrize('shape', [(2, 8, 8, 64, 64), (2, 3, 5, 64, 66), (3, 19, 33, 7, 9)])
def test_misaligned_view_and_channels_last(shape):
    dev = torch.device('cuda:0')
    c = case(shape, 'normal')
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
    assert not xl.is_contiguous() and not wl.is_contiguous()
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
    ys = ops.Conv3x3Function.apply(xs, ws)
    ys.backward(c['dy'].to(dev).contiguous(memory_format=torch.channels_last))
    assert torch.equal(ys.detach(), y) and torch.equal(xs.grad, dx) and torch.equal(ws.grad, dw)


@pytest.mark.parametrize('shape', [(3, 19, 33, 7, 9), (2, 512, 512, 4, 4), (1, 2, 2, 128, 128)])
def test_two_identical_calls_are_bit_equal(shape):
    c = case(shape, 'normal')
    a, b = run_op(c), run_op(c)
    for p, q in zip(a, b):
        assert torch.equal(p, q)


@pytest.mark.parametrize('shape', [(3, 19, 33, 7, 9), (2, 128, 128, 16, 16), (1, 2, 2, 128, 128)])
def test_no_sync_and_graph_replay_equals_eager(shape):
    ops = _ops()
    dev = torch.device('cuda:0')
    B, Ci, Co, H, W = shape
    g = torch.Generator().manual_seed(21)
    feeds = [(torch.randn(B, Ci, H, W, generator=g).to(dev), torch.randn(Co, Ci, 3, 3, generator=g).to(dev),
              torch.randn(B, Co, H, W, generator=g).to(dev)) for _ in range(3)]
    x = feeds[0][0].clone().requires_grad_(True)
    w = feeds[0][1].clone().requires_grad_(True)
    dy = feeds[0][2].clone()

    def step():
        # only detached results leave (a kept autograd graph would tie the leaves' accumulators to the stream they were made on)
        y = ops.Conv3x3Function.apply(x, w)
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
        for p, q in zip(captured, eager[i]):
            assert torch.equal(p, q), i


def _hold(name, got, ref64, plain, report):
    ek, ep = _e(got, ref64), _e(plain, ref64)
    bound = max(8.0 * ep, 8.0 * FLOOR)
    print('%-36s e_new %.3e  e_plain %.3e  bound %.3e' % (name, ek, ep, bound))
    report.append((ek / max(ep, FLOOR), name))
    assert ek <= bound, (name, ek, ep, bound)


def test_whole_trunk_against_the_float64_cpu_trunk(monkeypatch):
    """ResNet18(hip_conv=True) and ResNet18(fused_norm=True, hip_conv=True) on the GPU, training mode, B = 4 at 64 x 64,
    loaded from one state_dict: the four stage outputs, the input gradient and every parameter gradient against the
    float64 CPU trunk.  Yardstick: the plain fp32 trunk (library convolutions) on the same GPU, measured here; margin 8 as
    in tests/test_trunknorm.py (20 compounding normalisations with N = 16 at layer4).  The worst ratio is in DESIGN.md 4.19."""
    from vpn_amd.modules import network
    from vpn_amd.modules.network import ResNet18, _trunk_maps
    dev = torch.device('cuda:0')
    torch.manual_seed(3)
    state = {k: v.clone() for k, v in ResNet18().state_dict().items()}
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(4, 3, 64, 64, generator=g)
    ws = [torch.randn(4, ch, 64 // s, 64 // s, generator=g) for ch, s in ((64, 4), (128, 8), (256, 16), (512, 32))]
    calls = []

    class Counting:
        @staticmethod
        def apply(x, weight):
            calls.append(tuple(weight.shape))
            return _ops().Conv3x3Function.apply(x, weight)
    monkeypatch.setattr(network, 'Conv3x3Function', Counting)

    def run(model, dtype, device):
        model.load_state_dict(state, strict=True)
        model = model.to(device=device, dtype=dtype).train()
        x = imgs.to(device=device, dtype=dtype).requires_grad_(True)
        maps = _trunk_maps(model, x)
        sum((m * w.to(device=device, dtype=dtype)).sum() for m, w in zip(maps, ws)).backward()
        grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
        grads['input'] = x.grad
        return [m.detach() for m in maps], grads

    m64, g64 = run(ResNet18(), torch.float64, 'cpu')
    mp, gp = run(ResNet18(), torch.float32, dev)
    assert calls == []
    report = []
    for label, kwargs in (('hip_conv', dict(hip_conv=True)), ('fused_norm + hip_conv', dict(fused_norm=True, hip_conv=True))):
        del calls[:]
        mg, gg = run(ResNet18(**kwargs), torch.float32, dev)
        assert len(calls) == 13 and sorted(set(calls)) == [(c, c, 3, 3) for c in (64, 128, 256, 512)]
        assert set(gg) == set(g64) and len(gg) == 61            # all but fc.weight / fc.bias, and the input
        for i in range(4):
            _hold('%s: map %d' % (label, i), mg[i], m64[i], mp[i], report)
        for k in g64:
            _hold('%s: %s' % (label, k), gg[k], g64[k], gp[k], report)
    print('worst ratio e_new / max(e_plain, 2^-24): %.2f at %s' % max(report))
    # one stage: exactly its three stride-1 convolutions
    del calls[:]
    run(ResNet18(hip_conv=('layer4',)), torch.float32, dev)
    assert calls == [(512, 512, 3, 3)] * 3
