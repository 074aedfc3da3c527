"""GPU tests of the trunk's inference form (csrc/trunkfold.hip, ops.conv2d_bias_act, ResNet18.fold).
Shapes are (B, C_in, C_out, H, W, R, stride, pad).

Reference: the float64 restatement tests/trunkfold_ref.py on the CPU.
  * exact: integer-valued inputs (x in -3..3, w in -2..2, bias and residual in -9..9): every partial sum and both adds are
    integers below 2^24 in magnitude, so y must EQUAL the float64 result, in all eight combinations of bias, residual and
    ReLU.  y holds NaN before the call: an element the kernels forgot to write is caught;
  * rounded: seeded normal inputs; per element |y - y64| <= (2 K + 2) 2^-24 (sum |w||x| + |bias| + |residual|), K = R R C_in:
    the chain bound DESIGN.md 4.19 derives plus one rounding for each of the two adds; the ReLU does not round;
  * with no bias, no residual and no ReLU the result is vpn_amd.conv2d's bit for bit;
  * the folded trunk and the folded frozen VPNetOneRes hold the float64 CPU eval trunk within max(8 e_plain, 8 x 2^-24), e_plain
    measured here on the plain fp32 eval trunk of the same GPU (the rule of tests/test_trunkstride.py::_hold).
Measured on an MI355X: the worst fraction of the bound and the whole-trunk ratios are in DESIGN.md 4.25."""
import functools
import itertools
import os
import subprocess
import sys

import pytest
import torch

import network_ref as NR
import trunkfold_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -24

ONE_CHUNK = (1, 1, 1, 1, 1, 1, 2, 0)          # one chunk: unsplit
ONE_TILE = (2, 5, 7, 6, 5, 3, 2, 1)           # one tile, split, tails everywhere; 126 elements: the element merge
STRADDLE = (4, 5, 7, 6, 5, 3, 2, 1)           # split, 252 elements of 9 pixels a channel: a float4 of the merge holds two channels
STEM = (4, 3, 64, 128, 128, 7, 2, 3)          # the real stem, 256 tiles, unsplit
UNSPLIT3 = (1, 2, 2, 128, 128, 3, 1, 1)       # unsplit at stride 1
UNSPLIT1 = (1, 20, 2, 256, 256, 1, 2, 0)      # 1x1, 256 tiles and two chunks: unsplit by the tile rule
SPLIT1 = (2, 40, 7, 8, 8, 1, 2, 0)            # a 1x1 downsample of three chunks: split
SHAPES = [
    ONE_CHUNK,
    ONE_TILE,
    STRADDLE,
    (1, 4, 65, 16, 16, 3, 2, 1),              # M tail past 64
    (3, 19, 33, 7, 9, 3, 3, 0),               # stride 3, odd sizes
    (1, 3, 130, 2, 67, 7, 1, 5),              # padding wider than the image edge
    STEM,
    UNSPLIT3,
    (2, 6, 7, 8, 8, 1, 2, 0),                 # a 1x1 downsample (one chunk)
    SPLIT1,
    UNSPLIT1,
    (2, 256, 512, 4, 4, 3, 2, 1),             # layer4.0.conv1 at B = 2: 8 tiles, 32 slices
]
BIT_EQUAL = [SPLIT1, UNSPLIT1, ONE_TILE, UNSPLIT3, (1, 3, 130, 2, 67, 7, 1, 5), STEM]          # per R: one split, one unsplit
COMBOS = list(itertools.product((False, True), repeat=3))          # (bias, residual, relu)
_ids = lambda s: '-'.join(map(str, s))          # noqa: E731


def _ops():
    from vpn_amd import ops
    return ops


def _S(shape):
    return _ops().conv2d_splits(*shape, _ops().CONV_FWD)


def _out(shape):
    B, Ci, Co, H, W, k, st, p = shape
    return (B, Co) + R.out_size(H, W, k, st, p)


def test_shapes_reach_every_branch():
    """From the host rule (ops.conv2d_splits, held to the library's own vpn_conv2d_splits), not by assumption."""
    import vpn_amd._lib as lib
    L, c = lib.lib(), lib.CONSTANTS
    tile, tk, target = c['VPN_CONV_TILE'], c['VPN_CONV_TILE_K'], c['VPN_CONV_SPLIT_TARGET']
    assert len(set(SHAPES)) == len(SHAPES)
    for s in SHAPES:
        assert L.vpn_conv2d_splits(*s, 1) == _S(s), s

    def tiles_k(s):
        B, Co, OH, OW = _out(s)
        return -(-Co // tile) * -(-(B * OH * OW) // tile), s[5] * s[5] * s[1]
    # every kernel size in both regimes, among all shapes and among those of the bit-equality test
    for shapes in (SHAPES, BIT_EQUAL):
        for k in (1, 3, 7):
            got = {_S(s) for s in shapes if s[5] == k}
            assert 1 in got and max(got) > 1, (k, got)
    assert set(BIT_EQUAL) <= set(SHAPES)
    assert max(_S(s) for s in SHAPES) == c['VPN_CONV_MAX_SPLIT']
    # unsplit because there are tiles enough, not only because K is one chunk; unsplit by one chunk; split with one tile and more
    assert any(tiles_k(s)[0] >= target and tiles_k(s)[1] > tk and _S(s) == 1 for s in SHAPES)
    assert _S(ONE_CHUNK) == 1 and tiles_k(ONE_CHUNK) == (1, 1)
    assert _S(ONE_TILE) > 1 and tiles_k(ONE_TILE)[0] == 1
    assert any(tiles_k(s)[0] > 1 and _S(s) > 1 for s in SHAPES)
    assert _S(STEM) == 1 and tiles_k(STEM)[0] == 256 and _S(UNSPLIT3) == 1
    # tails in M, N and K
    assert any(_out(s)[1] % tile and _out(s)[1] > tile for s in SHAPES)
    assert any((_out(s)[0] * _out(s)[2] * _out(s)[3]) % tile for s in SHAPES) and any(tiles_k(s)[1] % tk for s in SHAPES)
    # the merge: a split shape whose element count is a multiple of 4 (16-byte accesses: torch's allocations are aligned) while
    # its OH OW is not, so a float4 holds two channels; and a split shape whose element count is no multiple of 4 (element accesses)
    B, Co, OH, OW = _out(STRADDLE)
    assert _S(STRADDLE) > 1 and (B * Co * OH * OW) % 4 == 0 and (OH * OW) % 4 != 0 and OH * OW == 9
    B, Co, OH, OW = _out(ONE_TILE)
    assert _S(ONE_TILE) > 1 and (B * Co * OH * OW) % 4 != 0


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """Seeded inputs on the CPU with the float64 convolution, shared by every test of a shape and never written to."""
    B, Ci, Co, H, W, k, st, p = shape
    g = torch.Generator().manual_seed(13)
    if kind == 'int':
        x = torch.randint(-3, 4, (B, Ci, H, W), generator=g).float()
        w = torch.randint(-2, 3, (Co, Ci, k, k), generator=g).float()
        bias = torch.randint(-9, 10, (Co,), generator=g).float()
        res = torch.randint(-9, 10, _out(shape), generator=g).float()
    else:
        x, w, bias, res = (torch.randn(s, generator=g) for s in ((B, Ci, H, W), (Co, Ci, k, k), (Co,), _out(shape)))
    return dict(x=x, w=w, bias=bias, res=res, conv=R.trunkstride_ref.forward(x, w, st, p), stride=st, pad=p)


def want(c, combo):
    """The float64 restatement from the shared convolution: the epilogue's three steps in their order."""
    y = c['conv']
    if combo[0]:
        y = y + c['bias'].double().view(1, -1, 1, 1)
    if combo[1]:
        y = y + c['res'].double()
    return torch.where(y < 0, torch.zeros_like(y), y) if combo[2] else y


@functools.lru_cache(maxsize=None)
def on_gpu(shape, kind):
    dev = torch.device('cuda:0')
    c = case(shape, kind)
    return {k: c[k].to(dev) for k in ('x', 'w', 'bias', 'res')}


def run_op(shape, kind, combo, **over):
    import vpn_amd
    c, d = case(shape, kind), dict(on_gpu(shape, kind), **over)
    with torch.no_grad():
        return vpn_amd.conv2d_bias_act(d['x'], d['w'], d['bias'] if combo[0] else None, d['res'] if combo[1] else None,
                                       c['stride'], c['pad'], combo[2])


def run_entry(shape, kind, combo):
    """The C entry on a y that holds NaN before the call."""
    from vpn_amd import _lib
    ops = _ops()
    dev = torch.device('cuda:0')
    d = on_gpu(shape, kind)
    y = torch.full(_out(shape), float('nan'), device=dev)
    ws, nbytes = ops._conv2d_ws(shape, ops.CONV_FWD, dev)
    _lib.call('vpn_conv2d_bias_act_fwd', d['x'], d['w'], d['bias'] if combo[0] else None, d['res'] if combo[1] else None, y, *shape,
              int(combo[2]), ws, nbytes, _lib.stream())
    return y


def test_restatement_from_the_shared_convolution_is_the_restatement():
    c = case(ONE_TILE, 'normal')
    for combo in COMBOS:
        full = R.forward(c['x'], c['w'], c['bias'] if combo[0] else None, c['res'] if combo[1] else None, c['stride'], c['pad'], combo[2])
        assert torch.equal(full, want(c, combo)), combo


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_exact_on_integer_inputs(shape):
    c = case(shape, 'int')
    assert 3 * 2 * shape[5] * shape[5] * shape[1] + 18 < 2 ** 24        # every partial sum, in any order, and both adds: exact integers
    for combo in COMBOS:
        w64 = want(c, combo)
        for got in (run_entry(shape, 'int', combo), run_op(shape, 'int', combo)):
            assert got.shape == w64.shape and got.dtype == torch.float32
            bad = int((~(got.double().cpu() == w64)).sum())          # a NaN left behind is counted
            assert bad == 0, (combo, bad, float((got.double().cpu() - w64).abs().max()))


_FRACTIONS = []


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_rounded_within_the_chain_bound_plus_two_roundings(shape):
    c = case(shape, 'normal')
    K = shape[5] * shape[5] * shape[1]
    A = R.trunkstride_ref.forward(c['x'].abs(), c['w'].abs(), c['stride'], c['pad'])
    for combo in COMBOS:
        mag = A + (c['bias'].double().abs().view(1, -1, 1, 1) if combo[0] else 0) + (c['res'].double().abs() if combo[1] else 0)
        bound = (2.0 * K + 2.0) * FLOOR * mag
        err = (run_op(shape, 'normal', combo).double().cpu() - want(c, combo)).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print('bias %d residual %d relu %d  K %5d  worst |y - y64| / bound %.4f' % (combo + (K, worst)))
        _FRACTIONS.append((worst, combo, shape))
        assert bool((err <= bound).all()), (combo, worst)


def test_report_the_worst_fraction_of_the_bound():
    """Printed for DESIGN.md 4.25, not asserted here (every case above asserts its own)."""
    if _FRACTIONS:
        print('worst |y - y64| / ((2 K + 2) 2^-24 A): %.4f for %s at %s' % max(_FRACTIONS))


@pytest.mark.parametrize('shape', BIT_EQUAL, ids=_ids)
def test_bit_equal_to_conv2d_without_an_epilogue(shape):
    import vpn_amd
    c, d = case(shape, 'normal'), on_gpu(shape, 'normal')
    with torch.no_grad():
        plain = vpn_amd.conv2d(d['x'], d['w'], c['stride'], c['pad'])
    assert torch.equal(run_op(shape, 'normal', (False, False, False)), plain)
    assert torch.equal(run_entry(shape, 'normal', (False, False, False)), plain)


@pytest.mark.parametrize('shape', [STRADDLE, (3, 19, 33, 7, 9, 3, 3, 0), UNSPLIT3], ids=_ids)
def test_misaligned_view_and_channels_last(shape):
    dev = torch.device('cuda:0')
    d = on_gpu(shape, 'normal')
    full = (True, True, True)
    y = run_op(shape, 'normal', full)

    def misaligned(t):
        flat = torch.empty(t.numel() + 1, device=dev)
        view = flat[1:].view(t.shape)                     # storage offset 1: 4 bytes past a 16-byte boundary
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    for over in (dict(x=misaligned(d['x'])), dict(res=misaligned(d['res'])), dict(x=misaligned(d['x']), res=misaligned(d['res'])),
                 dict(w=misaligned(d['w']), bias=misaligned(d['bias']))):
        assert torch.equal(run_op(shape, 'normal', full, **over), y), list(over)
    xl = d['x'].contiguous(memory_format=torch.channels_last)
    rl = d['res'].contiguous(memory_format=torch.channels_last)
    assert not xl.is_contiguous() and not rl.is_contiguous()
    for over in (dict(x=xl), dict(res=rl), dict(x=xl, res=rl)):
        got = run_op(shape, 'normal', full, **over)
        assert torch.equal(got, y) and got.is_contiguous(), list(over)


@pytest.mark.parametrize('shape', [ONE_TILE, STRADDLE, SPLIT1, UNSPLIT3], ids=_ids)
def test_repeats_without_sync_and_graph_replay_equals_eager(shape):
    import vpn_amd
    dev = torch.device('cuda:0')
    c = case(shape, 'normal')
    g = torch.Generator().manual_seed(21)
    names = ('x', 'w', 'bias', 'res')
    feeds = [[torch.randn(c[k].shape, generator=g).to(dev) for k in names] for _ in range(3)]
    x, w, bias, res = (t.clone() for t in feeds[0])

    def step():
        with torch.no_grad():
            return vpn_amd.conv2d_bias_act(x, w, bias, res, c['stride'], c['pad'], True)

    def feed(i):
        for t, s in zip((x, w, bias, res), feeds[i]):
            t.copy_(s)

    a = step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        b = step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(a, b)                                 # two identical calls
    eager = []
    for i in range(3):
        feed(i)
        eager.append(step().clone())
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
        assert torch.equal(captured, eager[i]), i


@pytest.mark.parametrize('shape', [UNSPLIT3, ONE_TILE, STRADDLE], ids=_ids)
def test_a_nan_in_x_reaches_y_through_the_relu(shape):
    """In the unsplit store, in the element merge and in the merge by 4: v < 0 ? 0 : v keeps a NaN."""
    d = on_gpu(shape, 'normal')
    x = d['x'].clone()
    x[0, 0, x.shape[2] // 2, x.shape[3] // 2] = float('nan')
    for combo in ((False, False, True), (True, True, True)):
        y = run_op(shape, 'normal', combo, x=x)
        clean = run_op(shape, 'normal', combo)
        nan = torch.isnan(y)
        assert bool(nan.any()) and not bool(nan.all())
        assert not bool(torch.isnan(y[1:]).any()) and bool(torch.isnan(y[0]).any())          # image 0 alone holds it
        assert torch.equal(y[~nan], clean[~nan])


# ---- the whole trunk and the frozen VPN

def _e(t, t64):
    return float((t.double().cpu() - t64).abs().max() / t64.abs().max().clamp_min(1e-300))


def _hold(name, got, ref64, plain, report):
    ek, ep = _e(got, ref64), _e(plain, ref64)
    bound = max(8.0 * ep, 8.0 * FLOOR)
    print('%-28s e_folded %.3e  e_plain %.3e  bound %.3e' % (name, ek, ep, bound))
    report.append((ek / max(ep, FLOOR), name))
    assert ek <= bound, (name, ek, ep, bound)


def _randomise_norms(model, seed):
    """Random running statistics, gamma with negative and zero channels."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                C = m.num_features
                gamma = torch.randn(C, generator=g) * 0.5 + 1.0
                gamma[torch.randperm(C, generator=g)[:C // 8]] *= -1.0
                gamma[torch.randperm(C, generator=g)[:C // 16]] = 0.0
                m.weight.copy_(gamma)
                m.bias.copy_(torch.randn(C, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return model


def test_whole_trunk_against_the_float64_cpu_eval_trunk(monkeypatch):
    from vpn_amd.modules import network
    from vpn_amd.modules.network import ResNet18, _trunk_features
    dev = torch.device('cuda:0')
    torch.manual_seed(3)
    state = _randomise_norms(ResNet18(), 5).state_dict()
    assert any(bool((v < 0).any()) and bool((v == 0).any()) for k, v in state.items() if k.endswith('bn1.weight'))
    imgs = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(4))

    def run(dtype, device, fold):
        m = ResNet18()
        m.load_state_dict(state, strict=True)
        m = m.to(device=device, dtype=dtype).eval()
        with torch.no_grad():
            maps, feats = _trunk_features(m.fold() if fold else m, imgs.to(device=device, dtype=dtype))
        return maps + [feats]

    calls = []
    real = network.conv2d_bias_act

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(network, 'conv2d_bias_act', counting)
    r64, plain = run(torch.float64, 'cpu', False), run(torch.float32, dev, False)
    assert calls == []
    folded = run(torch.float32, dev, True)
    assert len(calls) == 20
    report = []
    for i, name in enumerate(('map 0', 'map 1', 'map 2', 'map 3', 'features')):
        assert folded[i].shape == r64[i].shape
        _hold('trunk: ' + name, folded[i], r64[i], plain[i], report)
    print('worst ratio e_folded / max(e_plain, 2^-24): %.2f at %s' % max(report))
    again = run(torch.float32, dev, True)
    assert all(torch.equal(a, b) for a, b in zip(folded, again))


def test_frozen_vpn_folded_against_the_unfolded_model():
    from vpn_amd.modules.network import VPNetOneRes
    dev = torch.device('cuda:0')
    torch.manual_seed(6)
    base = VPNetOneRes()
    _randomise_norms(base.resnet, 7)
    state = base.state_dict()
    imgs = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(8))

    def run(dtype, device, fold):
        m = VPNetOneRes()
        m.load_state_dict(state, strict=True)
        m = m.to(device=device, dtype=dtype).eval()
        if fold:
            m.resnet.fold()
        with torch.no_grad():
            x = imgs.to(device=device, dtype=dtype)
            if device == 'cpu':          # the float64 model: the trunk by its modules, the heads by tests/network_ref.py
                feats, maps = m.extract_feature(x)
                heads = [[(l.weight.detach(), l.bias.detach()) for l in head] for head in m.head_linears()]
                return list(maps) + [feats, NR.vp_pack(*NR.stack([feats] * 3, heads), **m._rule)]
            params, maps, feats = m.forward_packed(x)
            return list(maps) + [feats, params]
    r64, plain, folded, again = run(torch.float64, 'cpu', False), run(torch.float32, dev, False), run(torch.float32, dev, True), run(torch.float32, dev, True)
    report = []
    for i, name in enumerate(('map 0', 'map 1', 'map 2', 'map 3', 'features', 'packed parameters')):
        assert folded[i].shape == r64[i].shape and bool(torch.isfinite(folded[i]).all())
        _hold('VPNetOneRes: ' + name, folded[i], r64[i], plain[i], report)
    print('worst ratio e_folded / max(e_plain, 2^-24): %.2f at %s' % max(report))
    assert all(torch.equal(a, b) for a, b in zip(folded, again))          # the folded forward repeats bit for bit


def test_train_gcn_step_example_runs_with_the_folded_vpn():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'train_gcn_step.py'), '--net', 'vpnet_oneres', '--vpn-fold',
                        '--steps', '2', '--batch', '2'], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith('step ')]
    assert len(lines) == 2, r.stdout
    for l in lines:
        cd, emd = float(l.split('CD Loss = ')[1].split(',')[0]), float(l.split('EMD Loss = ')[1])
        assert cd == cd and emd == emd and abs(cd) < float('inf') and abs(emd) < float('inf'), l
