"""The FC heads on the GPU (csrc/fcstack.hip through FcStackFunction) against tests/network_ref.py, and the three models
on a small injected trunk.  Every comparison: conftest.rel_err <= 1e-4, the project's fp32 bar."""
import pytest
import torch
import torch.nn as nn

import network_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
RULE = dict(clamp_min=0.01, clamp_max=0.8, volume_restrict=(8.0, 10.0, 10.0))


def dev():
    return torch.device('cuda:0')


def make_case(B, ins, hidden, outs, L=5, seed=0, scale=1.0):
    """CPU fp32 inputs and parameters: per group a list of (weight, bias), nn.Linear's layout, fan-in scaled."""
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(B, i, generator=g) for i in ins]
    params = []
    for i, o in zip(ins, outs):
        widths = [i] + [hidden] * (L - 1) + [o]
        params.append([(torch.randn(widths[l + 1], widths[l], generator=g) * scale / widths[l] ** 0.5,
                        torch.randn(widths[l + 1], generator=g) * 0.1) for l in range(L)])
    return xs, params


def epilogue_ref(raw, epilogue, sig):
    if epilogue == 'none':
        return raw
    if epilogue == 'tanh':
        return [torch.tanh(raw[0])]
    return [R.vp_pack(raw[0], raw[1], raw[2], bool(sig), RULE['clamp_min'], RULE['clamp_max'], RULE['volume_restrict'])]


def run_ref(xs, params, epilogue, sig, weights, masks=None):
    """-> outputs, dX per group, [(dW, db)] per group and layer; float64."""
    xs = [x.double().requires_grad_(True) for x in xs]
    ps = [[(w.double().requires_grad_(True), b.double().requires_grad_(True)) for w, b in head] for head in params]
    outs = epilogue_ref(R.stack(xs, ps, masks), epilogue, sig)
    sum((o * w.double()).sum() for o, w in zip(outs, weights)).backward()
    return [o.detach() for o in outs], [x.grad for x in xs], [[(w.grad, b.grad) for w, b in head] for head in ps]


def run_gpu(xs, params, epilogue, sig, weights, masks=None, dropout=None, seed=0, shared=False, frozen=()):
    from vpn_amd import FcStackFunction
    d = dev()
    if shared:
        x0 = xs[0].to(d).requires_grad_(True)
        gx = [x0] * len(xs)
    else:
        gx = [x.to(d).requires_grad_(True) for x in xs]
    ps = [[(w.to(d).requires_grad_(g not in frozen), b.to(d).requires_grad_(g not in frozen)) for w, b in head]
          for g, head in enumerate(params)]
    cfg = dict(G=len(xs), L=len(params[0]), epilogue=epilogue, dropout=dropout, seed=seed, is_sigmoid=bool(sig), **RULE)
    extra = [m.to(d) for head in (masks or []) for m in head] if dropout == 'mask' else []
    outs = FcStackFunction.apply(cfg, *gx, *[t for head in ps for wb in head for t in wb], *extra)
    outs = list(outs) if isinstance(outs, tuple) else [outs]
    sum((o * w.to(d)).sum() for o, w in zip(outs, weights)).backward()
    dx = [x0.grad] if shared else [x.grad for x in gx]
    return [o.detach() for o in outs], dx, [[(w.grad, b.grad) for w, b in head] for head in ps]


def out_weights(B, outs, epilogue, seed=5):
    g = torch.Generator().manual_seed(seed)
    if epilogue == 'vp_pack':
        return [torch.randn(B, outs[0] // 3, 10, generator=g)]
    return [torch.randn(B, o, generator=g) for o in outs]


def compare(got, want):
    (go, gdx, gp), (wo, wdx, wp) = got, want
    for a, b in zip(go, wo):
        assert a.shape == b.shape and rel_err(a.cpu(), b) <= TOL
    for a, b in zip(gdx, wdx):
        assert rel_err(a.cpu(), b) <= TOL
    for gh, wh in zip(gp, wp):
        for (gw, gb), (ww, wb) in zip(gh, wh):
            assert gw.shape == ww.shape and rel_err(gw.cpu(), ww) <= TOL and rel_err(gb.cpu(), wb) <= TOL


SHAPES = [(1, 37, 72, (15, 20, 15)),        # odd row lengths: no vector path
          (3, 40, 72, (15, 20, 15)),
          (65, 64, 128, (48, 64, 48)),      # crosses every batch chunk (8, 16, 64), several output tiles
          (8, 512, 1024, (48, 64, 48))]     # the reference's widths


@pytest.mark.parametrize('epilogue,sig', [('none', 1), ('vp_pack', 1), ('vp_pack', 0)])
@pytest.mark.parametrize('B,inw,hidden,outs', SHAPES)
def test_fc_stack_vs_ref(B, inw, hidden, outs, epilogue, sig):
    from vpn_amd import pack_head_outputs
    xs, params = make_case(B, [inw] * 3, hidden, outs, seed=B)
    wts = out_weights(B, outs, epilogue)
    got = run_gpu(xs, params, epilogue, sig, wts)
    compare(got, run_ref(xs, params, epilogue, sig, wts))
    if epilogue == 'vp_pack':       # the fused epilogue and the stand-alone head kernel apply one rule (vpn_head_rule.h)
        raw = run_gpu(xs, params, 'none', sig, out_weights(B, outs, 'none'))[0]
        packed = pack_head_outputs(raw[0], raw[1], raw[2], bool(sig), RULE['clamp_min'], RULE['clamp_max'], RULE['volume_restrict'])
        assert rel_err(got[0][0], packed) <= 1e-6


def test_fc_stack_one_group_tanh():
    xs, params = make_case(3, [40], 72, (1158,), seed=2)
    wts = out_weights(3, (1158,), 'tanh')
    got = run_gpu(xs, params, 'tanh', 1, wts)
    assert float(got[0][0].abs().max()) < 1.0
    compare(got, run_ref(xs, params, 'tanh', 1, wts))


def test_fc_stack_one_layer_and_wide_input():
    xs, params = make_case(3, [40] * 3, 72, (15, 20, 15), L=1, seed=3)
    wts = out_weights(3, (15, 20, 15), 'none')
    compare(run_gpu(xs, params, 'none', 1, wts), run_ref(xs, params, 'none', 1, wts))
    # a row longer than one register tile (1024 columns) and groups of different input widths
    xs, params = make_case(2, [1100, 40], 36, (9, 6), L=2, seed=4)
    wts = out_weights(2, (9, 6), 'none')
    compare(run_gpu(xs, params, 'none', 1, wts), run_ref(xs, params, 'none', 1, wts))


def test_shared_input_gradient_is_the_sum():
    B, outs = 3, (15, 20, 15)
    xs, params = make_case(B, [40] * 3, 72, outs, seed=6)
    xs = [xs[0]] * 3
    wts = out_weights(B, outs, 'vp_pack')
    sep = run_gpu(xs, params, 'vp_pack', 1, wts)
    one = run_gpu(xs, params, 'vp_pack', 1, wts, shared=True)
    want = run_ref(xs, params, 'vp_pack', 1, wts)
    assert rel_err(one[1][0].cpu(), sum(want[1])) <= TOL
    assert rel_err(one[1][0], sep[1][0] + sep[1][1] + sep[1][2]) <= 1e-6


def test_frozen_group():
    B, outs = 3, (15, 20, 15)
    xs, params = make_case(B, [40] * 3, 72, outs, seed=7)
    wts = out_weights(B, outs, 'vp_pack')
    full = run_gpu(xs, params, 'vp_pack', 1, wts)
    part = run_gpu(xs, params, 'vp_pack', 1, wts, frozen=(0,))
    assert all(w is None and b is None for w, b in part[2][0])       # no buffer was made for them: NULL dw / db went down
    for g in (1, 2):
        for (w, b), (fw, fb) in zip(part[2][g], full[2][g]):
            assert torch.equal(w, fw) and torch.equal(b, fb)
    assert all(torch.equal(a, b) for a, b in zip(part[1], full[1]))


def test_dropout_explicit_masks():
    B, outs = 9, (15, 20, 15)
    xs, params = make_case(B, [40] * 3, 72, outs, seed=8)
    g = torch.Generator().manual_seed(9)
    masks = [[(torch.rand(B, 72, generator=g) < 0.5).to(torch.uint8) for _ in range(4)] for _ in range(3)]
    wts = out_weights(B, outs, 'vp_pack')
    got = run_gpu(xs, params, 'vp_pack', 1, wts, masks=masks, dropout='mask')
    compare(got, run_ref(xs, params, 'vp_pack', 1, wts, masks=masks))
    assert rel_err(got[0][0], run_gpu(xs, params, 'vp_pack', 1, wts)[0][0]) > 1e-3       # the masks did something


def test_dropout_philox():
    B, hidden, outs = 65, 128, (48, 64, 48)
    xs, params = make_case(B, [64] * 3, hidden, outs, seed=10)
    wts = out_weights(B, outs, 'none')
    a = run_gpu(xs, params, 'none', 1, wts, dropout='philox', seed=1234)
    b = run_gpu(xs, params, 'none', 1, wts, dropout='philox', seed=1234)
    c = run_gpu(xs, params, 'none', 1, wts, dropout='philox', seed=1235)
    assert all(torch.equal(p, q) for p, q in zip(a[0] + a[1], b[0] + b[1]))
    assert not torch.equal(a[0][0], c[0][0])
    # the kept fraction of every (group, layer, b, o): in a stack of l + 2 layers whose layer l has zero weights and unit
    # biases and whose last layer is the identity, the output is keep_l / (1 - p), that is 2 or 0
    from vpn_amd import FcStackFunction
    d = dev()
    kept = total = 0
    for l in range(4):       # stacks of l + 2 layers: the output of the last layer counts the ones kept after layer l
        L = l + 2
        ws = []
        for g in range(3):
            for j in range(L):
                last = j == L - 1
                rows, cols = hidden, (64 if j == 0 else hidden)
                if last:                                    # the last layer copies its input: identity weights, no bias
                    ws += [torch.eye(hidden, device=d), torch.zeros(hidden, device=d)]
                elif j == L - 2:                            # the layer under test: zero weights, unit bias -> 2 * keep
                    ws += [torch.zeros(rows, cols, device=d), torch.ones(rows, device=d)]
                else:
                    ws += [torch.zeros(rows, cols, device=d), torch.zeros(rows, device=d)]
        x = torch.zeros(B, 64, device=d)
        outs_l = FcStackFunction.apply(dict(G=3, L=L, epilogue='none', dropout='philox', seed=77, p=0.5), x, x, x, *ws)
        for o in outs_l:
            assert bool(((o == 0) | (o == 2)).all())
            kept += int((o == 2).sum())
            total += o.numel()
    assert total == 65 * 128 * 4 * 3
    assert abs(kept / total - 0.5) <= 0.02        # 1 standard error of a fair coin is 0.0016 here
    # for fixed masks the stack is affine in x: <y(x + d) - y(x), w> = <dX, d>
    dlt = [torch.randn_like(x) for x in xs]
    moved = run_gpu([x + e for x, e in zip(xs, dlt)], params, 'none', 1, wts, dropout='philox', seed=1234)
    lhs = sum(float(((m.double() - y.double()) * w.to(d).double()).sum()) for m, y, w in zip(moved[0], a[0], wts))
    rhs = sum(float((gx.double() * e.to(d).double()).sum()) for gx, e in zip(a[1], dlt))
    print('philox linearity: lhs %.9g rhs %.9g' % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), abs(rhs))
    # a device seed: the kernels add the tensor's value to the host seed, forward and backward alike
    dseed = torch.full((1,), 1000, dtype=torch.int64, device=d)
    e = run_gpu(xs, params, 'none', 1, wts, dropout='philox', seed=dseed)
    f = run_gpu(xs, params, 'none', 1, wts, dropout='philox', seed=1000)
    assert all(torch.equal(p, q) for p, q in zip(e[0] + e[1], f[0] + f[1]))
    dseed += 234
    e = run_gpu(xs, params, 'none', 1, wts, dropout='philox', seed=dseed)
    assert all(torch.equal(p, q) for p, q in zip(e[0] + e[1], a[0] + a[1]))


def test_eval_applies_no_mask():
    from vpn_amd import FcHeads
    torch.manual_seed(0)
    heads = FcHeads({'a': 7, 'b': 5}, is_dropout=True, feat=40, hidden=72).to(dev())
    x = torch.randn(3, 40, device=dev())
    heads.train()
    t1, t2 = heads.run_heads([x, x]), heads.run_heads([x, x])
    assert not torch.equal(t1[0], t2[0])                       # a new draw every call
    heads.eval()
    e = heads.run_heads([x, x])
    params = [[(m.weight.detach().cpu(), m.bias.detach().cpu()) for m in head] for head in heads.head_linears()]
    want = R.stack([x.cpu(), x.cpu()], params)
    assert rel_err(e[0].cpu(), want[0]) <= TOL and rel_err(e[1].cpu(), want[1]) <= TOL


def test_deterministic():
    B, outs = 65, (48, 64, 48)
    xs, params = make_case(B, [64] * 3, 128, outs, seed=11)
    wts = out_weights(B, outs, 'vp_pack')
    a = run_gpu(xs, params, 'vp_pack', 1, wts)
    b = run_gpu(xs, params, 'vp_pack', 1, wts)
    flat = lambda r: r[0] + r[1] + [t for head in r[2] for wb in head for t in wb]
    assert all(torch.equal(p, q) for p, q in zip(flat(a), flat(b)))


def test_no_sync_and_graph_capture():
    from vpn_amd import FcStackFunction
    d = dev()
    B, outs = 9, (15, 20, 15)
    xs, params = make_case(B, [40] * 3, 72, outs, seed=12)
    gx = [x.to(d).requires_grad_(True) for x in xs]
    flat = [t.to(d).requires_grad_(True) for head in params for wb in head for t in wb]
    wt = out_weights(B, outs, 'vp_pack')[0].to(d)
    cfg = dict(G=3, L=5, epilogue='vp_pack', is_sigmoid=True, **RULE)

    def step():
        # only detached results leave: a kept autograd graph would keep the leaves' gradient accumulators, and with them
        # the stream they were made on; a backward captured later would then hand its gradients to that stream, a fork
        # out of the capture that nothing joins
        out = FcStackFunction.apply(cfg, *gx, *flat)
        return out.detach(), torch.autograd.grad((out * wt).sum(), gx + flat)

    eager = step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured[0], eager[0])
    assert all(torch.equal(p, q) for p, q in zip(captured[1], eager[1]))


class Mix(nn.Module):
    """A 1x1 channel mix by matmul (no convolution library is involved)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(cout, cin) / cin ** 0.5)

    def forward(self, x):
        return torch.einsum('oc,bchw->bohw', self.weight, x)


class PlainTrunk(nn.Module):
    def __init__(self, feat=40):
        super().__init__()
        self.conv1, self.bn1, self.relu, self.maxpool = Mix(3, 8), nn.Identity(), nn.ReLU(), nn.AvgPool2d(2)
        self.layer1, self.layer2, self.layer3, self.layer4 = Mix(8, 8), Mix(8, 16), Mix(16, 16), Mix(16, feat)


def test_whole_models():
    import vpn_amd
    from vpn_amd import VPNetOneRes, VPNetTwoRes, SDNet
    d = dev()
    torch.manual_seed(3)
    imgs = torch.rand(2, 3, 16, 16, device=d)
    K = 4
    one = VPNetOneRes(vp_num=K, hidden=72, feat=40, trunk=PlainTrunk()).to(d)
    res = one(imgs)
    assert len(res) == 5
    v, q, t, maps, feats = res
    assert len(v) == len(q) == len(t) == K and tuple(v[0].shape) == (2, 3) and tuple(q[0].shape) == (2, 4)
    assert len(maps) == 4 and tuple(feats.shape) == (2, 40)
    params, _, feats2 = one.forward_packed(imgs)
    assert tuple(params.shape) == (2, K, 10) and torch.equal(params[:, 1, 3:7], q[1])
    heads = [[(m.weight.detach().cpu(), m.bias.detach().cpu()) for m in head] for head in one.head_linears()]
    f = feats2.detach().cpu()
    want = R.vp_pack(*R.stack([f, f, f], heads), True, vpn_amd.config.VP_CLAMP_MIN, vpn_amd.config.VP_CLAMP_MAX, vpn_amd.config.VOLUME_RESTRICT)
    assert rel_err(params.detach().cpu(), want) <= TOL
    raw = [torch.randn(2, n * K, device=d) for n in (3, 4, 3)]          # the reference calls these on the class
    for got, ref in zip(VPNetOneRes.restrict_range(*raw), R.restrict_range(*[r.cpu().double() for r in raw], True, 0.01, 0.8)):
        assert rel_err(got.cpu(), ref) <= TOL
    u = torch.rand(2, K, 32, 3, device=d)
    pts = vpn_amd.Sampling.sample_primitives(params, [1, 0, 0, 0], 32, u=u)
    assert pts.shape[0] == 2 and pts.shape[-1] == 3 and bool(torch.isfinite(pts).all())
    # an Adam step moves every unfrozen parameter and leaves the frozen head alone
    one.fix_volume_weight()
    before = {n: p.detach().clone() for n, p in one.named_parameters()}
    opt = torch.optim.Adam([p for p in one.parameters() if p.requires_grad], lr=1e-2)
    params, _, _ = one.forward_packed(imgs)
    vpn_amd.Sampling.sample_primitives(params, [1, 0, 0, 0], 32, u=u).square().sum().backward()
    opt.step()
    for n, p in one.named_parameters():
        assert torch.equal(p, before[n]) == n.startswith('volume_fc.'), n

    two = VPNetTwoRes(vp_num=K, hidden=72, feat=40, trunk=(PlainTrunk(), PlainTrunk())).to(d)
    res = two(imgs)
    assert len(res) == 3 and len(res[0]) == K
    vf = two.extract_feature(two.volume_resnet, imgs).detach().cpu()
    tf = two.extract_feature(two.transform_resnet, imgs).detach().cpu()
    heads = [[(m.weight.detach().cpu(), m.bias.detach().cpu()) for m in head] for head in two.head_linears()]
    want = R.vp_pack(*R.stack([vf, tf, tf], heads), True, vpn_amd.config.VP_CLAMP_MIN, vpn_amd.config.VP_CLAMP_MAX, vpn_amd.config.VOLUME_RESTRICT)
    assert rel_err(two.forward_packed(imgs).detach().cpu(), want) <= TOL
    assert rel_err(vf, tf) > 1e-2                      # two different trunks: a swap of the routing would show

    sd = SDNet(hidden=72, feat=40, trunk=PlainTrunk()).to(d)
    off = sd(imgs)
    assert tuple(off.shape) == (2, 386, 3) and float(off.abs().max()) < 1.0
    before = {n: p.detach().clone() for n, p in sd.named_parameters()}
    opt = torch.optim.Adam(sd.parameters(), lr=1e-2)
    off.square().sum().backward()
    opt.step()
    assert all(not torch.equal(p, before[n]) for n, p in sd.named_parameters())
