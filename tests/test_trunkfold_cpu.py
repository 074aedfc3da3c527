"""CPU-only checks of the trunk's inference form (csrc/trunkfold.hip, ops.conv2d_bias_act, vpn_amd.fold_batch_norm,
ResNet18.fold): the C ABI, every rejection before any HIP call, the restatement tests/trunkfold_ref.py against
torch's own convolution and eval-mode batch norm in float64, the fold against the restatement, the routing of the trunk and
of the three models, the state_dict, the stale fold, the example's switch and the kernels' resources."""
import ast
import ctypes
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from kernel_resources import kernel_resources, load_build
import trunkfold_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'vpn_conv2d_bias_act_fwd'


def test_header_declares_the_entry_and_the_library_exports_it():
    b = load_build()
    assert 'trunkfold.hip' in b.SOURCES
    assert b.PER_FILE.get('trunkfold.hip', []) == b.PER_FILE.get('trunkstride.hip', [])
    import vpn_amd
    import vpn_amd._lib as lib
    from vpn_amd import ops
    _v, _i, _z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert lib.SIGNATURES[ENTRY] == (_i, [_v] * 5 + [_i] * 9 + [_v, _z, _v])
    assert hasattr(ctypes.CDLL(b.build(verbose=False)), ENTRY)
    assert lib.lib().vpn_abi_version() == lib.ABI_VERSION == 9          # an entry was added, none changed
    assert vpn_amd.conv2d_bias_act is ops.conv2d_bias_act is vpn_amd.modules.network.conv2d_bias_act
    assert vpn_amd.fold_batch_norm is vpn_amd.modules.network.fold_batch_norm
    text = open(lib.HEADER_PATH).read()
    comment = text[text.index('csrc/trunkfold.hip'):text.index('int ' + ENTRY)]
    assert 'nn.Conv2d + nn.BatchNorm2d (eval) + add + ReLU' in comment and 'vpnet_one_resnet.py:45-57' in comment


def test_every_rejection_comes_before_any_hip_call():
    """On a machine without a GPU a HIP call would fail with a positive HIP error: every code below is the entry's own, and
    where vpn_conv2d_fwd rejects the same arguments, the same."""
    import vpn_amd._lib as lib
    L = lib.lib()
    bad, big = lib.CONSTANTS['VPN_E_BADARG'], lib.CONSTANTS['VPN_E_TOOBIG']
    buf = (ctypes.c_float * 64)()              # host memory standing in for tensors: validation never reads them
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 16 == 0
    off = ctypes.c_void_p(p.value + 4)

    def fold(x=p, w=p, bias=p, res=p, y=p, B=1, Ci=1, Co=1, H=1, W=1, R=1, st=1, pad=0, relu=1, ws=None, wsb=0):
        return L.vpn_conv2d_bias_act_fwd(x, w, bias, res, y, B, Ci, Co, H, W, R, st, pad, relu, ws, wsb, None)

    def plain(x=p, w=p, bias=None, res=None, y=p, B=1, Ci=1, Co=1, H=1, W=1, R=1, st=1, pad=0, relu=1, ws=None, wsb=0):
        return L.vpn_conv2d_fwd(x, w, y, B, Ci, Co, H, W, R, st, pad, ws, wsb, None)

    def both(code, **k):
        assert fold(**k) == code and plain(**k) == code, k
        assert fold(bias=None, res=None, relu=0, **k) == code, k

    split = dict(B=2, Ci=5, Co=7, H=6, W=5, R=3, st=2, pad=1)            # one tile, three chunks: split
    dims = (2, 5, 7, 6, 5, 3, 2, 1)
    assert L.vpn_conv2d_splits(*dims, 1) > 1
    for k in ('x', 'w', 'y'):
        both(bad, **{k: None})
    for k in ('B', 'Ci', 'Co', 'H', 'W'):
        both(bad, **{k: 0})
        both(bad, **{k: -3})
    for k in (0, 2, 4, 5, 6, 8, 9, -3):
        both(bad, R=k, pad=4, H=9, W=9)
    for k in (dict(st=0), dict(st=-2), dict(pad=-1), dict(R=3, H=2, W=9), dict(R=3, H=9, W=2), dict(R=7, H=1, W=1, pad=2)):
        both(bad, **k)
    # relu outside {0, 1}: the entry's own rejection, also where everything else is fine and no workspace is needed
    for r in (2, -1, 3, 256, 2 ** 31 - 1):
        assert fold(relu=r) == bad and fold(relu=r, bias=None, res=None) == bad, r
    # a workspace that is needed and missing, too small or misaligned
    need = L.vpn_conv2d_workspace(*dims, 1)
    assert need > 0
    both(bad, **split)
    both(bad, ws=p, wsb=need - 4, **split)
    both(bad, ws=off, wsb=1 << 20, **split)
    # 2^31 elements or more in x, y or w; more than 65535 tiles along M; padded coordinates are ints
    for k in (dict(B=2 ** 15, H=2 ** 8, W=2 ** 8), dict(B=2 ** 10, Ci=2 ** 5, H=2 ** 8, W=2 ** 8), dict(B=2 ** 13, H=2 ** 8, W=2 ** 8, pad=2 ** 8),
              dict(B=2 ** 15, H=2 ** 8, W=2 ** 8, st=2), dict(Ci=2 ** 14, Co=2 ** 14, R=3, pad=1), dict(Ci=2 ** 13, Co=2 ** 13, R=7, pad=3),
              dict(Co=65536 * 64)):
        both(big, ws=p, wsb=64, **k)
    both(big, H=2 ** 20, W=2 ** 20)
    both(big, pad=2 ** 30, st=2 ** 30)


def test_every_refusal_of_the_function_is_raised_before_any_launch(monkeypatch):
    import vpn_amd
    from vpn_amd import _lib

    def no_library(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'call', no_library)
    monkeypatch.setattr(_lib, 'lib', no_library)
    f = vpn_amd.conv2d_bias_act
    x, w, b = torch.randn(2, 3, 8, 8), torch.randn(5, 3, 3, 3), torch.randn(5)
    res = torch.randn(2, 5, 4, 4)                                      # stride 2, padding 1
    # inference only
    for k in range(4):
        args = [x, w, b, res]
        args[k] = args[k].clone().requires_grad_(True)
        with pytest.raises(RuntimeError, match=r'conv2d \+ batch_norm_act'):
            f(*args, stride=2, padding=1)
    # what conv2d refuses
    with pytest.raises(ValueError, match='B, C_in, H, W'):
        f(x[0], w, b, None, 2, 1)
    with pytest.raises(ValueError, match='C_out, C_in, R, R'):
        f(x, torch.randn(5, 3, 3, 1), b, None, 2, 1)
    for k in (2, 5):
        with pytest.raises(NotImplementedError, match='kernel size'):
            f(x, torch.randn(5, 3, k, k), b, None, 2, 1)
    with pytest.raises(ValueError, match='input channels'):
        f(x, torch.randn(5, 4, 3, 3), b, None, 2, 1)
    for stride in (0, -1, 1.5, (2, 2)):
        with pytest.raises(ValueError, match='stride'):
            f(x, w, b, None, stride, 1)
    for padding in (-1, 0.5, 'same', (1, 1)):
        with pytest.raises(ValueError, match='padding'):
            f(x, w, b, None, 2, padding)
    with pytest.raises(NotImplementedError, match='fp32'):
        f(x.double(), w.double(), None, None, 2, 1)
    with pytest.raises(NotImplementedError, match='fp32'):
        f(x, w.half(), None, None, 2, 1)
    with pytest.raises(ValueError, match='empty'):
        f(x[:0], w, b, None, 2, 1)
    with pytest.raises(ValueError, match='smaller than'):
        f(x[:, :, :4, :4], torch.randn(5, 3, 7, 7), b, None, 2, 1)
    # the bias and the residual
    for bias in (torch.randn(4), torch.randn(5, 1), torch.randn(1, 5), torch.randn(())):
        with pytest.raises(ValueError, match=r'bias must be \(C_out,\)'):
            f(x, w, bias, None, 2, 1)
    for bias in (b.double(), b.half(), torch.zeros(5, dtype=torch.int32)):
        with pytest.raises(NotImplementedError, match='bias is'):
            f(x, w, bias, None, 2, 1)
    for r in (torch.randn(2, 5, 4, 5), torch.randn(2, 5, 8, 8), torch.randn(1, 5, 4, 4), torch.randn(2, 5, 16), torch.randn(2, 1, 4, 4)):
        with pytest.raises(ValueError, match='residual must have the shape'):
            f(x, w, b, r, 2, 1)
    with pytest.raises(NotImplementedError, match='residual is'):
        f(x, w, b, res.double(), 2, 1)
    for relu in (2, -1, None, 'yes', 0.5):
        with pytest.raises(ValueError, match='relu'):
            f(x, w, b, res, 2, 1, relu)
    # a tensor on another device
    for k, name in ((1, 'weight'), (2, 'bias'), (3, 'residual')):
        args = [x, w, b, res]
        args[k] = args[k].to('meta')
        with pytest.raises(ValueError, match='%s is on meta' % name):
            f(*args, stride=2, padding=1)
    # the last refusal: there is no CPU path
    with pytest.raises(ValueError, match='GPU only'):
        f(x, w, b, res, 2, 1)
    with pytest.raises(ValueError, match='GPU only'):
        f(x, w)                                                        # the defaults: no bias, no residual, stride 1, padding 0


@pytest.mark.parametrize('cfg', [(k, st) for k in (1, 3, 7) for st in (1, 2, 3)], ids=lambda c: 'R%d-s%d' % c)
def test_restatement_equals_torch_in_float64(cfg):
    """relu(F.batch_norm(F.conv2d(x, w), ..., training=False) + res) against the restatement of the op on the restated fold."""
    k, st = cfg
    p = k // 2
    eps = 1e-5
    for B, Ci, Co, H, W in [(2, 3, 5, 9, 11), (1, 4, 6, 8, 7)]:
        g = torch.Generator().manual_seed(11)
        OH, OW = R.out_size(H, W, k, st, p)
        x = torch.randn(B, Ci, H, W, generator=g, dtype=torch.float64)
        w = torch.randn(Co, Ci, k, k, generator=g, dtype=torch.float64)
        gamma, beta, mean = (torch.randn(Co, generator=g, dtype=torch.float64) for _ in range(3))
        var = torch.rand(Co, generator=g, dtype=torch.float64) + 0.1
        res = torch.randn(B, Co, OH, OW, generator=g, dtype=torch.float64)
        wf, bf = R.fold(w, gamma, beta, mean, var, eps)
        for use_res in (False, True):
            for relu in (False, True):
                t = F.batch_norm(F.conv2d(x, w, None, st, p), mean, var, gamma, beta, False, 0.1, eps)
                t = t + res if use_res else t
                t = F.relu(t) if relu else t
                a = R.forward(x, wf, bf, res if use_res else None, st, p, relu)
                assert a.shape == t.shape == (B, Co, OH, OW)
                err = float((a - t).abs().max() / t.abs().max())
                assert err <= 1e-12, (cfg, use_res, relu, err)
        # without a bias the op is the convolution's restatement
        assert torch.equal(R.forward(x, w, None, None, st, p, False), R.trunkstride_ref.forward(x, w, st, p))


def _norm(C, seed, gamma=None, var=None):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C).eval()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g) if gamma is None else gamma)
        bn.bias.copy_(torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.1 if var is None else var)
    return bn


def test_fold_batch_norm_equals_the_restatement():
    import vpn_amd
    C = 6
    g = torch.Generator().manual_seed(5)
    w = torch.randn(C, 4, 3, 3, generator=g)
    x = torch.randn(2, 4, 7, 7, generator=g)
    norms = {'plain': _norm(C, 1),
             'negative and zero gamma': _norm(C, 2, gamma=torch.tensor([-1.5, 0.0, 0.7, -0.01, 0.0, 2.0])),
             'running_var of 0': _norm(C, 3, var=torch.tensor([0.0, 1.0, 0.0, 0.3, 2.0, 0.0]))}
    for name, bn in norms.items():
        wf, bf = vpn_amd.fold_batch_norm(w, bn)
        assert wf.dtype == bf.dtype == torch.float32 and wf.shape == w.shape and bf.shape == (C,), name
        assert not wf.requires_grad and not bf.requires_grad
        w64, b64 = R.fold(w, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)
        assert torch.equal(wf, w64.float()) and torch.equal(bf, b64.float()), name          # float64, rounded to fp32 once
        assert bool(torch.isfinite(wf).all()) and bool(torch.isfinite(bf).all()), name
        # and the folded convolution is the eval-mode norm of the convolution
        with torch.no_grad():
            want = bn.double()(F.conv2d(x.double(), w.double(), None, 1, 1))
        got = R.forward(x, w64, b64, None, 1, 1, False)
        assert float((got - want).abs().max() / want.abs().max()) <= 1e-12, name
        bn.float()
    wf, bf = vpn_amd.fold_batch_norm(w, norms['negative and zero gamma'])
    assert int(wf[1].ne(0).sum()) == 0 and int(wf[4].ne(0).sum()) == 0          # a zero gamma channel: only the shift is left
    assert float(bf[1]) == float(norms['negative and zero gamma'].bias[1])
    # the mode of the norm is not asked, and nothing of it is written
    bn = _norm(C, 1).train()
    before = {k: v.clone() for k, v in bn.state_dict().items()}
    a = vpn_amd.fold_batch_norm(w, bn)
    b = vpn_amd.fold_batch_norm(w, norms['plain'])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(v, before[k]) for k, v in bn.state_dict().items())
    with pytest.raises(ValueError, match='affine'):
        vpn_amd.fold_batch_norm(w, nn.BatchNorm2d(C, affine=False))
    with pytest.raises(ValueError, match='running statistics'):
        vpn_amd.fold_batch_norm(w, nn.BatchNorm2d(C, track_running_stats=False))
    with pytest.raises(ValueError, match='C_out'):
        vpn_amd.fold_batch_norm(w[:5], norms['plain'])


# ---- the routing, with conv2d_bias_act replaced by a torch composition that counts its calls

def _composition(calls):
    def conv2d_bias_act(x, weight, bias=None, residual=None, stride=1, padding=0, relu=True):
        calls.append(dict(w=tuple(weight.shape), stride=stride, padding=padding, bias=bias is not None,
                          residual=residual is not None, relu=relu))
        y = F.conv2d(x, weight, bias, stride, padding)
        y = y if residual is None else y + residual
        return F.relu(y) if relu else y
    return conv2d_bias_act


def _randomise_norms(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.randn(m.num_features, generator=g))
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    return model


@pytest.fixture
def calls(monkeypatch):
    from vpn_amd.modules import network
    out = []
    monkeypatch.setattr(network, 'conv2d_bias_act', _composition(out))
    return out


# (weight shape, stride, padding) of the trunk's 20 convolutions, sorted
def _trunk_convs():
    out = [((64, 3, 7, 7), 2, 3)] + [((64, 64, 3, 3), 1, 1)] * 4
    for c in (64, 128, 256):
        out += [((2 * c, c, 3, 3), 2, 1), ((2 * c, c, 1, 1), 2, 0)] + [((2 * c, 2 * c, 3, 3), 1, 1)] * 3
    return sorted(out)


def test_folded_trunk_makes_twenty_calls_and_equals_the_unfolded_trunk(calls):
    from vpn_amd.modules.network import ResNet18, _trunk_maps, _trunk_features
    torch.manual_seed(1)
    m = _randomise_norms(ResNet18().eval(), 2)
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        want_maps, want_feats = _trunk_features(m, x)
        want_y = m(x)
        assert calls == []
        assert m.fold() is m
        got = _trunk_maps(m, x)
        assert len(calls) == 20
        assert sorted((c['w'], c['stride'], c['padding']) for c in calls) == _trunk_convs()
        assert all(c['bias'] for c in calls)
        assert sum(c['residual'] for c in calls) == 8
        assert all(c['relu'] for c in calls if c['residual'])
        off = [c for c in calls if not c['relu']]
        assert [c['w'] for c in off] == [(128, 64, 1, 1), (256, 128, 1, 1), (512, 256, 1, 1)] and not any(c['residual'] for c in off)
        assert calls[0]['w'] == (64, 3, 7, 7) and calls[0]['relu'] and not calls[0]['residual']
        for a, b in zip(got, want_maps):
            assert a.shape == b.shape and float((a - b).abs().max() / b.abs().max()) <= 1e-5
        del calls[:]
        maps, feats = _trunk_features(m, x)
        assert len(calls) == 20 and all(torch.equal(a, b) for a, b in zip(maps, got))
        assert feats.shape == (2, 512) and float((feats - want_feats).abs().max() / want_feats.abs().max()) <= 1e-5
        del calls[:]
        y = m(x)
        assert len(calls) == 20 and float((y - want_y).abs().max() / want_y.abs().max()) <= 1e-5


@pytest.mark.parametrize('kwargs', [dict(), dict(fused_norm=True, fused_pool=True, fused_tail=True, hip_conv=True, hip_conv_strided=True)],
                         ids=['plain', 'every keyword'])
def test_the_keywords_select_nothing_on_the_folded_path(calls, kwargs, monkeypatch):
    """With every keyword on, the unfolded trunk would reach the library on this machine; the folded one calls the patched
    op 20 times and the two ATen pools, and gives the plain trunk's folded result bit for bit."""
    from vpn_amd import _lib
    from vpn_amd.modules.network import ResNet18, _trunk_features

    def no_library(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'call', no_library)
    torch.manual_seed(1)
    plain = _randomise_norms(ResNet18().eval(), 2)
    m = ResNet18(**kwargs).eval()
    m.load_state_dict(plain.state_dict(), strict=True)
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        want = _trunk_features(plain.fold(), x)
        del calls[:]
        got = _trunk_features(m.fold(), x)
    assert len(calls) == 20
    assert all(torch.equal(a, b) for a, b in zip(got[0], want[0])) and torch.equal(got[1], want[1])


def test_the_fold_is_not_used_with_grad_mode_on_in_training_mode_or_after_unfold(calls):
    from vpn_amd.modules.network import ResNet18, _trunk_maps
    torch.manual_seed(1)
    m = _randomise_norms(ResNet18().eval(), 2)
    ref = ResNet18()
    ref.load_state_dict(m.state_dict(), strict=True)
    x = torch.randn(2, 3, 32, 32)
    m.fold()
    # grad mode on, eval: the unfolded graph, differentiable
    ref.eval()
    got, want = _trunk_maps(m, x), _trunk_maps(ref, x)
    assert calls == [] and all(torch.equal(a, b) for a, b in zip(got, want)) and got[3].requires_grad
    assert torch.equal(m(x), ref(x)) and calls == []
    # training mode under no_grad: the batch statistics, and the running ones move as the unfolded trunk's do
    m.train()
    ref.train()
    with torch.no_grad():
        got, want = _trunk_maps(m, x), _trunk_maps(ref, x)
    assert calls == [] and all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.equal(v, ref.state_dict()[k]) for k, v in m.state_dict().items())
    # after unfold
    m.eval()
    ref.eval()
    assert m.unfold() is m
    with torch.no_grad():
        got, want = _trunk_maps(m, x), _trunk_maps(ref, x)
        assert calls == [] and all(torch.equal(a, b) for a, b in zip(got, want))
        assert torch.equal(m(x), ref(x)) and calls == []
        m.fold()
        _trunk_maps(m, x)
    assert len(calls) == 20


def test_state_dict_is_unchanged_by_the_fold():
    import inspect
    from vpn_amd.modules.network import ResNet18, BasicBlock
    torch.manual_seed(0)
    m, other = ResNet18().eval(), ResNet18()
    before = m.state_dict()
    keys = list(before)
    n_params, n_buffers, n_modules = len(list(m.parameters())), len(list(m.buffers())), len(list(m.modules()))
    m.fold()
    after = m.state_dict()
    assert len(before) == len(after) == 122 and list(after) == keys
    assert all(torch.equal(after[k], before[k]) for k in keys)
    assert (len(list(m.parameters())), len(list(m.buffers())), len(list(m.modules()))) == (n_params, n_buffers, n_modules)
    other.load_state_dict(after, strict=True)                          # both ways
    m.load_state_dict(other.state_dict(), strict=True)
    m.unfold()
    assert list(m.state_dict()) == keys
    # no keyword was added
    assert list(inspect.signature(ResNet18.__init__).parameters) == ['self', 'num_classes', 'fused_norm', 'hip_conv', 'hip_conv_strided',
                                                                     'fused_pool', 'fused_tail']
    assert list(inspect.signature(BasicBlock.__init__).parameters) == ['self', 'inplanes', 'planes', 'stride', 'fused_norm', 'hip_conv',
                                                                       'hip_conv_strided']


def test_a_stale_fold_raises_until_fold_is_called_again(calls):
    from vpn_amd.modules.network import ResNet18, _trunk_maps
    torch.manual_seed(1)
    m = _randomise_norms(ResNet18().eval(), 2).fold()
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        _trunk_maps(m, x)
        assert len(calls) == 20
        # load_state_dict copies into every tensor: their versions move
        m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()}, strict=True)
        del calls[:]
        for run in (lambda: _trunk_maps(m, x), lambda: m(x)):
            with pytest.raises(RuntimeError, match=r'fold\(\) again'):
                run()
        assert calls == []                                             # raised before the first site
        _trunk_maps(m.fold(), x)
        assert len(calls) == 20
        # an in-place edit of one running_var
        m.layer3[1].bn2.running_var.mul_(2.0)
        with pytest.raises(RuntimeError, match=r'fold\(\) again'):
            _trunk_maps(m, x)
        want = _trunk_maps(m.unfold(), x)
        got = _trunk_maps(m.fold(), x)                                 # the new fold is of the new statistics
        assert all(float((a - b).abs().max() / b.abs().max()) <= 1e-5 for a, b in zip(got, want))
        # an optimiser step
        opt = torch.optim.SGD([m.layer1[0].conv1.weight], lr=0.1)
        m.layer1[0].conv1.weight.grad = torch.ones_like(m.layer1[0].conv1.weight)
        opt.step()
        with pytest.raises(RuntimeError, match=r'fold\(\) again'):
            _trunk_maps(m, x)
        # a parameter that was replaced
        m.fold()
        m.conv1.weight = nn.Parameter(m.conv1.weight.detach().clone())
        with pytest.raises(RuntimeError, match=r'fold\(\) again'):
            _trunk_maps(m, x)
        _trunk_maps(m.fold(), x)
    # with grad mode on the fold is not asked, stale or not
    m.bn1.running_var.mul_(2.0)
    _trunk_maps(m, x)


def test_the_models_take_the_folded_path_through_their_own_extract_feature(calls):
    from vpn_amd.modules.network import VPNetOneRes, VPNetTwoRes, SDNet
    torch.manual_seed(2)
    x = torch.randn(1, 3, 32, 32)

    def close(a, b):
        return a.shape == b.shape and float((a - b).abs().max() / b.abs().max()) <= 1e-5
    with torch.no_grad():
        one = VPNetOneRes().eval()
        _randomise_norms(one.resnet, 3)
        want_feats, want_maps = one.extract_feature(x)
        assert calls == []
        one.resnet.fold()
        feats, maps = one.extract_feature(x)
        assert len(calls) == 20 and close(feats, want_feats) and all(close(a, b) for a, b in zip(maps, want_maps))

        two = VPNetTwoRes().eval()
        trunks = [two.volume_resnet, two.transform_resnet]
        assert len(trunks) == 2
        for t in trunks:
            _randomise_norms(t, 4)
        want = [two.extract_feature(t, x) for t in trunks]
        del calls[:]
        for t in trunks:
            t.fold()
        got = [two.extract_feature(t, x) for t in trunks]
        assert len(calls) == 40 and all(close(a, b) for a, b in zip(got, want))

        sd = SDNet().eval()
        _randomise_norms(sd._model, 5)
        want = sd.extract_feature(x)
        del calls[:]
        sd._model.fold()
        got = sd.extract_feature(x)
        assert len(calls) == 20 and close(got, want)


def test_the_gcn_example_takes_the_fold_switch():
    """--vpn-fold is a flag of its own, off by default, and the example folds the frozen trunk after .eval() (read from the
    source: the example needs a GPU to run)."""
    src = open(os.path.join(ROOT, 'examples', 'train_gcn_step.py')).read()
    tree = ast.parse(src)
    adds = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, 'attr', '') == 'add_argument' and n.args
            and getattr(n.args[0], 'value', None) == '--vpn-fold']
    assert len(adds) == 1
    kw = {k.arg: ast.literal_eval(k.value) for k in adds[0].keywords if k.arg != 'help'}
    assert kw == {'action': 'store_true'}
    folds = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, 'attr', '') == 'fold']
    assert len(folds) == 1 and ast.unparse(folds[0]) == 'vpn.resnet.fold()'
    evals = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, 'attr', '') == 'eval']
    assert min(n.lineno for n in evals) < folds[0].lineno
    guard = [n for n in ast.walk(tree) if isinstance(n, ast.If) and any(f is c for c in ast.walk(n) for f in folds)]
    assert any(ast.unparse(n.test) == 'args.vpn_fold' for n in guard)


def test_trunkfold_compiles_as_build_py_compiles_it_within_the_resource_limits():
    rows = kernel_resources('trunkfold.hip')
    # one GEMM kernel per kernel size, the epilogue merge by 4 and by 1
    assert len(rows) == 5, list(rows)
    assert sum('cf_gemm_kernel' in k for k in rows) == 3 and sum('cf_merge_kernel' in k for k in rows) == 2
    for k, v in rows.items():
        assert v['ScratchSize'] == 0, (k, v)
        assert v['LDS'] <= 64 * 1024, (k, v)
        assert v['AGPRs'] + v['VGPRs'] <= 128, (k, v)          # four waves per SIMD fit
