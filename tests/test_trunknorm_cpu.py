"""CPU-only checks of the trunk's norm / add / ReLU op (csrc/trunknorm.hip, ops.BatchNormActFunction, ResNet18(fused_norm);
DESIGN.md 4.18): the restatement tests/trunknorm_ref.py against torch's own batch norm and autograd in float64, the
state_dict of the fused trunk, what the op refuses before any launch, and the C ABI."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
import trunknorm_ref as R


def _case(shape, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = torch.randn(shape, generator=g, dtype=dtype)
    return dict(x=x, res=torch.randn(shape, generator=g, dtype=dtype), dy=torch.randn(shape, generator=g, dtype=dtype),
                w=1 + 0.3 * torch.randn(C, generator=g, dtype=dtype), b=0.3 * torch.randn(C, generator=g, dtype=dtype),
                rm=0.1 * torch.randn(C, generator=g, dtype=dtype), rv=1 + 0.2 * torch.rand(C, generator=g, dtype=dtype))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('relu,residual', [(1, 0), (1, 1), (0, 0), (0, 1)])
@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (3, 8, 4, 4), (5, 6, 33, 31)])
def test_restatement_equals_torch_in_float64(shape, relu, residual, training):
    c = _case(shape, 7)
    momentum, eps = 0.1, 1e-5
    x = c['x'].clone().requires_grad_(True)
    w, b = c['w'].clone().requires_grad_(True), c['b'].clone().requires_grad_(True)
    res = c['res'].clone().requires_grad_(True) if residual else None
    rm, rv = c['rm'].clone(), c['rv'].clone()
    out = F.batch_norm(x, rm, rv, w, b, training, momentum, eps)
    if residual:
        out = out + res
    if relu:
        out = torch.relu(out)
    out.backward(c['dy'])
    nbt = torch.tensor(5)
    y, _pre, mean, invstd, rm2, rv2, nbt2 = R.forward(c['x'], c['w'], c['b'], c['rm'], c['rv'], nbt, c['res'] if residual else None,
                                                     training, momentum, eps, relu)
    dx, dw, db, dres = R.backward(c['dy'], c['x'], y, c['w'], mean, invstd, training, relu, bool(residual))
    assert int(nbt2) == 5 + int(training) and int(nbt) == 5
    pairs = [(y, out.detach()), (rm2, rm), (rv2, rv), (dx, x.grad), (dw, w.grad), (db, b.grad)]
    if residual:
        pairs.append((dres, res.grad))
    else:
        assert dres is None
    for i, (a, t) in enumerate(pairs):
        assert _rel(a, t) <= 1e-12, (i, _rel(a, t))


def test_fused_trunk_has_the_same_state_dict():
    from vpn_amd.modules.network import ResNet18, BasicBlock
    torch.manual_seed(0)
    plain, fused = ResNet18(), ResNet18(fused_norm=True)
    sp, sf = plain.state_dict(), fused.state_dict()
    assert len(sp) == 122 and list(sp) == list(sf)
    assert all(sp[k].shape == sf[k].shape and sp[k].dtype == sf[k].dtype for k in sp)
    fused.load_state_dict(sp, strict=True)
    plain.load_state_dict(fused.state_dict(), strict=True)
    assert all(torch.equal(fused.state_dict()[k], sp[k]) for k in sp)
    assert fused.fused_norm and not plain.fused_norm and not ResNet18(num_classes=10).fused_norm
    assert all(m.fused_norm for m in fused.modules() if isinstance(m, BasicBlock))
    assert not any(m.fused_norm for m in plain.modules() if isinstance(m, BasicBlock))
    assert not BasicBlock(8, 8).fused_norm and BasicBlock(8, 16, 2, fused_norm=True).downsample is not None


def test_every_refusal_is_raised_before_any_launch(monkeypatch):
    import vpn_amd
    from vpn_amd import ops, _lib

    def no_library(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'call', no_library)
    monkeypatch.setattr(_lib, 'lib', no_library)
    c = _case((2, 3, 4, 4), 3, torch.float32)
    nbt = torch.tensor(0)

    def apply(x=c['x'], w=c['w'], b=c['b'], rm=c['rm'], rv=c['rv'], n=nbt, res=None, training=True, momentum=0.1):
        return ops.BatchNormActFunction.apply(x, w, b, rm, rv, n, res, training, momentum, 1e-5, True)

    with pytest.raises(NotImplementedError, match='fp32'):
        apply(x=c['x'].double())
    with pytest.raises(NotImplementedError, match='fp32'):
        apply(x=c['x'].half(), w=c['w'].half(), b=c['b'].half())
    with pytest.raises(NotImplementedError, match='fp32'):
        apply(res=c['res'].double())
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        apply(x=c['x'][:1, :, :1, :1])
    apply_eval_n1 = pytest.raises(ValueError, match='GPU only')          # N == 1 is fine in eval: the next refusal is the device
    with apply_eval_n1:
        apply(x=c['x'][:1, :, :1, :1], training=False)
    with pytest.raises(NotImplementedError, match='momentum=None'):
        apply(momentum=None)
    with pytest.raises(NotImplementedError, match='track_running_stats=False'):
        apply(rm=None, rv=None, n=None)
    with pytest.raises(ValueError, match='residual has shape'):
        apply(res=c['res'][:, :, :2])
    with pytest.raises(ValueError, match='weight must have shape'):
        apply(w=c['w'][:2])
    with pytest.raises(ValueError, match='GPU only'):
        apply()
    # the functional form reads the module: the same refusals
    bn = torch.nn.BatchNorm2d(3)
    with pytest.raises(ValueError, match='GPU only'):
        vpn_amd.batch_norm_act(c['x'], bn, residual=c['res'], relu=True)
    with pytest.raises(NotImplementedError, match='momentum=None'):
        vpn_amd.batch_norm_act(c['x'], torch.nn.BatchNorm2d(3, momentum=None))
    with pytest.raises(NotImplementedError, match='track_running_stats=False'):
        vpn_amd.batch_norm_act(c['x'], torch.nn.BatchNorm2d(3, track_running_stats=False))
    with pytest.raises(ValueError, match='residual has shape'):
        vpn_amd.batch_norm_act(c['x'], bn, residual=c['res'][:1])
    assert int(bn.num_batches_tracked) == 0 and torch.equal(bn.running_mean, torch.zeros(3))


def test_header_declares_the_entry_points_and_the_library_exports_them():
    import importlib.util
    spec = importlib.util.spec_from_file_location('vpn_build', os.path.join(ROOT, 'volumetric-primitives-net_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert 'trunknorm.hip' in b.SOURCES
    import vpn_amd._lib as lib
    from vpn_amd import ops
    _v, _i, _f, _z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert lib.SIGNATURES['vpn_bn_act_workspace'] == (_z, [_i, _i, _i, _i])
    assert lib.SIGNATURES['vpn_bn_act_fwd'] == (_i, [_v] * 7 + [_i] * 5 + [_f, _f, _i] + [_v] * 4 + [_z, _v])
    assert lib.SIGNATURES['vpn_bn_act_bwd'] == (_i, [_v] * 6 + [_i] * 5 + [_f, _i] + [_v] * 5 + [_z, _v])
    L = ctypes.CDLL(b.build(verbose=False))
    for name in ('vpn_bn_act_fwd', 'vpn_bn_act_bwd', 'vpn_bn_act_workspace'):
        assert hasattr(L, name), name
    assert lib.lib().vpn_abi_version() == lib.ABI_VERSION == 9          # entries were added, none changed
    one, sl = lib.CONSTANTS['VPN_BN_ONE_PASS_MAX'], lib.CONSTANTS['VPN_BN_SLICE']
    assert ops.TRUNKNORM_ONE_PASS_MAX == one and ops.TRUNKNORM_SLICE == sl and one % sl == 0 and sl % 1024 == 0


def test_shape_validation_and_workspace_need_no_gpu():
    import vpn_amd._lib as lib
    L = lib.lib()
    bad, big = lib.CONSTANTS['VPN_E_BADARG'], lib.CONSTANTS['VPN_E_TOOBIG']
    one, sl = lib.CONSTANTS['VPN_BN_ONE_PASS_MAX'], lib.CONSTANTS['VPN_BN_SLICE']
    assert L.vpn_bn_act_workspace(2, 8, 64, 64) == 0 and 2 * 64 * 64 == one
    assert L.vpn_bn_act_workspace(2, 3, 64, 65) == 3 * -(-2 * 64 * 65 // sl) * 8
    assert L.vpn_bn_act_workspace(8, 64, 64, 64) == 64 * 16 * 8
    assert L.vpn_bn_act_workspace(0, 3, 4, 4) == 0
    buf = (ctypes.c_float * 64)()              # host memory standing in for tensors: validation never reads them
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(x=p, B=2, C=1, H=2, W=2, training=1, momentum=0.1, eps=1e-5, ws=None, wsb=0, rm=p):
        return L.vpn_bn_act_fwd(x, None, p, p, rm, p, p, B, C, H, W, training, momentum, eps, 1, p, p, p, ws, wsb, None)
    assert fwd(x=None) == bad and fwd(B=0) == bad and fwd(C=-1) == bad and fwd(eps=-1.0) == bad and fwd(momentum=1.5) == bad
    assert fwd(B=1, H=1, W=1) == bad                                   # one value per channel in training
    assert fwd(training=0, rm=None) == bad                             # eval reads the running statistics
    assert fwd(B=4, H=64, W=64) == bad and fwd(B=4, H=64, W=64, ws=p, wsb=8) == bad     # two-launch regime: workspace
    assert fwd(B=65536, H=2048, W=1, ws=p, wsb=64) == big and fwd(B=2 ** 16, H=2 ** 8, W=2 ** 8) == big
    assert L.vpn_bn_act_bwd(p, p, None, p, p, p, 2, 1, 2, 2, 1, 1e-5, 1, p, None, p, p, None, 0, None) == bad    # ReLU needs y
    assert L.vpn_bn_act_bwd(None, p, p, p, p, p, 2, 1, 2, 2, 1, 1e-5, 1, p, None, p, p, None, 0, None) == bad
    assert L.vpn_bn_act_bwd(p, p, p, p, p, p, 4, 1, 64, 64, 1, 1e-5, 1, p, None, p, p, None, 0, None) == bad
    assert L.vpn_bn_act_bwd(p, p, p, p, p, p, 2, 1, 2, 2, 1, 1e-5, 1, None, None, None, None, None, 0, None) == 0  # nothing wanted
