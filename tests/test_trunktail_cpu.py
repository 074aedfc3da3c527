"""CPU-only checks of the trunk's tail (the tt_ kernels of csrc/trunknorm.hip, ops.BatchNormMeanFunction,
ResNet18(fused_tail)): the restatement tests/trunktail_ref.py against torch's own batch norm, add, ReLU, mean
and autograd in float64, the C ABI, the state_dict of the trunk, the pools it accepts and the examples' switch."""
import ast
import ctypes
import itertools
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import ROOT
import trunknorm_ref
import trunktail_ref as R

SHAPES = [(8, 512, 4, 4), (3, 64, 4, 4), (2, 3, 5, 7), (2, 5, 16, 16), (1, 4, 19, 27), (5, 6, 33, 31), (2, 3, 64, 65), (3, 2, 53, 53),
          (40, 2, 15, 15), (4, 3, 1, 1)]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize('relu,residual', [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_restatement_equals_torch_in_float64(shape, training, relu, residual):
    g = torch.Generator().manual_seed(11)
    B, C, H, W = shape
    f64 = dict(generator=g, dtype=torch.float64)
    x, res, dy, dm = torch.randn(shape, **f64), torch.randn(shape, **f64), torch.randn(shape, **f64), torch.randn((B, C), **f64)
    w0, b0 = 1 + 0.3 * torch.randn(C, **f64), 0.3 * torch.randn(C, **f64)
    rm0, rv0 = 0.1 * torch.randn(C, **f64), 1 + 0.2 * torch.rand(C, **f64)
    xa, w, b = x.clone().requires_grad_(True), w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    ra = res.clone().requires_grad_(True)
    rm, rv = rm0.clone(), rv0.clone()
    out = F.batch_norm(xa, rm, rv, w, b, training, 0.1, 1e-5)
    if residual:
        out = out + ra
    if relu:
        out = torch.relu(out)
    mean = out.mean((2, 3))
    torch.autograd.backward([out, mean], [dy, dm])                  # both gradients flow
    y, m, _pre, sm, si, rm2, rv2, nbt = R.forward(x, w0, b0, rm0, rv0, torch.tensor(5), res if residual else None, training, 0.1,
                                                  1e-5, relu)
    dx, dw, db, dres = R.backward(dy, dm, x, y, w0, sm, si, training, relu, bool(residual))
    assert int(nbt) == 5 + int(training) and m.shape == (B, C)
    pairs = [(y, out.detach()), (m, mean.detach()), (rm2, rm), (rv2, rv), (dx, xa.grad), (dw, w.grad), (db, b.grad)]
    if residual:
        pairs.append((dres, ra.grad))
    else:
        assert dres is None
    for i, (a, t) in enumerate(pairs):
        assert _rel(a, t) <= 1e-12, (i, _rel(a, t))
    # one side alone: the other gradient is absent, not zero
    only_m = R.backward(None, dm, x, y, w0, sm, si, training, relu, bool(residual))
    zeros = R.backward(torch.zeros_like(dy), dm, x, y, w0, sm, si, training, relu, bool(residual))
    only_y = R.backward(dy, None, x, y, w0, sm, si, training, relu, bool(residual))
    plain = trunknorm_ref.backward(dy, x, y, w0, sm, si, training, relu, bool(residual))
    for a, t in list(zip(only_m, zeros)) + list(zip(only_y, plain)):
        assert (a is None and t is None) or torch.equal(a, t)


def test_header_declares_the_entry_points_and_the_library_exports_them():
    import vpn_amd._lib as lib
    _v, _i, _f, _z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert lib.SIGNATURES['vpn_bn_tail_workspace'] == (_z, [_i, _i, _i, _i])
    assert lib.SIGNATURES['vpn_bn_tail_fwd'] == (_i, [_v] * 7 + [_i] * 5 + [_f, _f, _i] + [_v] * 5 + [_z, _v])
    assert lib.SIGNATURES['vpn_bn_tail_bwd'] == (_i, [_v] * 7 + [_i] * 5 + [_f, _i] + [_v] * 5 + [_z, _v])
    # the existing entries of the ring are as they were
    assert lib.SIGNATURES['vpn_bn_act_fwd'] == (_i, [_v] * 7 + [_i] * 5 + [_f, _f, _i] + [_v] * 4 + [_z, _v])
    assert lib.SIGNATURES['vpn_bn_act_bwd'] == (_i, [_v] * 6 + [_i] * 5 + [_f, _i] + [_v] * 5 + [_z, _v])
    L = lib.lib()
    for name in ('vpn_bn_tail_fwd', 'vpn_bn_tail_bwd', 'vpn_bn_tail_workspace'):
        assert hasattr(L, name), name
    assert L.vpn_abi_version() == lib.ABI_VERSION == 9              # entries were added, none changed


def test_shape_validation_and_workspace_need_no_gpu():
    import vpn_amd._lib as lib
    L = lib.lib()
    bad, big, sl = lib.CONSTANTS['VPN_E_BADARG'], lib.CONSTANTS['VPN_E_TOOBIG'], lib.CONSTANTS['VPN_BN_SLICE']
    for shape in SHAPES + [(2, 8, 64, 64), (1, 3, 90, 91), (0, 3, 4, 4), (65536, 1, 1025, 1)]:
        assert L.vpn_bn_tail_workspace(*shape) == (0 if shape[0] == 65536 else L.vpn_bn_act_workspace(*shape)), shape
    assert L.vpn_bn_tail_workspace(2, 8, 64, 64) == 0 and L.vpn_bn_tail_workspace(2, 3, 64, 65) == 3 * -(-2 * 64 * 65 // sl) * 8
    buf = (ctypes.c_float * 64)()              # host memory standing in for tensors: validation never reads them
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(x=p, B=2, C=1, H=2, W=2, training=1, momentum=0.1, eps=1e-5, ws=None, wsb=0, rm=p, y=p, m=p, sm=p):
        return L.vpn_bn_tail_fwd(x, p, p, p, rm, p, p, B, C, H, W, training, momentum, eps, 1, y, m, sm, p, ws, wsb, None)
    assert fwd(m=None) == bad and fwd(m=None, training=0) == bad
    assert fwd(x=None) == bad and fwd(y=None) == bad and fwd(B=0) == bad and fwd(C=-1) == bad and fwd(eps=-1.0) == bad
    assert fwd(momentum=1.5) == bad and fwd(B=1, H=1, W=1) == bad and fwd(training=0, rm=None) == bad and fwd(sm=None) == bad
    assert fwd(B=4, H=64, W=64) == bad and fwd(B=4, H=64, W=64, ws=p, wsb=8) == bad     # two-launch regime: workspace
    # rows longer than half a slice: one batch row per workgroup of the apply launch, so B is the grid's second dimension
    assert fwd(B=65536, H=1025, W=1, ws=p, wsb=1 << 30) == big and fwd(B=65536, H=1025, W=1, training=0) == big
    assert fwd(B=65536, H=2048, W=1, ws=p, wsb=64) == big                                 # more than 65535 slices

    def bwd(dy=p, dm=p, x=p, y=p, B=2, H=2, W=2, dx=p, dres=p, dw=p, db=p, ws=None, wsb=0, training=1, relu=1):
        return L.vpn_bn_tail_bwd(dy, dm, x, y, p, p, p, B, 1, H, W, training, 1e-5, relu, dx, dres, dw, db, ws, wsb, None)
    assert bwd(dy=None, dm=None) == bad and bwd(x=None) == bad and bwd(y=None) == bad and bwd(B=1, H=1, W=1) == bad
    assert bwd(B=4, H=64, W=64) == bad and bwd(B=4, H=64, W=64, ws=p, wsb=8) == bad
    assert bwd(B=65536, H=1025, W=1) == big
    for kw in (dict(), dict(dy=None), dict(dm=None), dict(B=4, H=64, W=64)):             # nothing wanted: nothing launched
        assert bwd(dx=None, dres=None, dw=None, db=None, **kw) == 0


def test_fused_tail_trunk_has_the_same_state_dict_and_the_keyword_is_independent():
    from vpn_amd.modules.network import ResNet18
    torch.manual_seed(0)
    plain, fused = ResNet18(), ResNet18(fused_tail=True)
    sp, sf = plain.state_dict(), fused.state_dict()
    assert len(sp) == 122 and list(sp) == list(sf)
    assert all(sp[k].shape == sf[k].shape and sp[k].dtype == sf[k].dtype for k in sp)
    fused.load_state_dict(sp, strict=True)
    plain.load_state_dict(fused.state_dict(), strict=True)
    assert fused.fused_tail and not plain.fused_tail and isinstance(fused.avgpool, nn.AdaptiveAvgPool2d)
    assert not (fused.fused_norm or fused.fused_pool or fused.hip_conv or fused.hip_conv_strided)
    for f, c, s, q, t in itertools.product((False, True), repeat=5):
        net = ResNet18(fused_norm=f, hip_conv=c, hip_conv_strided=s, fused_pool=q, fused_tail=t)
        assert (net.fused_norm, bool(net.hip_conv), net.hip_conv_strided, net.fused_pool, net.fused_tail) == (f, c, s, q, t)
        assert list(net.state_dict()) == list(sp)
        assert all(b.fused_norm == f for b in net.layer4)


class _NoCall(nn.Module):
    def forward(self, x):
        raise AssertionError('the pool was called')


def test_pools_the_tail_accepts():
    from vpn_amd.modules.network import ResNet18, SDNet, VPNetOneRes, _is_tail_pool, _trunk_features, _trunk_maps
    assert _is_tail_pool(nn.AdaptiveAvgPool2d(1)) and _is_tail_pool(nn.AdaptiveAvgPool2d((1, 1)))
    assert _is_tail_pool(nn.Sequential(nn.AdaptiveAvgPool2d(output_size=(1, 1))))
    for foreign in (nn.AdaptiveAvgPool2d(2), nn.AdaptiveAvgPool2d((1, 2)), nn.AdaptiveMaxPool2d(1), nn.AvgPool2d(4), nn.Identity(),
                    nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Identity()), nn.Sequential(), nn.Sequential(nn.AvgPool2d(4))):
        assert not _is_tail_pool(foreign), foreign
    fused = ResNet18(fused_tail=True)
    fused.avgpool = nn.AvgPool2d(2)                   # any other pool is refused, not handed to ATen
    with pytest.raises(ValueError, match='AdaptiveAvgPool2d to 1x1 only'):
        fused._layer4_tail(torch.zeros(1, 256, 4, 4))
    with pytest.raises(ValueError, match='AdaptiveAvgPool2d to 1x1 only'):
        fused(torch.zeros(1, 3, 32, 32))
    sd = SDNet(trunk=ResNet18(fused_tail=True))       # SDNet replaces the trunk's pool by a Sequential of one: accepted
    assert isinstance(sd._model.avgpool, nn.Sequential) and _is_tail_pool(sd._model.avgpool)
    vp = VPNetOneRes(vp_num=2, trunk=ResNet18(fused_tail=True))
    vp.avgpool = _NoCall()
    with pytest.raises(ValueError, match='AdaptiveAvgPool2d to 1x1 only'):          # the model's own pool, before anything runs
        vp.extract_feature(torch.zeros(1, 3, 32, 32))
    sd._model.avgpool = nn.Sequential(nn.AvgPool2d(4))
    with pytest.raises(ValueError, match='AdaptiveAvgPool2d to 1x1 only'):
        sd.extract_feature(torch.zeros(1, 3, 32, 32))
    # a trunk without fused_tail: _trunk_maps and the pool itself
    plain = ResNet18().eval()
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        maps, feats = _trunk_features(plain, x)
        ref = _trunk_maps(plain, x)
        assert all(torch.equal(a, b) for a, b in zip(maps, ref)) and torch.equal(feats, torch.flatten(plain.avgpool(ref[3]), 1))
        assert feats.shape == (1, 512)


def test_the_op_refuses_cpu_tensors_before_any_launch(monkeypatch):
    import vpn_amd
    from vpn_amd import _lib

    def no_library(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'call', no_library)
    monkeypatch.setattr(_lib, 'lib', no_library)
    bn = nn.BatchNorm2d(3)
    with pytest.raises(ValueError, match='GPU only'):
        vpn_amd.batch_norm_act_mean(torch.randn(2, 3, 4, 4), bn)
    with pytest.raises(NotImplementedError, match='fp32'):
        vpn_amd.batch_norm_act_mean(torch.randn(2, 3, 4, 4).double(), bn)
    with pytest.raises(ValueError, match='GPU only'):
        vpn_amd.BatchNormMeanFunction.apply(torch.randn(2, 3, 4, 4), None, None, bn.running_mean, bn.running_var, None, None, True,
                                            0.1, 1e-5, True)
    assert int(bn.num_batches_tracked) == 0


@pytest.mark.parametrize('name', ['train_step.py', 'train_sphere_step.py', 'train_gcn_step.py'])
def test_examples_take_the_tail_switch(name):
    """Every example lists --trunk-tail torch|hip, default torch, and maps it to fused_tail (read from the source: the
    examples need a GPU to run)."""
    src = open(os.path.join(ROOT, 'examples', name)).read()
    calls = [n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.Call) and getattr(n.func, 'attr', '') == 'add_argument'
             and n.args and getattr(n.args[0], 'value', None) == '--trunk-tail']
    assert len(calls) == 1
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--trunk-tail', **{k.arg: ast.literal_eval(k.value) for k in calls[0].keywords})
    assert ap.parse_args([]).trunk_tail == 'torch'
    for v in ('torch', 'hip'):
        assert ap.parse_args(['--trunk-tail', v]).trunk_tail == v
    with pytest.raises(SystemExit):
        ap.parse_args(['--trunk-tail', 'aten'])
    assert "fused_tail=args.trunk_tail == 'hip'" in src
    assert "(args.trunk_norm, args.trunk_conv, args.trunk_tail) != ('torch', 'torch', 'torch')" in src      # alone it selects the project's trunk
