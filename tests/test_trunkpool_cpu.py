"""CPU-only checks of the stem's pool op (the tp_ kernels of csrc/trunknorm.hip, ops.BatchNormPoolFunction,
ResNet18(fused_pool)): the restatement tests/trunkpool_ref.py against torch's own batch norm, ReLU, max pool
and autograd in float64, the size rule, the C ABI, the state_dict of the trunk and the examples' switch."""
import ast
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
import trunkpool_ref as R

SHAPES = [(2, 3, 5, 7), (3, 64, 4, 4), (2, 4, 8, 8), (2, 5, 16, 16), (1, 4, 19, 27), (2, 2, 64, 64), (1, 3, 90, 91), (2, 3, 64, 65),
          (3, 2, 53, 53), (3, 2, 40, 40), (2, 64, 32, 32), (2, 2, 2, 3)]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('shape', SHAPES)
def test_restatement_equals_torch_in_float64(shape, training):
    g = torch.Generator().manual_seed(11)
    B, C, H, W = shape
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    dp = torch.randn((B, C) + R.out_size(H, W), generator=g, dtype=torch.float64)
    w0, b0 = 1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64), 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    rm0, rv0 = 0.1 * torch.randn(C, generator=g, dtype=torch.float64), 1 + 0.2 * torch.rand(C, generator=g, dtype=torch.float64)
    xa, w, b = x.clone().requires_grad_(True), w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    rm, rv = rm0.clone(), rv0.clone()
    out, flat = F.max_pool2d(torch.relu(F.batch_norm(xa, rm, rv, w, b, training, 0.1, 1e-5)), 3, 2, 1, return_indices=True)
    out.backward(dp)
    p, idx, _pre, mean, invstd, rm2, rv2, nbt = R.forward(x, w0, b0, rm0, rv0, torch.tensor(5), training, 0.1, 1e-5)
    dx, dw, db = R.backward(dp, x, p, idx, w0, mean, invstd, training)
    assert int(nbt) == 5 + int(training) and idx.dtype == torch.uint8 and int(idx.max()) <= 8
    assert torch.equal(idx, R.taps_from_flat(flat, H, W)) and torch.equal(R.flat_from_taps(idx, H, W), flat)
    for i, (a, t) in enumerate([(p, out.detach()), (rm2, rm), (rv2, rv), (dx, xa.grad), (dw, w.grad), (db, b.grad)]):
        assert _rel(a, t) <= 1e-12, (i, _rel(a, t))


def test_exact_ties_keep_the_first_tap():
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 3, 6, 7), generator=g, dtype=torch.float64).repeat_interleave(2, 2).repeat_interleave(2, 3)
    p, flat = F.max_pool2d(torch.relu(x), 3, 2, 1, return_indices=True)
    best, idx = R.first_max(R.taps(torch.relu(x)))
    assert torch.equal(best, p) and torch.equal(idx, R.taps_from_flat(flat, 12, 14))


def test_pool_out_size_is_max_pool2ds():
    from vpn_amd import ops
    for H in range(1, 13):
        for W in range(1, 13):
            assert ops.pool_out_size(H, W) == tuple(F.max_pool2d(torch.zeros(1, 1, H, W), 3, 2, 1).shape[2:]) == R.out_size(H, W)


def test_header_declares_the_entry_points_and_the_library_exports_them():
    import vpn_amd._lib as lib
    _v, _i, _f, _z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert lib.SIGNATURES['vpn_bn_pool_workspace'] == (_z, [_i, _i, _i, _i])
    assert lib.SIGNATURES['vpn_bn_pool_fwd'] == (_i, [_v] * 6 + [_i] * 5 + [_f, _f] + [_v] * 5 + [_z, _v])
    assert lib.SIGNATURES['vpn_bn_pool_bwd'] == (_i, [_v] * 7 + [_i] * 5 + [_f] + [_v] * 4 + [_z, _v])
    L = lib.lib()
    for name in ('vpn_bn_pool_fwd', 'vpn_bn_pool_bwd', 'vpn_bn_pool_workspace'):
        assert hasattr(L, name), name
    assert L.vpn_abi_version() == lib.ABI_VERSION == 9              # entries were added, none changed
    assert lib.CONSTANTS['VPN_BN_POOL_SLICE'] == 512


def test_shape_validation_and_workspace_need_no_gpu():
    import vpn_amd._lib as lib
    L = lib.lib()
    bad, big, sl = lib.CONSTANTS['VPN_E_BADARG'], lib.CONSTANTS['VPN_E_TOOBIG'], lib.CONSTANTS['VPN_BN_SLICE']
    assert L.vpn_bn_pool_workspace(2, 8, 64, 64) == 8 * 4 * 8 and L.vpn_bn_pool_workspace(2, 3, 64, 65) == 3 * -(-2 * 64 * 65 // sl) * 8
    assert L.vpn_bn_pool_workspace(0, 3, 4, 4) == 0
    buf = (ctypes.c_float * 64)()              # host memory standing in for tensors: validation never reads them
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(x=p, B=2, C=1, H=2, W=2, training=1, momentum=0.1, eps=1e-5, ws=None, wsb=0, rm=p, idx=p):
        return L.vpn_bn_pool_fwd(x, p, p, rm, p, p, B, C, H, W, training, momentum, eps, p, idx, p, p, ws, wsb, None)
    assert fwd(x=None) == bad and fwd(idx=None) == bad and fwd(B=0) == bad and fwd(C=-1) == bad and fwd(eps=-1.0) == bad
    assert fwd(momentum=1.5) == bad and fwd(B=1, H=1, W=1) == bad and fwd(training=0, rm=None) == bad
    assert fwd(B=4, H=64, W=64) == bad and fwd(B=4, H=64, W=64, ws=p, wsb=8) == bad     # two-launch regime: workspace
    assert fwd(B=65536, H=2048, W=1, ws=p, wsb=64) == big and fwd(B=65535 * 512 + 1, H=1, W=1, training=0) == big

    def bwd(dp=p, idx=p, B=2, H=2, W=2, dx=p, dw=p, db=p, ws=p, wsb=64, training=1):
        return L.vpn_bn_pool_bwd(dp, p, p, idx, p, p, p, B, 1, H, W, training, 1e-5, dx, dw, db, ws, wsb, None)
    assert bwd(dp=None) == bad and bwd(idx=None) == bad and bwd(ws=None, wsb=0) == bad and bwd(wsb=4) == bad
    assert bwd(B=1, H=1, W=1) == bad and bwd(B=65536, H=2048, W=1) == big
    assert bwd(dx=None, dw=None, db=None, ws=None, wsb=0) == 0                           # nothing wanted


def test_fused_pool_trunk_has_the_same_state_dict():
    from vpn_amd.modules.network import ResNet18
    torch.manual_seed(0)
    plain, fused = ResNet18(), ResNet18(fused_pool=True)
    sp, sf = plain.state_dict(), fused.state_dict()
    assert len(sp) == 122 and list(sp) == list(sf)
    assert all(sp[k].shape == sf[k].shape and sp[k].dtype == sf[k].dtype for k in sp)
    fused.load_state_dict(sp, strict=True)
    plain.load_state_dict(fused.state_dict(), strict=True)
    assert fused.fused_pool and not fused.fused_norm and not plain.fused_pool and not ResNet18(fused_norm=True).fused_pool
    assert isinstance(fused.maxpool, torch.nn.MaxPool2d)
    both = ResNet18(fused_norm=True, hip_conv=True, hip_conv_strided=True, fused_pool=True)
    assert both.fused_norm and both.fused_pool and list(both.state_dict()) == list(sp)
    fused.maxpool = torch.nn.MaxPool2d(2, 2)                   # any other pool is refused, not handed to ATen
    with pytest.raises(ValueError, match='MaxPool2d\\(3, 2, 1\\) only'):
        fused._stem_tail(torch.zeros(1, 64, 4, 4))


def test_the_op_refuses_cpu_tensors_before_any_launch(monkeypatch):
    import vpn_amd
    from vpn_amd import _lib

    def no_library(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'call', no_library)
    monkeypatch.setattr(_lib, 'lib', no_library)
    bn = torch.nn.BatchNorm2d(3)
    with pytest.raises(ValueError, match='GPU only'):
        vpn_amd.batch_norm_relu_pool(torch.randn(2, 3, 4, 4), bn)
    with pytest.raises(NotImplementedError, match='fp32'):
        vpn_amd.batch_norm_relu_pool(torch.randn(2, 3, 4, 4).double(), bn)
    assert int(bn.num_batches_tracked) == 0


@pytest.mark.parametrize('name', ['train_step.py', 'train_sphere_step.py', 'train_gcn_step.py'])
def test_examples_take_the_pool_switch(name):
    """The --trunk-norm argument of every example lists hip+pool and maps it to fused_norm and fused_pool (read from the
    source: the examples need a GPU to run)."""
    src = open(os.path.join(ROOT, 'examples', name)).read()
    calls = [n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.Call) and getattr(n.func, 'attr', '') == 'add_argument'
             and n.args and getattr(n.args[0], 'value', None) == '--trunk-norm']
    assert len(calls) == 1
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--trunk-norm', **{k.arg: ast.literal_eval(k.value) for k in calls[0].keywords})
    assert ap.parse_args([]).trunk_norm == 'torch'
    for v in ('torch', 'hip', 'hip+pool'):
        assert ap.parse_args(['--trunk-norm', v]).trunk_norm == v
    assert "fused_norm=args.trunk_norm != 'torch'" in src and "fused_pool=args.trunk_norm == 'hip+pool'" in src
