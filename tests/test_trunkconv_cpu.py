"""CPU-only checks of the trunk's 3x3 convolution (csrc/trunkconv.hip, ops.Conv3x3Function, ResNet18(hip_conv); DESIGN.md
4.19): the C ABI and its published constants, every rejection before any HIP call, the host rule for the slices, the
restatement tests/trunkconv_ref.py against torch's own convolution and autograd in float64, the state_dict of the trunk, and
the kernels' scratch."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from kernel_resources import kernel_resources, load_build
import trunkconv_ref as R

TILE_CONSTANTS = ('VPN_CONV_TILE', 'VPN_CONV_TILE_K', 'VPN_CONV_SPLIT_TARGET', 'VPN_CONV_MAX_SPLIT')


def test_header_declares_the_entry_points_and_the_library_exports_them():
    b = load_build()
    assert 'trunkconv.hip' in b.SOURCES
    import vpn_amd
    import vpn_amd._lib as lib
    from vpn_amd import ops
    _v, _i, _z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert lib.SIGNATURES['vpn_conv3x3_workspace'] == (_z, [_i] * 6)
    assert lib.SIGNATURES['vpn_conv3x3_splits'] == (_i, [_i] * 6)
    assert lib.SIGNATURES['vpn_conv3x3_fwd'] == (_i, [_v] * 3 + [_i] * 5 + [_v, _z, _v])
    assert lib.SIGNATURES['vpn_conv3x3_bwd'] == (_i, [_v] * 5 + [_i] * 5 + [_v, _z, _v])
    L = ctypes.CDLL(b.build(verbose=False))
    for name in ('vpn_conv3x3_fwd', 'vpn_conv3x3_bwd', 'vpn_conv3x3_workspace', 'vpn_conv3x3_splits'):
        assert hasattr(L, name), name
    assert lib.lib().vpn_abi_version() == lib.ABI_VERSION == 9          # entries were added, none changed
    c = lib.CONSTANTS
    assert all(c[k] > 0 for k in TILE_CONSTANTS)
    assert c['VPN_CONV_TILE'] % 32 == 0 and c['VPN_CONV_TILE_K'] % 2 == 0          # whole 32x32x2 MFMA tiles and steps
    assert (c['VPN_CONV_FWD'], c['VPN_CONV_DX'], c['VPN_CONV_DW']) == (1, 2, 4)
    assert (ops.CONV_TILE, ops.CONV_TILE_K, ops.CONV_SPLIT_TARGET, ops.CONV_MAX_SPLIT) == tuple(c[k] for k in TILE_CONSTANTS)
    assert vpn_amd.conv3x3 is vpn_amd.modules.network.conv3x3 and callable(ops.Conv3x3Function.apply)


def test_host_rule_for_the_slices_and_the_workspace():
    import vpn_amd._lib as lib
    from vpn_amd import ops
    L = lib.lib()
    T, TK, target, smax = (lib.CONSTANTS[k] for k in TILE_CONSTANTS)
    shapes = [(1, 1, 1, 1, 1), (2, 5, 7, 5, 3), (3, 19, 33, 7, 9), (1, 3, 130, 2, 67), (2, 70, 6, 1, 33), (2, 6, 70, 33, 1),
              (8, 64, 64, 32, 32), (8, 128, 128, 16, 16), (8, 256, 256, 8, 8), (8, 512, 512, 4, 4), (64, 64, 64, 32, 32),
              (64, 512, 512, 4, 4), (1, 2, 2, 128, 128), (1, 114, 1024, 3, 6)]
    for s in shapes:
        B, Ci, Co, H, W = s
        outs = {ops.CONV_FWD: B * Co * H * W, ops.CONV_DX: B * Ci * H * W, ops.CONV_DW: Co * Ci * 9}
        need = {}
        for product, n in outs.items():
            S = ops.conv3x3_splits(*s, product)
            assert L.vpn_conv3x3_splits(*s, product) == S and 1 <= S <= smax, (s, product)
            need[product] = S * n * 4 if S > 1 else 0
            assert L.vpn_conv3x3_workspace(*s, product) == need[product], (s, product)
        assert L.vpn_conv3x3_workspace(*s, ops.CONV_DX | ops.CONV_DW) == max(need[ops.CONV_DX], need[ops.CONV_DW])
        assert L.vpn_conv3x3_workspace(*s, 0) == 0
    # layer4 forward at B = 8: 8 x 2 tiles, 16 slices of 18 chunks; layer1 at B = 64: 1024 tiles, unsplit
    assert ops.conv3x3_splits(8, 512, 512, 4, 4, ops.CONV_FWD) == target // 16
    assert ops.conv3x3_splits(64, 64, 64, 32, 32, ops.CONV_FWD) == 1 and L.vpn_conv3x3_workspace(64, 64, 64, 32, 32, 1) == 0
    assert L.vpn_conv3x3_splits(2, 5, 7, 5, 3, 3) == lib.CONSTANTS['VPN_E_BADARG']          # one product at a time
    assert L.vpn_conv3x3_workspace(0, 1, 1, 1, 1, 7) == 0


def test_every_rejection_comes_before_any_hip_call():
    """On a machine without a GPU a HIP call would fail with a positive HIP error: every code below is the entry's own."""
    import vpn_amd._lib as lib
    L = lib.lib()
    bad, big = lib.CONSTANTS['VPN_E_BADARG'], lib.CONSTANTS['VPN_E_TOOBIG']
    buf = (ctypes.c_float * 64)()              # host memory standing in for tensors: validation never reads them
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 16 == 0
    off = ctypes.c_void_p(p.value + 4)

    def fwd(x=p, w=p, y=p, B=1, Ci=1, Co=1, H=1, W=1, ws=None, wsb=0):
        return L.vpn_conv3x3_fwd(x, w, y, B, Ci, Co, H, W, ws, wsb, None)

    def bwd(dy=p, x=p, w=p, dx=p, dw=p, B=1, Ci=1, Co=1, H=1, W=1, ws=None, wsb=0):
        return L.vpn_conv3x3_bwd(dy, x, w, dx, dw, B, Ci, Co, H, W, ws, wsb, None)

    split = dict(B=2, Ci=5, Co=7, H=5, W=3)                   # one tile, three chunks or more in every product: split
    assert all(L.vpn_conv3x3_splits(2, 5, 7, 5, 3, k) > 1 for k in (1, 2, 4))
    # null pointers and non-positive sizes
    assert fwd(x=None) == bad and fwd(w=None) == bad and fwd(y=None) == bad
    assert bwd(dy=None) == bad and bwd(x=None) == bad and bwd(w=None) == bad
    for k in ('B', 'Ci', 'Co', 'H', 'W'):
        assert fwd(**{k: 0}) == bad and fwd(**{k: -3}) == bad and bwd(**{k: 0}) == bad, k
    # a workspace that is needed and missing, too small or misaligned
    need_f = L.vpn_conv3x3_workspace(2, 5, 7, 5, 3, 1)
    need_b = L.vpn_conv3x3_workspace(2, 5, 7, 5, 3, 6)
    assert need_f > 0 and need_b > 0
    assert fwd(**split) == bad and fwd(ws=p, wsb=need_f - 4, **split) == bad and fwd(ws=off, wsb=1 << 20, **split) == bad
    assert bwd(**split) == bad and bwd(ws=p, wsb=need_b - 4, **split) == bad and bwd(ws=off, wsb=1 << 20, **split) == bad
    assert bwd(dw=None, ws=p, wsb=L.vpn_conv3x3_workspace(2, 5, 7, 5, 3, 2) - 4, **split) == bad
    assert bwd(dx=None, ws=p, wsb=L.vpn_conv3x3_workspace(2, 5, 7, 5, 3, 4) - 4, **split) == bad
    # nothing wanted: nothing launched, whatever the workspace
    assert bwd(dx=None, dw=None, **split) == 0 and bwd(dx=None, dw=None) == 0
    # 2^31 elements or more in x, y or w; more than 65535 tiles along M
    assert fwd(B=2 ** 15, Ci=1, Co=1, H=2 ** 8, W=2 ** 8, ws=p, wsb=64) == big                  # x and y: 2^31
    assert fwd(B=2 ** 10, Ci=2 ** 5, Co=1, H=2 ** 8, W=2 ** 8, ws=p, wsb=64) == big             # x alone
    assert bwd(B=2 ** 10, Ci=1, Co=2 ** 5, H=2 ** 8, W=2 ** 8, ws=p, wsb=64) == big             # y alone
    assert fwd(Ci=2 ** 14, Co=2 ** 14, ws=p, wsb=64) == big and bwd(Ci=2 ** 14, Co=2 ** 14, ws=p, wsb=64) == big      # w: 9 * 2^28
    assert fwd(Co=65536 * 64, ws=p, wsb=64) == big and bwd(Ci=65536 * 64, ws=p, wsb=64) == big  # gridDim.y
    assert L.vpn_conv3x3_splits(1, 1, 65536 * 64, 1, 1, 1) == big
    assert fwd(H=2 ** 20, W=2 ** 20) == big


@pytest.mark.parametrize('shape', [(1, 1, 1, 1, 1), (2, 5, 7, 5, 3), (3, 19, 33, 7, 9), (1, 3, 13, 2, 17), (2, 7, 6, 1, 33),
                                   (2, 6, 7, 33, 1)])
def test_restatement_equals_torch_in_float64(shape):
    B, Ci, Co, H, W = shape
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Co, Ci, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, Co, H, W, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, None, 1, 1)
    y.backward(dy)
    ry = R.forward(x.detach(), w.detach())
    rdx, rdw = R.backward(dy, x.detach(), w.detach())
    for name, a, t in (('y', ry, y.detach()), ('dx', rdx, x.grad), ('dw', rdw, w.grad)):
        err = float((a - t).abs().max() / t.abs().max().clamp_min(1e-300))
        assert err <= 1e-12, (name, err)


def test_hip_conv_trunk_has_the_same_state_dict():
    from vpn_amd.modules.network import ResNet18, BasicBlock
    torch.manual_seed(0)
    plain, hip, both = ResNet18(), ResNet18(hip_conv=True), ResNet18(fused_norm=True, hip_conv=('layer4', 'layer2'))
    sp = plain.state_dict()
    for m in (hip, both):
        sm = m.state_dict()
        assert len(sp) == 122 and list(sp) == list(sm)
        assert all(sp[k].shape == sm[k].shape and sp[k].dtype == sm[k].dtype for k in sp)
        m.load_state_dict(sp, strict=True)
        plain.load_state_dict(m.state_dict(), strict=True)
        assert all(torch.equal(m.state_dict()[k], sp[k]) for k in sp)
    assert plain.hip_conv == () and not plain.fused_norm and not hip.fused_norm and both.fused_norm
    assert hip.hip_conv == ('layer1', 'layer2', 'layer3', 'layer4') and both.hip_conv == ('layer2', 'layer4')
    assert ResNet18(hip_conv='layer3').hip_conv == ('layer3',) and ResNet18(hip_conv=[]).hip_conv == ()
    with pytest.raises(ValueError, match='hip_conv'):
        ResNet18(hip_conv=('layer5',))
    assert all(m.hip_conv for m in hip.modules() if isinstance(m, BasicBlock))
    assert [n for n, m in both.named_modules() if isinstance(m, BasicBlock) and m.hip_conv] == ['layer2.0', 'layer2.1', 'layer4.0', 'layer4.1']
    # the modules that would take the new path: 13 convolutions with kernel 3, stride 1, padding 1
    from vpn_amd.modules.network import _is_trunk_conv3x3
    routed = [n for n, m in hip.named_modules() if isinstance(m, torch.nn.Conv2d) and n.startswith('layer') and _is_trunk_conv3x3(m)]
    assert len(routed) == 13 and 'layer2.0.conv1' not in routed and not any('downsample' in n for n in routed)
    assert not _is_trunk_conv3x3(hip.conv1)


def test_every_refusal_of_the_function_is_raised_before_any_launch(monkeypatch):
    import vpn_amd
    from vpn_amd import ops, _lib

    def no_library(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'call', no_library)
    monkeypatch.setattr(_lib, 'lib', no_library)
    x, w = torch.randn(2, 3, 4, 4), torch.randn(5, 3, 3, 3)
    with pytest.raises(ValueError, match='B, C_in, H, W'):
        vpn_amd.conv3x3(x[0], w)
    with pytest.raises(ValueError, match='C_out, C_in, 3, 3'):
        vpn_amd.conv3x3(x, torch.randn(5, 3, 1, 1))
    with pytest.raises(ValueError, match='input channels'):
        vpn_amd.conv3x3(x, torch.randn(5, 4, 3, 3))
    with pytest.raises(NotImplementedError, match='fp32'):
        ops.Conv3x3Function.apply(x.double(), w.double())
    with pytest.raises(NotImplementedError, match='fp32'):
        ops.Conv3x3Function.apply(x, w.half())
    with pytest.raises(ValueError, match='empty'):
        vpn_amd.conv3x3(x[:0], w)
    with pytest.raises(ValueError, match='GPU only'):
        vpn_amd.conv3x3(x, w)


def test_trunkconv_compiles_as_build_py_compiles_it_without_scratch():
    rows = kernel_resources('trunkconv.hip')
    kernels = {k: v for k, v in rows.items() if 'cv_gemm_kernel' in k or 'cg_merge_kernel' in k}
    assert len(kernels) == len(rows) == 4, list(rows)          # the GEMM kernel for data and weights, the merge by 4 and by 1
    assert sum('cv_gemm_kernel' in k for k in kernels) == 2 and sum('cg_merge_kernel' in k for k in kernels) == 2
    for k, v in kernels.items():
        assert v['ScratchSize'] == 0, (k, v)
        assert v['LDS'] <= 64 * 1024, (k, v)
    assert all(v['AGPRs'] + v['VGPRs'] <= 128 for v in kernels.values()), kernels          # four waves per SIMD fit
