"""CPU-only checks of the trunk's strided convolutions (csrc/trunkstride.hip, ops.Conv2dFunction, vpn_amd.conv2d,
ResNet18(hip_conv_strided)): the C ABI, every rejection before any HIP call, the host rule for the slices
(held to the 3x3 rule where the two overlap), the restatement tests/trunkstride_ref.py against torch's own convolution and
autograd in float64, the state_dict and the routing of the trunk, and the kernels' resources."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from kernel_resources import kernel_resources, load_build
import trunkstride_ref as R

ENTRIES = ('vpn_conv2d_workspace', 'vpn_conv2d_splits', 'vpn_conv2d_fwd', 'vpn_conv2d_bwd')


def trunk_sites(B, side):
    """(B, C_in, C_out, H, W, R, stride, pad) of the seven stride-2 convolutions of the ResNet-18 trunk for a side x side
    image: the stem, then conv1 and the downsample of the first block of layer2, layer3 and layer4."""
    out = [(B, 3, 64, side, side, 7, 2, 3)]
    for i, c in enumerate((64, 128, 256)):
        s = side // (4 << i)
        out += [(B, c, 2 * c, s, s, 3, 2, 1), (B, c, 2 * c, s, s, 1, 2, 0)]
    return out


ODD = [(1, 1, 1, 1, 1, 1, 2, 0), (1, 1, 1, 1, 1, 3, 2, 1), (1, 2, 3, 2, 2, 7, 2, 3), (2, 3, 5, 9, 11, 7, 2, 3), (2, 5, 7, 6, 5, 3, 2, 1),
       (2, 6, 7, 8, 8, 1, 2, 0), (1, 4, 65, 16, 16, 3, 2, 1), (3, 19, 33, 7, 9, 3, 3, 0), (2, 5, 7, 5, 3, 3, 1, 1), (2, 5, 7, 5, 3, 1, 1, 0),
       (1, 3, 130, 2, 67, 7, 1, 5), (4, 3, 64, 128, 128, 7, 2, 3)]


def test_header_declares_the_entry_points_and_the_library_exports_them():
    b = load_build()
    assert 'trunkstride.hip' in b.SOURCES
    import vpn_amd
    import vpn_amd._lib as lib
    from vpn_amd import ops
    _v, _i, _z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert lib.SIGNATURES['vpn_conv2d_workspace'] == (_z, [_i] * 9)
    assert lib.SIGNATURES['vpn_conv2d_splits'] == (_i, [_i] * 9)
    assert lib.SIGNATURES['vpn_conv2d_fwd'] == (_i, [_v] * 3 + [_i] * 8 + [_v, _z, _v])
    assert lib.SIGNATURES['vpn_conv2d_bwd'] == (_i, [_v] * 5 + [_i] * 8 + [_v, _z, _v])
    L = ctypes.CDLL(b.build(verbose=False))
    for name in ENTRIES:
        assert hasattr(L, name), name
    assert lib.lib().vpn_abi_version() == lib.ABI_VERSION == 9          # entries were added, none changed
    assert vpn_amd.conv2d is vpn_amd.modules.network.conv2d and callable(ops.Conv2dFunction.apply)
    assert ops.CONV2D_KERNELS == (1, 3, 7)


def test_host_rule_for_the_slices_and_the_workspace():
    import vpn_amd._lib as lib
    from vpn_amd import ops
    L = lib.lib()
    smax = lib.CONSTANTS['VPN_CONV_MAX_SPLIT']
    shapes = trunk_sites(8, 128) + trunk_sites(64, 128) + ODD
    assert len(trunk_sites(8, 128)) == 7
    for s in shapes:
        B, Ci, Co, H, W, k, st, p = s
        OH, OW = ops.conv2d_out_size(H, W, k, st, p)
        assert (OH, OW) == R.out_size(H, W, k, st, p) and OH >= 1 and OW >= 1
        outs = {ops.CONV_FWD: B * Co * OH * OW, ops.CONV_DX: B * Ci * H * W, ops.CONV_DW: Co * Ci * k * k}
        need = {}
        for product, n in outs.items():
            S = ops.conv2d_splits(*s, product)
            assert L.vpn_conv2d_splits(*s, product) == S and 1 <= S <= smax, (s, product)
            need[product] = S * n * 4 if S > 1 else 0
            assert L.vpn_conv2d_workspace(*s, product) == need[product], (s, product)
        assert L.vpn_conv2d_workspace(*s, ops.CONV_DX | ops.CONV_DW) == max(need[ops.CONV_DX], need[ops.CONV_DW])
        assert L.vpn_conv2d_workspace(*s, 7) == max(need.values())
        assert L.vpn_conv2d_workspace(*s, 0) == 0
    # kernel 3, stride 1, padding 1: the rule of the 3x3 convolutions, slice for slice and byte for byte
    for s in [(1, 1, 1, 1, 1), (2, 5, 7, 5, 3), (3, 19, 33, 7, 9), (1, 3, 130, 2, 67), (8, 64, 64, 32, 32), (8, 512, 512, 4, 4),
              (64, 64, 64, 32, 32), (64, 512, 512, 4, 4), (1, 2, 2, 128, 128), (1, 114, 1024, 3, 6)]:
        for product in (1, 2, 4):
            assert L.vpn_conv2d_splits(*s, 3, 1, 1, product) == L.vpn_conv3x3_splits(*s, product) == ops.conv3x3_splits(*s, product)
        for products in range(8):
            assert L.vpn_conv2d_workspace(*s, 3, 1, 1, products) == L.vpn_conv3x3_workspace(*s, products), (s, products)
    # the real stem at B = 4: 1 x 256 tiles, unsplit; its weight gradient: 1 x 3 tiles, 32 slices
    assert ops.conv2d_splits(4, 3, 64, 128, 128, 7, 2, 3, ops.CONV_FWD) == 1
    assert ops.conv2d_splits(4, 3, 64, 128, 128, 7, 2, 3, ops.CONV_DW) == smax
    assert L.vpn_conv2d_splits(2, 5, 7, 5, 3, 3, 1, 1, 3) == lib.CONSTANTS['VPN_E_BADARG']          # one product at a time
    assert L.vpn_conv2d_workspace(0, 1, 1, 1, 1, 1, 1, 0, 7) == 0 and L.vpn_conv2d_workspace(1, 1, 1, 1, 1, 5, 1, 2, 7) == 0


def test_every_rejection_comes_before_any_hip_call():
    """On a machine without a GPU a HIP call would fail with a positive HIP error: every code below is the entry's own."""
    import vpn_amd._lib as lib
    L = lib.lib()
    bad, big = lib.CONSTANTS['VPN_E_BADARG'], lib.CONSTANTS['VPN_E_TOOBIG']
    buf = (ctypes.c_float * 64)()              # host memory standing in for tensors: validation never reads them
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 16 == 0
    off = ctypes.c_void_p(p.value + 4)

    def fwd(x=p, w=p, y=p, B=1, Ci=1, Co=1, H=1, W=1, R=1, st=1, pad=0, ws=None, wsb=0):
        return L.vpn_conv2d_fwd(x, w, y, B, Ci, Co, H, W, R, st, pad, ws, wsb, None)

    def bwd(dy=p, x=p, w=p, dx=p, dw=p, B=1, Ci=1, Co=1, H=1, W=1, R=1, st=1, pad=0, ws=None, wsb=0):
        return L.vpn_conv2d_bwd(dy, x, w, dx, dw, B, Ci, Co, H, W, R, st, pad, ws, wsb, None)

    def splits(B=1, Ci=1, Co=1, H=1, W=1, R=1, st=1, pad=0, product=1):
        return L.vpn_conv2d_splits(B, Ci, Co, H, W, R, st, pad, product)

    split = dict(B=2, Ci=5, Co=7, H=6, W=5, R=3, st=2, pad=1)            # one tile, three chunks or more in every product: split
    dims = (2, 5, 7, 6, 5, 3, 2, 1)
    assert all(L.vpn_conv2d_splits(*dims, k) > 1 for k in (1, 2, 4))
    # null pointers and non-positive sizes
    assert fwd(x=None) == bad and fwd(w=None) == bad and fwd(y=None) == bad
    assert bwd(dy=None) == bad and bwd(x=None) == bad and bwd(w=None) == bad
    for k in ('B', 'Ci', 'Co', 'H', 'W'):
        assert fwd(**{k: 0}) == bad and fwd(**{k: -3}) == bad and bwd(**{k: 0}) == bad and splits(**{k: 0}) == bad, k
    # the kernel size, the stride, the padding, an image that is smaller than the kernel even when padded
    for k in (0, 2, 4, 5, 6, 8, 9, -3):
        assert fwd(R=k, pad=4, H=9, W=9) == bad and bwd(R=k, pad=4, H=9, W=9) == bad and splits(R=k, pad=4, H=9, W=9) == bad, k
    assert fwd(st=0) == bad and fwd(st=-2) == bad and bwd(st=0) == bad and splits(st=0) == bad
    assert fwd(pad=-1) == bad and bwd(pad=-1) == bad and splits(pad=-1) == bad
    assert fwd(R=3, H=2, W=9) == bad and fwd(R=3, H=9, W=2) == bad and bwd(R=3, H=2, W=9) == bad and bwd(R=7, H=9, W=2, pad=2) == bad
    assert fwd(R=7, H=1, W=1, pad=2) == bad and splits(R=7, H=1, W=1, pad=2) == bad and splits(R=7, H=1, W=1, pad=3) == 4          # 49 taps: four chunks
    # a workspace that is needed and missing, too small or misaligned
    need_f = L.vpn_conv2d_workspace(*dims, 1)
    need_b = L.vpn_conv2d_workspace(*dims, 6)
    assert need_f > 0 and need_b > 0
    assert fwd(**split) == bad and fwd(ws=p, wsb=need_f - 4, **split) == bad and fwd(ws=off, wsb=1 << 20, **split) == bad
    assert bwd(**split) == bad and bwd(ws=p, wsb=need_b - 4, **split) == bad and bwd(ws=off, wsb=1 << 20, **split) == bad
    assert bwd(dw=None, ws=p, wsb=L.vpn_conv2d_workspace(*dims, 2) - 4, **split) == bad
    assert bwd(dx=None, ws=p, wsb=L.vpn_conv2d_workspace(*dims, 4) - 4, **split) == bad
    # nothing wanted: nothing launched, whatever the workspace
    assert bwd(dx=None, dw=None, **split) == 0 and bwd(dx=None, dw=None) == 0
    # 2^31 elements or more in x, y or w; more than 65535 tiles along M
    assert fwd(B=2 ** 15, H=2 ** 8, W=2 ** 8, ws=p, wsb=64) == big                                  # x and y: 2^31
    assert fwd(B=2 ** 10, Ci=2 ** 5, H=2 ** 8, W=2 ** 8, ws=p, wsb=64) == big                       # x alone
    assert bwd(B=2 ** 10, Co=2 ** 5, H=2 ** 8, W=2 ** 8, ws=p, wsb=64) == big                       # y alone
    assert fwd(B=2 ** 13, H=2 ** 8, W=2 ** 8, pad=2 ** 8, ws=p, wsb=64) == big                      # y alone, by the padding
    assert fwd(B=2 ** 15, H=2 ** 8, W=2 ** 8, st=2, ws=p, wsb=64) == big                            # x alone: y is a quarter of it
    assert fwd(Ci=2 ** 14, Co=2 ** 14, R=3, pad=1, ws=p, wsb=64) == big and bwd(Ci=2 ** 14, Co=2 ** 14, R=3, pad=1, ws=p, wsb=64) == big
    assert fwd(Ci=2 ** 13, Co=2 ** 13, R=7, pad=3, ws=p, wsb=64) == big                             # w: 49 * 2^26
    assert fwd(Co=65536 * 64, ws=p, wsb=64) == big and bwd(Ci=65536 * 64, ws=p, wsb=64) == big      # gridDim.y
    assert splits(Co=65536 * 64) == big
    assert fwd(H=2 ** 20, W=2 ** 20) == big
    assert fwd(pad=2 ** 30, st=2 ** 30) == big and splits(pad=2 ** 30, st=2 ** 30) == big           # padded coordinates are ints


@pytest.mark.parametrize('cfg', [(7, 2, 3), (3, 2, 1), (1, 2, 0), (3, 1, 1), (1, 1, 0), (3, 3, 0)], ids=lambda c: 'R%d-s%d-p%d' % c)
def test_restatement_equals_torch_in_float64(cfg):
    k, st, p = cfg
    # (H + 2 p - R) a multiple of the stride and not, in each direction
    for B, Ci, Co, H, W in [(2, 3, 5, 9, 11), (2, 5, 7, 8, 10), (1, 4, 6, 7, 8), (3, 2, 3, 12, 7), (1, 1, 1, max(1, k - 2 * p), max(1, k - 2 * p))]:
        g = torch.Generator().manual_seed(7)
        OH, OW = R.out_size(H, W, k, st, p)
        x = torch.randn(B, Ci, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(Co, Ci, k, k, generator=g, dtype=torch.float64, requires_grad=True)
        dy = torch.randn(B, Co, OH, OW, generator=g, dtype=torch.float64)
        y = F.conv2d(x, w, None, st, p)
        assert tuple(y.shape) == (B, Co, OH, OW)
        y.backward(dy)
        ry = R.forward(x.detach(), w.detach(), st, p)
        rdx, rdw = R.backward(dy, x.detach(), w.detach(), st, p)
        for name, a, t in (('y', ry, y.detach()), ('dx', rdx, x.grad), ('dw', rdw, w.grad)):
            assert a.shape == t.shape
            err = float((a - t).abs().max() / t.abs().max().clamp_min(1e-300))
            assert err <= 1e-12, (name, (B, Ci, Co, H, W), err)
    rem = {((H + 2 * p - k) % st == 0, (W + 2 * p - k) % st == 0) for H, W in ((9, 11), (8, 10), (7, 8), (12, 7))}
    assert st == 1 or len(rem) > 1, rem


def test_restatement_is_the_3x3_restatement_at_stride_1_padding_1():
    import trunkconv_ref as R3
    g = torch.Generator().manual_seed(9)
    x, w, dy = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((2, 5, 5, 3), (7, 5, 3, 3), (2, 7, 5, 3)))
    assert torch.allclose(R.forward(x, w, 1, 1), R3.forward(x, w), rtol=0, atol=1e-13)
    for a, b in zip(R.backward(dy, x, w, 1, 1), R3.backward(dy, x, w)):
        assert torch.allclose(a, b, rtol=0, atol=1e-13)


def test_hip_conv_strided_trunk_has_the_same_state_dict_and_routes_seven_modules():
    from vpn_amd.modules.network import ResNet18, BasicBlock, _is_trunk_conv3x3, _is_trunk_conv_strided
    torch.manual_seed(0)
    plain, strided, both = ResNet18(), ResNet18(hip_conv_strided=True), ResNet18(fused_norm=True, hip_conv=True, hip_conv_strided=True)
    sp = plain.state_dict()
    for m in (strided, both):
        sm = m.state_dict()
        assert len(sp) == 122 and list(sp) == list(sm)
        assert all(sp[k].shape == sm[k].shape and sp[k].dtype == sm[k].dtype for k in sp)
        m.load_state_dict(sp, strict=True)
        plain.load_state_dict(m.state_dict(), strict=True)
        assert all(torch.equal(m.state_dict()[k], sp[k]) for k in sp)
    # independent keywords, unchanged defaults
    assert not plain.hip_conv_strided and plain.hip_conv == () and not plain.fused_norm
    assert strided.hip_conv_strided and strided.hip_conv == () and not strided.fused_norm
    assert both.hip_conv_strided and both.hip_conv == ('layer1', 'layer2', 'layer3', 'layer4') and both.fused_norm
    hip = ResNet18(hip_conv=True)
    assert not hip.hip_conv_strided and not any(m.hip_conv_strided for m in hip.modules() if isinstance(m, BasicBlock))
    assert all(m.hip_conv_strided and not m.hip_conv for m in strided.modules() if isinstance(m, BasicBlock))

    def routed(model):
        """The modules whose forward the trunk replaces, by the predicates its forward uses."""
        out = []
        for n, m in model.named_modules():
            if not isinstance(m, torch.nn.Conv2d):
                continue
            block = model.get_submodule(n.split('.conv')[0].split('.downsample')[0]) if n.startswith('layer') else model
            if n.startswith('layer') and block.hip_conv and _is_trunk_conv3x3(m):
                out.append(n)
            elif block.hip_conv_strided and _is_trunk_conv_strided(m):
                out.append(n)
        return out
    seven = ['conv1'] + [n for i in (2, 3, 4) for n in ('layer%d.0.conv1' % i, 'layer%d.0.downsample.0' % i)]
    assert routed(plain) == [] and routed(strided) == seven
    assert len(routed(hip)) == 13 and not set(routed(hip)) & set(seven)
    assert len(routed(both)) == 20 and set(routed(both)) == set(routed(hip)) | set(seven)
    assert len([m for m in plain.modules() if isinstance(m, torch.nn.Conv2d)]) == 20
    # no module is taken by both predicates
    assert not any(_is_trunk_conv3x3(m) and _is_trunk_conv_strided(m) for m in plain.modules() if isinstance(m, torch.nn.Conv2d))


def test_routed_calls_are_counted_with_the_function_patched(monkeypatch):
    """The forward itself, on the CPU, with both functions replaced by torch's convolution: 7 calls with the strided
    keyword alone, 13 + 7 with both, the result the plain trunk's."""
    from vpn_amd.modules import network
    from vpn_amd.modules.network import ResNet18, _trunk_maps
    calls3, calls2 = [], []

    class Count3:
        @staticmethod
        def apply(x, weight):
            calls3.append(tuple(weight.shape))
            return F.conv2d(x, weight, None, 1, 1)

    class Count2:
        @staticmethod
        def apply(x, weight, stride, padding):
            calls2.append(tuple(weight.shape) + (stride, padding))
            return F.conv2d(x, weight, None, stride, padding)
    monkeypatch.setattr(network, 'Conv3x3Function', Count3)
    monkeypatch.setattr(network, 'Conv2dFunction', Count2)
    torch.manual_seed(1)
    plain = ResNet18().eval()
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        want = _trunk_maps(plain, x)
        assert calls3 == [] and calls2 == []
        expect2 = [(64, 3, 7, 7, 2, 3)] + [t for c in (64, 128, 256) for t in ((2 * c, c, 3, 3, 2, 1), (2 * c, c, 1, 1, 2, 0))]
        for kwargs, n3 in ((dict(hip_conv_strided=True), 0), (dict(hip_conv=True, hip_conv_strided=True), 13), (dict(hip_conv=True), 13)):
            del calls3[:], calls2[:]
            m = ResNet18(**kwargs).eval()
            m.load_state_dict(plain.state_dict(), strict=True)
            got = _trunk_maps(m, x)
            assert len(calls3) == n3 and calls2 == (expect2 if kwargs.get('hip_conv_strided') else []), kwargs
            assert all(torch.equal(a, b) for a, b in zip(got, want))
            del calls3[:], calls2[:]
            assert torch.equal(m(x), plain(x))                     # forward() goes through _stem: the stem is routed there too
            assert len(calls3) == n3 and len(calls2) == (7 if kwargs.get('hip_conv_strided') else 0)


def test_every_refusal_of_the_function_is_raised_before_any_launch(monkeypatch):
    import vpn_amd
    from vpn_amd import ops, _lib

    def no_library(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'call', no_library)
    monkeypatch.setattr(_lib, 'lib', no_library)
    x, w = torch.randn(2, 3, 8, 8), torch.randn(5, 3, 3, 3)
    with pytest.raises(ValueError, match='B, C_in, H, W'):
        vpn_amd.conv2d(x[0], w, 2, 1)
    with pytest.raises(ValueError, match='C_out, C_in, R, R'):
        vpn_amd.conv2d(x, torch.randn(5, 3, 3, 1), 2, 1)
    with pytest.raises(ValueError, match='C_out, C_in, R, R'):
        vpn_amd.conv2d(x, w[0], 2, 1)
    for k in (2, 5):
        with pytest.raises(NotImplementedError, match='kernel size'):
            vpn_amd.conv2d(x, torch.randn(5, 3, k, k), 2, 1)
    with pytest.raises(ValueError, match='input channels'):
        vpn_amd.conv2d(x, torch.randn(5, 4, 3, 3), 2, 1)
    for stride in (0, -1, 1.5, (2, 2)):
        with pytest.raises(ValueError, match='stride'):
            vpn_amd.conv2d(x, w, stride, 1)
    for padding in (-1, 0.5, 'same', (1, 1)):
        with pytest.raises(ValueError, match='padding'):
            vpn_amd.conv2d(x, w, 2, padding)
    with pytest.raises(NotImplementedError, match='fp32'):
        ops.Conv2dFunction.apply(x.double(), w.double(), 2, 1)
    with pytest.raises(NotImplementedError, match='fp32'):
        ops.Conv2dFunction.apply(x, w.half(), 2, 1)
    with pytest.raises(ValueError, match='empty'):
        vpn_amd.conv2d(x[:0], w, 2, 1)
    with pytest.raises(ValueError, match='smaller than'):
        vpn_amd.conv2d(x[:, :, :4, :4], torch.randn(5, 3, 7, 7), 2, 1)
    with pytest.raises(ValueError, match='GPU only'):
        vpn_amd.conv2d(x, w, 2, 1)
    with pytest.raises(ValueError, match='GPU only'):
        vpn_amd.conv2d(x, w)                                       # the defaults: stride 1, padding 0


def test_trunkstride_compiles_as_build_py_compiles_it_within_the_resource_limits():
    rows = kernel_resources('trunkstride.hip')
    kernels = {k: v for k, v in rows.items() if 'cs_gemm_kernel' in k or 'cg_merge_kernel' in k}
    # the GEMM kernel for three kernel sizes x three products, the merge by 4 and by 1
    assert len(kernels) == len(rows) == 11, list(rows)
    assert sum('cs_gemm_kernel' in k for k in kernels) == 9 and sum('cg_merge_kernel' in k for k in kernels) == 2
    for k, v in kernels.items():
        assert v['ScratchSize'] == 0, (k, v)
        assert v['LDS'] <= 64 * 1024, (k, v)
        assert v['AGPRs'] + v['VGPRs'] <= 128, (k, v)          # four waves per SIMD fit
