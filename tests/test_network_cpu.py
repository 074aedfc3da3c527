"""The network stage without a GPU: the C ABI's argument checks, the ResNet-18 trunk's names and sizes, the heads'
state_dict against the names recorded from the reference (tests/golden/g11_network.npz, tools/make_golden_network.py),
fix_volume_weight, the absence of a CPU path, and the CPU restatement against the reference's recorded range case."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import network_ref as R
from conftest import GOLDEN


def _g11():
    with np.load(os.path.join(GOLDEN, 'g11_network.npz'), allow_pickle=False) as z:
        return {k: np.array(z[k]) for k in z.files}


class TinyTrunk(nn.Module):
    """The attribute surface of the ResNet that extract_feature touches, 40 channels out."""

    def __init__(self, feat=40):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 8, 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(8)
        self.relu = nn.ReLU()
        self.maxpool = nn.MaxPool2d(2)
        self.layer1 = nn.Conv2d(8, 8, 1)
        self.layer2 = nn.Conv2d(8, 16, 1)
        self.layer3 = nn.Conv2d(16, 16, 1)
        self.layer4 = nn.Conv2d(16, feat, 1)


def test_fc_stack_argument_checks():
    import vpn_amd._lib as lib
    L = lib.lib()
    tail = (0, 0.5, 0, None, 0, 0, 1, 0.0, 1.0, 1.0, 1.0, 1.0)
    st = lib.FcStack()
    assert L.vpn_fc_stack_fwd(st, *tail, None, None) == -1                      # G = L = B = 0
    st.G, st.L, st.B = 1, 1, 1
    assert L.vpn_fc_stack_fwd(st, *tail, None, None) == -1                      # null pointers
    assert L.vpn_fc_stack_bwd(st, lib.FcGrad(), *tail, None, 0, None) == -1
    st.in0[0], st.out[0] = 4, 4
    for f in ('x', 'w', 'bias', 'act'):
        getattr(st, f)[0] = 64                                                  # never dereferenced: checks only
    st.B = 0
    assert L.vpn_fc_stack_fwd(st, *tail, None, None) == -1
    st.B, st.L = 1, 0
    assert L.vpn_fc_stack_fwd(st, *tail, None, None) == -1
    st.L, st.G = 9, 1
    assert L.vpn_fc_stack_fwd(st, *tail, None, None) == -2                      # more layers than VPN_FC_MAX_LAYERS
    st.L, st.G = 5, 5
    assert L.vpn_fc_stack_fwd(st, *tail, None, None) == -2                      # G L over the struct's capacity
    assert L.vpn_fc_stack_bwd(st, lib.FcGrad(), *tail, None, 0, None) == -2
    st.L, st.G = 1, 1
    assert L.vpn_fc_stack_fwd(st, 0, 0.5, 0, None, lib.FC_TANH, 0, 1, 0.0, 1.0, 1.0, 1.0, 1.0, None, None) == -1      # no `final`
    assert L.vpn_fc_stack_fwd(st, lib.FC_DROPOUT_MASK, 1.5, 0, None, 0, 0, 1, 0.0, 1.0, 1.0, 1.0, 1.0, None, None) == -1
    assert L.vpn_fc_stack_bwd(st, lib.FcGrad(), *tail, None, 0, None) == -1    # no workspace
    assert L.vpn_fc_stack_workspace(3, 8, 1024) == 3 * 8 * 1024 * (32 + 1) * 4
    assert L.vpn_fc_stack_workspace(0, 8, 1024) == 0
    assert ctypes_sizes_match(lib)


def ctypes_sizes_match(lib):
    import ctypes
    # VpnFcStack: 4 + 24 + 24 int32, then 5 x 24 pointers; VpnFcGrad: 4 x 24 pointers
    return ctypes.sizeof(lib.FcStack) == 4 * 52 + 8 * 120 and ctypes.sizeof(lib.FcGrad) == 8 * 96


def test_header_and_binding_agree():
    from test_cabi_cpu import _header_symbols
    import vpn_amd._lib as lib
    syms = _header_symbols()
    for name in ('vpn_fc_stack_fwd', 'vpn_fc_stack_bwd', 'vpn_fc_stack_workspace'):
        assert name in syms and name in lib.SIGNATURES and hasattr(lib.lib(), name)
    assert sorted(lib.SIGNATURES) == syms


def test_resnet18_names_and_size():
    from vpn_amd.modules.network import ResNet18
    net = ResNet18()
    sd = net.state_dict()
    assert len(sd) == 122
    for k in ('layer2.0.downsample.1.running_var', 'fc.bias', 'bn1.num_batches_tracked', 'conv1.weight',
              'layer4.1.bn2.weight', 'layer1.0.conv1.weight'):
        assert k in sd, k
    assert 'layer1.0.downsample.0.weight' not in sd
    assert sum(p.numel() for p in net.parameters()) == 11689512
    assert tuple(sd['fc.weight'].shape) == (1000, 512) and tuple(sd['conv1.weight'].shape) == (64, 3, 7, 7)


def test_extract_feature_cpu():
    from vpn_amd.modules.network import VPNetOneRes
    net = VPNetOneRes().eval()
    with torch.no_grad():
        feats, maps = net.extract_feature(torch.rand(1, 3, 64, 64))
    assert tuple(feats.shape) == (1, 512)
    assert [tuple(m.shape) for m in maps] == [(1, 64, 16, 16), (1, 128, 8, 8), (1, 256, 4, 4), (1, 512, 2, 2)]


@pytest.mark.parametrize('drop', [0, 1])
def test_head_names_equal_reference(drop):
    from vpn_amd.modules.network import VPNetOneRes, VPNetTwoRes, SDNet
    g = _g11()
    K = int(g['vp_num'])
    one = VPNetOneRes(vp_num=K, is_dropout=bool(drop), trunk=TinyTrunk(512))
    two = VPNetTwoRes(vp_num=K, is_dropout=bool(drop), trunk=(TinyTrunk(512), TinyTrunk(512)))
    sd = SDNet(trunk=TinyTrunk(512))
    for tag, net in (('one', one), ('two', two), ('sd', sd)):
        state = net.state_dict()
        mine = [k for k in state if '_fc.' in k or '.deform.' in k]
        assert mine == list(g['%s_drop%d_names' % (tag, drop)]), tag
        shapes = [list(state[k].shape) + [0] * (2 - state[k].dim()) for k in mine]
        assert shapes == g['%s_drop%d_shapes' % (tag, drop)].tolist(), tag
        twin = type(net)(**({'vp_num': K, 'is_dropout': bool(drop)} if tag != 'sd' else {}),
                         trunk=(TinyTrunk(512), TinyTrunk(512)) if tag == 'two' else TinyTrunk(512))
        twin.load_state_dict(state, strict=True)
        assert all(torch.equal(a, b) for a, b in zip(twin.state_dict().values(), state.values()))


def test_full_model_state_dict_names():
    from vpn_amd.modules.network import VPNetOneRes, SDNet
    sd = VPNetOneRes().state_dict()
    assert len(sd) == 122 + 30 and 'resnet.layer3.0.downsample.0.weight' in sd and 'translate_fc.4.bias' in sd
    sd = SDNet().state_dict()
    assert len(sd) == 122 + 10 and '_model.fc.weight' in sd and '_model.deform.4.weight' in sd
    assert tuple(sd['_model.deform.4.weight'].shape) == (386 * 3, 1024)


def test_fix_volume_weight():
    from vpn_amd.modules.network import VPNetOneRes, VPNetTwoRes
    one = VPNetOneRes(hidden=72, feat=40, trunk=TinyTrunk())
    one.fix_volume_weight()
    frozen = {n for n, p in one.named_parameters() if not p.requires_grad}
    assert frozen == {n for n, _ in one.named_parameters() if n.startswith('volume_fc.')} and len(frozen) == 10
    two = VPNetTwoRes(hidden=72, feat=40, trunk=(TinyTrunk(), TinyTrunk()))
    two.fix_volume_weight()
    frozen = {n for n, p in two.named_parameters() if not p.requires_grad}
    assert frozen == {n for n, _ in two.named_parameters() if n.startswith(('volume_fc.', 'volume_resnet.'))}
    assert any(n.startswith('volume_resnet.') for n in frozen)


def test_range_rules_are_staticmethods_as_in_the_reference():
    import inspect
    from vpn_amd.modules.network import VPNetOneRes, VPNetTwoRes
    for cls in (VPNetOneRes, VPNetTwoRes):
        assert isinstance(inspect.getattr_static(cls, 'restrict_range'), staticmethod)
        assert isinstance(inspect.getattr_static(cls, 'restrict_volumes'), staticmethod)
        v = cls.restrict_volumes([torch.ones(2, 3), torch.ones(2, 3)])
        assert torch.allclose(v[1], torch.tensor([1 / 8, 1 / 10, 1 / 10]).expand(2, 3))
        with pytest.raises(RuntimeError, match='GPU only'):
            cls.restrict_range(torch.rand(2, 6), torch.rand(2, 8), torch.rand(2, 6))


def test_no_cpu_path():
    from vpn_amd.modules.network import VPNetOneRes, VPNetTwoRes, SDNet, FcHeads
    imgs = torch.rand(2, 3, 16, 16)
    nets = [VPNetOneRes(vp_num=2, hidden=72, feat=40, trunk=TinyTrunk()),
            VPNetTwoRes(vp_num=2, hidden=72, feat=40, trunk=(TinyTrunk(), TinyTrunk())),
            SDNet(vertex_num=5, hidden=72, feat=40, trunk=TinyTrunk())]
    for net in nets:
        with pytest.raises(RuntimeError, match='GPU only'):
            net(imgs)
    heads = FcHeads({'a': 7}, feat=40, hidden=72)
    with pytest.raises(RuntimeError, match='GPU only'):
        heads.run_heads([torch.rand(2, 40)])


@pytest.mark.parametrize('sig', [0, 1])
def test_network_ref_reproduces_reference_case(sig):
    g = _g11()
    v, q, t = (torch.from_numpy(g['raw_' + n]) for n in ('volumes', 'rotates', 'translates'))
    p = R.vp_pack(v, q, t, bool(sig), float(g['clamp'][0]), float(g['clamp'][1]), g['volume_restrict'].tolist())
    want = torch.cat([torch.from_numpy(g['sig%d_%s' % (sig, n)]) for n in ('volumes', 'rotates', 'translates')], dim=2)
    assert p.dtype == torch.float32 and tuple(p.shape) == (2, 3, 10)
    assert float((p - want).abs().max()) <= 2e-7            # one fp32 rounding of values below 2
    assert int(g['vp_num']) == 16
