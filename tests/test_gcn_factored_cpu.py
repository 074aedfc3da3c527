"""CPU checks of conv1 in factored form (GCNModel(factored_input=True), ops.GcnFactoredInputFunction, the gcn_factored_
kernels of csrc/gcn.hip): the algebra in float64 through tests/gcn_ref.py, the model's surface, the argument
contract and the kernels' resources."""
import pytest
import torch

import gcn_factored_ref as F
from conftest import rel_err
from kernel_resources import kernel_resources


def test_constructor_takes_the_switch_and_keeps_the_state_dict():
    from vpn_amd.modules.gcn import GCNModel, to_pyg2_state_dict
    torch.manual_seed(0)
    plain = GCNModel(img_feature_dim=8 + 4, v_num=16)
    fact = GCNModel(img_feature_dim=8 + 4, v_num=16, factored_input=True)
    assert plain.factored_input is False and fact.factored_input is True
    sd, fd = plain.state_dict(), fact.state_dict()
    assert list(sd) == list(fd) and all(sd[k].shape == fd[k].shape for k in sd)
    assert fd['conv1.weight'].shape == (39 + 12, 512) and 'conv1.lin.weight' not in fd
    for layout in (sd, to_pyg2_state_dict(sd)):
        m = GCNModel(img_feature_dim=8 + 4, v_num=16, factored_input=True)
        m.load_state_dict(layout)
        for k, v in m.state_dict().items():
            assert torch.equal(v, sd[k]), k
    assert [n for n, _ in fact.named_parameters()] == [n for n, _ in plain.named_parameters()]


@pytest.mark.parametrize('name', sorted(F.OP_CASES))
def test_plain_and_factored_agree_in_float64(name):
    """Both are sums of at most 1511 products per output taken in different orders: each is within 1511 * 2^-53 of the
    exact value relative to the sum of the terms' magnitudes, far inside 1e-12 of the largest output."""
    c = F.op_case(name)
    args = (c['verts'].double(), c['bounds'].double(), c['glob'].double() if c['glob'] is not None else None,
            c['weight'].double(), c['venc'], [m.double() for m in c['maps']])
    a, b = F.plain(*args), F.factored(*args)
    assert a.shape == (2, c['verts'].shape[1], c['weight'].shape[1])
    assert rel_err(b, a) <= 1e-12, rel_err(b, a)
    if name == 'corners_outside':
        out, inside = F.outside_fractions(c['verts'], c['bounds'], 32)
        assert out >= 0.2 and inside >= 0.2, (out, inside)


def test_contract_is_checked_before_any_launch():
    """On CPU tensors: a ValueError from the shapes alone, before the device is asked for anything."""
    import vpn_amd
    v, b, g, m = torch.zeros(1, 5, 3), torch.zeros(1, 4), torch.zeros(1, 2), [torch.zeros(1, 4, 3, 3)]
    with pytest.raises(ValueError, match='multiple of 4'):
        vpn_amd.gcn_factored_input(v, b, g, torch.zeros(39 + 4 + 2, 6), 39, m)
    with pytest.raises(ValueError, match='rows'):
        vpn_amd.gcn_factored_input(v, b, g, torch.zeros(39 + 4 + 2 + 1, 8), 39, m)
    with pytest.raises(ValueError, match='venc'):
        vpn_amd.gcn_factored_input(v, b, g, torch.zeros(5 + 4 + 2, 8), 5, m)
    with pytest.raises(ValueError, match='at most 4'):
        vpn_amd.gcn_factored_input(v, b, g, torch.zeros(39 + 20 + 2, 8), 39, m * 5)
    with pytest.raises(ValueError, match='at most 8192'):
        vpn_amd.gcn_factored_input(torch.zeros(1, 8193, 3), b, g, torch.zeros(39 + 4 + 2, 8), 39, m)
    with pytest.raises(RuntimeError, match='GPU only'):                   # a valid call has no CPU path
        vpn_amd.gcn_factored_input(v, b, g, torch.zeros(39 + 4 + 2, 8), 39, m)
    from vpn_amd import ops
    assert vpn_amd.GcnFactoredInputFunction is ops.GcnFactoredInputFunction and ops.GCN_SORT_MAX_N == 8192


def test_entries_were_added_without_an_abi_change():
    import vpn_amd._lib as lib
    L = lib.lib()
    assert L.vpn_abi_version() == lib.ABI_VERSION == 9
    for name in ('vpn_gcn_factored_proj_workspace', 'vpn_gcn_factored_fwd', 'vpn_gcn_factored_bwd_workspace',
                 'vpn_gcn_factored_bwd'):
        assert name in lib.SIGNATURES and hasattr(L, name), name
    # sizes from the shapes: projected maps [B, sum H W, Cout]; sorted records, cell starts, q, 128-row partial sums
    assert L.vpn_gcn_factored_proj_workspace(2, 8, 2, 3, 4, 2, 2, 0, 0, 0, 0) == 2 * 16 * 8 * 4
    assert L.vpn_gcn_factored_proj_workspace(2, 6, 1, 3, 4, 0, 0, 0, 0, 0, 0) == 0
    assert L.vpn_gcn_factored_bwd_workspace(2, 100, 8, 39, 1, 3, 4, 0, 0, 0, 0, 0, 0) == \
        (2 * 100 * 4 + 2 * (4 * 5 + 2) + 2 * 100 * 2 + 2 * 39 * 8) * 4
    assert L.vpn_gcn_factored_fwd(None, None, None, None, None, 1, 1, 4, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, None, None, None,
                                  None) == -1
    assert L.vpn_gcn_factored_bwd(None, None, None, None, None, 1, 1, 4, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, None, None, None,
                                  None, None, None, None) == -1


def test_factored_kernels_use_no_scratch():
    rows = kernel_resources('gcn.hip')
    for k in ('gcn_factored_fwd_kernel', 'gcn_factored_enc_partial_kernel', 'gcn_factored_enc_final_kernel',
              'gcn_factored_vertex_bwd_kernel'):
        hits = [v for name, v in rows.items() if k in name]
        assert len(hits) == 1, (k, list(rows))
        assert hits[0]['ScratchSize'] == 0, (k, hits[0])
    fwd = [v for name, v in rows.items() if 'gcn_factored_fwd_kernel' in name][0]
    assert fwd['LDS'] <= 32 * 1024, fwd                                   # Theta_e's chunk and the tile's encodings: five workgroups a CU
