"""CPU checks of the GCN's collapsed layer pairs (GCNModel(collapse_pairs=True), ops.gcn_blocks, ops.GcnAggregate2Function,
ops.GcnProjectFunction, csrc/gcnpair.hip): the pair algebra in float64, the block partition, the model's
surface, the argument contract, the C entries and the kernels' resources."""
import pytest
import torch

import gcn_collapse_ref as P
import gcn_input_ref as G
import gcn_ref as R
from conftest import rel_err
from kernel_resources import kernel_resources


@pytest.mark.parametrize('dims', [(51, 8, 8), (8, 8, 8), (8, 4, 3)], ids=lambda d: '-'.join(map(str, d)))
def test_plain_and_collapsed_pair_agree_in_float64(dims):
    """Both are sums of the same products in different orders; with at most 51 * 8 terms of O(1) an output each is within
    a few hundred 2^-53 of the exact value, far inside 1e-12 of the largest."""
    Ci, Cm, Co = dims
    faces, n = G.irregular_mesh()
    norm = R.gcn_norm(R.unique_edges(faces), n)
    gen = torch.Generator().manual_seed(Ci + Cm + Co)
    shapes = dict(x=(2, n, Ci), ta=(Ci, Cm), tb=(Cm, Co), ba=(Cm,), bb=(Co,))
    data = {k: torch.randn(*s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    W = torch.randn(2, n, Co, generator=gen, dtype=torch.float64)
    outs = []
    for form in (P.pair_plain, P.pair_collapsed):
        leaves = {k: v.clone().requires_grad_(True) for k, v in data.items()}
        y = form(leaves['x'], leaves['ta'], leaves['tb'], leaves['ba'], leaves['bb'], norm)
        (y * W).sum().backward()
        outs.append(dict(y=y.detach(), **{'d' + k: v.grad for k, v in leaves.items()}))
    assert outs[0]['y'].shape == (2, n, Co)
    for k in outs[0]:
        assert rel_err(outs[1][k], outs[0][k]) <= 1e-12, (k, rel_err(outs[1][k], outs[0][k]))


def test_block_partition():
    from vpn_amd import ops
    limit = ops.GCN_HOP2_MAX_ROWS
    assert limit in (128, 256)
    tables = {}
    for name, (faces, n) in P.meshes(limit).items():
        t = ops.gcn_blocks(faces, n, 'cpu')
        edges = ops.gcn_edges(faces)
        assert ops.gcn_closed_ranges(edges, n) == P.closed_ranges(edges, n), name
        if t is not None:
            assert t.dtype == torch.int32 and t.dim() == 1
            P.check_table(t.tolist(), edges, n, limit)
            assert ops.gcn_blocks(faces.clone(), n, 'cpu') is t, name            # cached by content
        tables[name] = None if t is None else t.tolist()
    assert tables['two_irregular_and_lone'] == [0, 19]
    assert ops.gcn_closed_ranges(ops.gcn_edges(P.meshes(limit)['two_irregular_and_lone'][0]), 19) == [0, 8, 9, 17, 18]
    assert tables['single_vertex'] == [0, 1]
    per = limit // 3 * 3                                                         # whole triangles a block
    assert tables['triangles_70'] == list(range(0, 210, per)) + [210]
    assert tables['interleaved'] == [0, 12]
    assert tables['clique_70'] == [0, 70]
    assert tables['strip_max'] == [0, limit]
    assert tables['strip_max_plus_1'] is None
    assert ops.gcn_block_starts(ops.gcn_edges(P.meshes(limit)['two_irregular_and_lone'][0]), 19, limit=9) == [0, 9, 18, 19]
    with pytest.raises(ValueError, match='index vertex'):
        ops.gcn_blocks(torch.tensor([[0, 1, 5]]), 4, 'cpu')


def test_constructor_takes_the_switch_and_keeps_the_state_dict():
    from vpn_amd.modules.gcn import GCNModel, to_pyg2_state_dict
    torch.manual_seed(0)
    plain = GCNModel(img_feature_dim=8 + 4, v_num=16)
    coll = GCNModel(img_feature_dim=8 + 4, v_num=16, collapse_pairs=True)
    both = GCNModel(img_feature_dim=8 + 4, v_num=16, factored_input=True, collapse_pairs=True)
    assert plain.collapse_pairs is False and coll.collapse_pairs is True and both.factored_input and both.collapse_pairs
    sd = plain.state_dict()
    for m in (coll, both):
        md = m.state_dict()
        assert list(sd) == list(md) and all(sd[k].shape == md[k].shape for k in sd)
        assert [n for n, _ in m.named_parameters()] == [n for n, _ in plain.named_parameters()]
    for layout in (sd, to_pyg2_state_dict(sd)):
        m = GCNModel(img_feature_dim=8 + 4, v_num=16, collapse_pairs=True)
        m.load_state_dict(layout)
        for k, v in m.state_dict().items():
            assert torch.equal(v, sd[k]), k


def test_contract_is_checked_before_any_launch():
    """On CPU tensors: a ValueError from the shapes alone, before the device is asked for anything."""
    import vpn_amd
    from vpn_amd import ops
    faces, n = G.irregular_mesh()
    graph, blocks = ops.gcn_graph(faces, n, 'cpu'), ops.gcn_blocks(faces, n, 'cpu')
    h = torch.zeros(2, n, 4)
    with pytest.raises(ValueError, match=r'h must be \[B,N,C\]'):
        vpn_amd.gcn_aggregate2(h[0], None, None, graph, blocks)
    with pytest.raises(ValueError, match='graph has 9 vertices'):
        vpn_amd.gcn_aggregate2(torch.zeros(2, n + 1, 4), None, None, graph, blocks)
    with pytest.raises(ValueError, match='u must be'):
        vpn_amd.gcn_aggregate2(h, torch.zeros(3), None, graph, blocks)
    with pytest.raises(ValueError, match='bias must be'):
        vpn_amd.gcn_aggregate2(h, None, torch.zeros(1, 4), graph, blocks)
    with pytest.raises(ValueError, match='blocks must be int32'):
        vpn_amd.gcn_aggregate2(h, None, None, graph, blocks.long())
    for b in (blocks, None):                                              # a valid call has no CPU path, table or not
        with pytest.raises(RuntimeError, match='GPU only'):
            vpn_amd.gcn_aggregate2(h, torch.zeros(4), torch.zeros(4), graph, b, relu=True)
    x = torch.zeros(2, 5, 8)
    with pytest.raises(ValueError, match='at most 4'):
        vpn_amd.gcn_project(x, torch.zeros(8, 5))
    with pytest.raises(ValueError, match='at most 1024'):
        vpn_amd.gcn_project(torch.zeros(2, 1025), torch.zeros(1025, 3))
    with pytest.raises(ValueError, match=r'x must be \[\.\.\., Ci\]'):
        vpn_amd.gcn_project(x, torch.zeros(7, 3))
    with pytest.raises(ValueError, match=r'theta must be \[Ci,Co\]'):
        vpn_amd.gcn_project(x, torch.zeros(8))
    with pytest.raises(RuntimeError, match='GPU only'):
        vpn_amd.gcn_project(x, torch.zeros(8, 3))
    assert vpn_amd.GcnAggregate2Function is ops.GcnAggregate2Function and vpn_amd.GcnProjectFunction is ops.GcnProjectFunction
    assert ops.GCN_PROJECT_MAX_CO == 4 and ops.GCN_PROJECT_MAX_CI == 1024


def test_entries_were_added_without_an_abi_change():
    import vpn_amd._lib as lib
    L = lib.lib()
    assert L.vpn_abi_version() == lib.ABI_VERSION == 9
    for name in ('vpn_gcn_aggregate2_workspace', 'vpn_gcn_aggregate2', 'vpn_gcn_project_bwd_workspace', 'vpn_gcn_project_fwd',
                 'vpn_gcn_project_bwd'):
        assert name in lib.SIGNATURES and hasattr(L, name), name
    # sizes from the shapes: a sum per (sample, block, channel); a partial sum of dTheta per 64 rows
    assert L.vpn_gcn_aggregate2_workspace(2, 3, 5) == 2 * 3 * 5 * 4 and L.vpn_gcn_aggregate2_workspace(2, 0, 5) == 0
    assert L.vpn_gcn_project_bwd_workspace(130, 8, 2) == 3 * 8 * 2 * 4
    assert L.vpn_gcn_project_bwd_workspace(130, 8, 5) == 0 and L.vpn_gcn_project_bwd_workspace(130, 1025, 2) == 0
    assert L.vpn_gcn_aggregate2(None, None, None, None, None, None, 1, None, None, 1, 1, 1, 0, None, None, None) == -1
    assert L.vpn_gcn_project_fwd(None, None, 1, 4, 1, None, None) == -1
    assert L.vpn_gcn_project_bwd(None, None, None, 1, 4, 1, None, None, None, None) == -1


def test_pair_kernels_use_no_scratch_and_hop2_fits_twice_a_cu():
    from vpn_amd import ops
    rows = kernel_resources('gcnpair.hip')
    for k, count in (('gcn_hop2_kernel', 2), ('gcn_project_fwd_kernel', 2), ('gcn_project_bwd_kernel', 2),
                     ('gcn_project_dtheta_kernel', 1)):
        hits = [v for name, v in rows.items() if k in name]
        assert len(hits) == count, (k, list(rows))                        # the dwordx4 and the element instantiation
        for h in hits:
            assert h['ScratchSize'] == 0, (k, h)
    assert len(rows) == 7, list(rows)
    for v in (v for name, v in rows.items() if 'gcn_hop2_kernel' in name):
        assert v['LDS'] <= 64 * 1024, v
        assert v['LDS'] >= 2 * ops.GCN_HOP2_MAX_ROWS * 4 * 4                # both hops' rows are there, at least a dwordx4 wide
