"""CPU checks of the GCN refinement stage (modules/gcn.py, csrc/gcn.hip): the g7 fixtures captured from the reference's
gcn.py reproduce through the float64 restatement (tests/gcn_ref.py), the normalised adjacency has PyG's gcn_norm
properties, the two GCNConv checkpoint layouts convert, and every new kernel compiles without scratch."""
import torch

import gcn_ref as R
from conftest import load_golden, rel_err
from test_kernel_budget_cpu import _resources


def test_g7_fixtures_reproduce_through_the_restatement():
    z = load_golden('g7_gcn_bounds')
    assert torch.equal(R.bounds(z['imgs']), z['bounds'])
    z = load_golden('g7_gcn_encoding')
    assert rel_err(R.positional_encoding(z['verts'].double()), z['encoding']) <= 1e-6
    z = load_golden('g7_gcn_pooling')
    maps = [z['map%d' % i].double().requires_grad_(True) for i in range(4)]
    v = z['verts'].double().requires_grad_(True)
    assert torch.equal(R.bounds(z['rgbs']), z['bounds'])
    p = R.pooling(maps, v, z['bounds'].double())
    assert rel_err(p, z['pooled']) <= 1e-5
    (p * z['W'].double()).sum().backward()
    assert rel_err(v.grad, z['grad_verts']) <= 1e-4
    for i, m in enumerate(maps):
        assert rel_err(m.grad, z['grad_map%d' % i]) <= 1e-4


def _check_adjacency(faces, n):
    from vpn_amd import ops
    edges = ops.gcn_edges(faces)
    rp, col, w = ops.gcn_normalized_adjacency(edges, n)
    rows = torch.repeat_interleave(torch.arange(n), (rp[1:] - rp[:-1]).long())
    A = torch.zeros(n, n, dtype=torch.float64)
    A[rows, col.long()] = w.double()
    assert torch.equal(A, A.t())
    assert int(rp[-1]) == 2 * edges.shape[0] + n and bool((A.diagonal() > 0).all())
    # PyG gcn_norm: w_ij = 1 / sqrt(deg_i deg_j), deg with the self loop -> row sums sum_j 1 / sqrt(deg_i deg_j)
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, edges.flatten(), torch.ones(edges.numel(), dtype=torch.float64)) + 1
    assert torch.allclose(A.diagonal(), 1 / deg, rtol=1e-6)
    ref = ((A > 0).double() / (deg[:, None] * deg[None, :]).sqrt()).sum(1)
    assert torch.allclose(A.sum(1), ref, rtol=1e-6)
    # the same matrix from the float64 restatement's entry list
    src, dst, ww = R.gcn_norm(edges, n)
    B = torch.zeros(n, n, dtype=torch.float64).index_put_((dst, src), ww, accumulate=True)
    assert torch.allclose(A, B, rtol=1e-6, atol=0)
    ei = torch.cat([edges, edges.flip(1)]).view(2, -1)
    assert torch.equal(ops.gcn_edge_index(edges), ei)
    assert torch.equal(ei[:, 0::2].t(), edges) and torch.equal(ei[:, 1::2].t(), edges.flip(1))


def test_normalized_adjacency_on_the_sphere_template_and_a_composed_mesh():
    from vpn_amd.modules.meshing import uv_sphere
    v, f = uv_sphere()
    _check_adjacency(f, v.shape[0])
    composed = torch.cat([f + v.shape[0] * k for k in range(16)])
    _check_adjacency(composed, 16 * v.shape[0])


def test_state_dict_layouts_round_trip():
    from vpn_amd.modules.gcn import GCNModel, to_pyg2_state_dict
    torch.manual_seed(0)
    a = GCNModel(img_feature_dim=8 + 4, v_num=16)
    sd = a.state_dict()
    assert 'conv1.weight' in sd and sd['conv1.weight'].shape == (39 + 12, 512) and 'conv1.lin.weight' not in sd
    pyg2 = to_pyg2_state_dict(sd)
    assert pyg2['conv1.lin.weight'].shape == (512, 39 + 12) and 'conv1.weight' not in pyg2
    assert set(k for k in pyg2 if k.startswith('fc.')) == set(k for k in sd if k.startswith('fc.'))
    for layout in (sd, pyg2):
        b = GCNModel(img_feature_dim=8 + 4, v_num=16)
        b.load_state_dict(layout)
        for k, v in b.state_dict().items():
            assert torch.equal(v, sd[k]), k


def test_gcn_kernels_use_no_scratch():
    for k in ('gcn_aggregate_kernel', 'gcn_colsum_partial_kernel', 'gcn_colsum_final_kernel', 'gcn_bounds_kernel',
              'gcn_extent_kernel', 'gcn_nhwc_kernelILb1', 'gcn_nhwc_kernelILb0', 'gcn_input_kernel', 'gcn_pool_sort_kernel',
              'gcn_pool_bwd_kernel', 'gcn_vertex_bwd_kernel', 'gcn_extent_bwd_kernel'):
        if k == 'gcn_aggregate_kernel':
            rs = [_resources('gcn.hip', k + 'ILi4'), _resources('gcn.hip', k + 'ILi1')]
        else:
            rs = [_resources('gcn.hip', k)]
        for r in rs:
            assert r['ScratchSize'] == 0, (k, r)
