"""GPU tests of the plain GCN input op and its neighbours (ops.GcnInputFunction, GcnAggregateFunction, gcn_bounds; csrc/gcn.hip,
DESIGN.md 4.7) against the float64 restatement, at the edges the model tests do not reach: the cases of tests/gcn_input_ref.py.

dverts is compared twice: norm-wise over all decidable rows (the 1e-4 bar of test_gcn.py), and split into the rows that hold
an extent (E: they carry a sum over all N vertices) and the others (O), each element-wise against its own largest component,
with the bar of test_gpu_parity._raster_case: 1e-3, or 4 x the error of the same restatement evaluated in fp32 on the CPU."""
import pytest
import torch

import gcn_input_ref as G
import gcn_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ALL = ('verts', 'glob', 'maps')


@pytest.fixture(scope='module')
def vpn():
    import vpn_amd
    return vpn_amd


def _run(vpn, c, wanted=ALL):
    """(x, dverts, dglob, [dmap]) of one forward + backward on the GPU; an input outside `wanted` requires no gradient."""
    v = c['verts'].to(DEV).requires_grad_('verts' in wanted)
    g = c['glob'].to(DEV).requires_grad_('glob' in wanted) if c['glob'] is not None else None
    mp = [m.to(DEV).requires_grad_('maps' in wanted) for m in c['maps']]
    x = vpn.ops.GcnInputFunction.apply(v, c['bounds'].to(DEV), g, c['venc'], *mp)
    (x * c['R'].to(DEV)).sum().backward()
    return x.detach(), v.grad, g.grad if g is not None else None, [m.grad for m in mp]


_FIRST = {}


def _first(vpn, name):
    """The first full run of a case in this process, kept for the tests that compare a later run with it."""
    if name not in _FIRST:
        _FIRST[name] = _run(vpn, G.case(name))
    return _FIRST[name]


def _bit_equal(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and len(a[3]) == len(b[3])
    assert (a[2] is None and b[2] is None) or torch.equal(a[2], b[2])
    for p, q in zip(a[3], b[3]):
        assert torch.equal(p, q)


def _check_dverts(name, dv, c=None):
    """The norm-wise bar over the decidable rows and the split measure against the fp32 restatement's own."""
    c = c or G.case(name)
    dv64, dv32 = G.reference64(name)[1], G.reference32(name)[1]
    keep = ~c['masked']
    e = rel_err(dv[keep], dv64[keep])
    (o, ex), (o32, ex32) = G.split_errors(dv, dv64, c), G.split_errors(dv32, dv64, c)
    print(name, 'dverts %.2e  split O %.2e (fp32 restatement %.2e)  E %.2e (fp32 restatement %.2e)' % (e, o, o32, ex, ex32))
    assert e <= 1e-4
    assert o <= G.split_bar(o32), (o, o32)
    assert ex <= G.split_bar(ex32), (ex, ex32)


@pytest.mark.parametrize('name', G.PARITY_CASES)
def test_op_against_float64(vpn, name):
    c = G.case(name)
    x, dv, dg, dm = [t.cpu() if isinstance(t, torch.Tensor) else t for t in _first(vpn, name)]
    x64, dv64, dg64, dm64 = G.reference64(name)
    assert x.shape == x64.shape and dv.shape == dv64.shape and len(dm) == len(dm64)
    errs = dict(x=rel_err(x, x64))
    if dg64 is not None:
        assert dg.shape == dg64.shape
        errs['dglob'] = rel_err(dg.cpu(), dg64)
    else:
        assert dg is None
    for i, (a, b) in enumerate(zip(dm, dm64)):
        assert a.shape == b.shape
        errs['dmap%d' % i] = rel_err(a.cpu(), b)
    print(name, errs)
    assert errs.pop('x') <= 1e-5
    for k, e in errs.items():
        assert e <= 1e-4, (k, e)
    _check_dverts(name, dv, c)


def test_ties_send_the_extent_term_to_the_lowest_index(vpn):
    """gcn_extent_kernel keeps the lowest index of a tie and gcn_extent_bwd_kernel sends the whole sum there, as torch.max /
    torch.min do in the reference: every other vertex of a tie group keeps its direct term alone.  The bar is 1e-4 of the
    largest direct term (the extent term is ~N times an ordinary one, so a misplaced share of it cannot hide)."""
    c = G.case('ties')
    dv = _first(vpn, 'ties')[1].cpu().double()
    dv64, direct = G.reference64('ties')[1], G.reference_without_extent_term(c)
    scale = float(direct.abs().max())
    for i, cols in G.later_tie_rows().items():
        for ref in (dv64, direct):
            assert float((dv[:, i, cols] - ref[:, i, cols]).abs().max()) <= 1e-4 * scale, (i, cols)
    for key, g in G.TIE_GROUPS.items():
        col = 2 if key[0] == 'z' else 1
        assert bool(((dv[:, min(g), col] - direct[:, min(g), col]).abs() > 10 * 1e-4 * scale).all()), key


@pytest.mark.parametrize('name', ['small_square', 'nonsquare'])
def test_gradient_subsets(vpn, name):
    c, full = G.case(name), _first(vpn, name)
    for wanted in (('verts',), ('maps',), ('glob',), ('maps', 'glob')):
        part = _run(vpn, c, wanted)
        assert torch.equal(part[0], full[0])
        assert torch.equal(part[1], full[1]) if 'verts' in wanted else part[1] is None, wanted
        assert torch.equal(part[2], full[2]) if 'glob' in wanted else part[2] is None, wanted
        for p, q in zip(part[3], full[3]):
            assert torch.equal(p, q) if 'maps' in wanted else p is None, wanted


def test_the_sort_limit(vpn):
    """N = 8192 sorts (test_op_against_float64[n8192]).  One vertex more: the forward and the vertices' gradient run as at any
    N, a map that requires a gradient is a ValueError from forward, before any launch, and the process goes on as before."""
    before = _first(vpn, 'small_square')
    c = G.case('n8193')
    assert c['verts'].shape[1] == vpn.ops.GCN_SORT_MAX_N + 1
    x64 = G.reference64('n8193')[0]
    with torch.no_grad():
        x = vpn.ops.GcnInputFunction.apply(c['verts'].to(DEV), c['bounds'].to(DEV), None, c['venc'], *[m.to(DEV) for m in c['maps']])
    assert x.shape == x64.shape and rel_err(x.cpu(), x64) <= 1e-5
    xv, dv, _, dm = _run(vpn, c, ('verts',))
    assert torch.equal(xv, x) and all(m is None for m in dm)
    _check_dverts('n8193', dv.cpu(), c)
    for wanted in (('maps',), ALL):
        with pytest.raises(ValueError, match=str(vpn.ops.GCN_SORT_MAX_N)):
            _run(vpn, c, wanted)
    one = [m.to(DEV).requires_grad_(l == 2) for l, m in enumerate(c['maps'])]
    with pytest.raises(ValueError, match='8193'):
        vpn.ops.GcnInputFunction.apply(c['verts'].to(DEV), c['bounds'].to(DEV), None, c['venc'], *one)
    torch.cuda.synchronize()
    _bit_equal(_run(vpn, G.case('small_square')), before)


@pytest.mark.parametrize('name', ['nonsquare', 'crowded', 'n1025'])
def test_two_runs_are_bit_equal(vpn, name):
    _bit_equal(_run(vpn, G.case(name)), _first(vpn, name))


# ---- aggregation

def _agg_meshes():
    return {'irregular': G.irregular_mesh(), 'single_vertex': (torch.zeros(0, 3, dtype=torch.long), 1),
            'random_131': G.random_mesh(131, 300, 5)}


@pytest.mark.parametrize('C', [1, 4, 6, 260])
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('with_bias', [False, True])
def test_aggregation_edge_cases_against_float64(vpn, C, relu, with_bias):
    for mesh, (faces, N) in _agg_meshes().items():
        B = 3
        gen = torch.Generator().manual_seed(C * 4 + relu * 2 + with_bias)
        graph = vpn.ops.gcn_graph(faces, N, DEV)
        h, g = torch.randn(B, N, C, generator=gen), torch.randn(B, N, C, generator=gen)
        bias = torch.randn(C, generator=gen) if with_bias else None
        hd = h.to(DEV).requires_grad_(True)
        bd = bias.to(DEV).requires_grad_(True) if with_bias else None
        y = vpn.ops.GcnAggregateFunction.apply(hd, bd, graph.row_ptr, graph.col, graph.w, relu)
        y.backward(g.to(DEV))
        h64 = h.double().requires_grad_(True)
        b64 = bias.double().requires_grad_(True) if with_bias else None
        y64 = R.aggregate(h64, R.gcn_norm(R.unique_edges(faces), N), b64)
        if relu:
            y64 = y64.relu()
        y64.backward(g.double())
        assert y.shape == y64.shape
        assert rel_err(y.detach().cpu(), y64.detach()) <= 1e-5, mesh
        assert rel_err(hd.grad.cpu(), h64.grad) <= 1e-5, mesh
        if with_bias:
            assert rel_err(bd.grad.cpu(), b64.grad) <= 1e-5, mesh
        if mesh != 'random_131':                     # a vertex in no face has its self loop alone, weight 1: y = h + bias, exactly
            lone = h[:, N - 1] + (bias if with_bias else 0)
            assert torch.equal(y.detach().cpu()[:, N - 1], lone.relu() if relu else lone), mesh
    assert (3 * 131 * C // (4 if C % 4 == 0 else 1)) % 256 != 0          # random_131 ends inside a workgroup


# ---- bounds

@pytest.mark.parametrize('shape', G.BOUNDS_SHAPES)
def test_bounds_shapes_and_sub_threshold_pixels(vpn, shape):
    imgs, only = G.bounds_images(*shape)
    out = vpn.ops.gcn_bounds(imgs.to(DEV)).cpu()
    want = R.bounds(only)
    assert out.shape == want.shape and torch.equal(out, want), (out, want)
