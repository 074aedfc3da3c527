"""GPU tests of the GCN's collapsed layer pairs (ops.gcn_aggregate2, ops.gcn_project, GCNModel(collapse_pairs=True),
csrc/gcnpair.hip): the two-hop aggregation bit for bit against two one-hop launches, the skinny projection
element-wise against float64, the model against the float64 restatement of tests/gcn_ref.py."""
import pytest
import torch

import gcn_collapse_ref as P
import gcn_input_ref as G
import gcn_ref as R
from conftest import rel_err
from test_gcn import _run_gpu, _run_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def vpn():
    import vpn_amd
    return vpn_amd


def _meshes(vpn):
    m = P.meshes(vpn.ops.GCN_HOP2_MAX_ROWS)
    m['random_131'] = G.random_mesh(131, 300, 5)
    return m


def _case(C, n, seed):
    gen = torch.Generator().manual_seed(seed)
    return dict(h=torch.randn(2, n, C, generator=gen), u=torch.randn(C, generator=gen), b=torch.randn(C, generator=gen),
                g=torch.randn(2, n, C, generator=gen))


def _leaves(c, with_u, with_b, grads=('h', 'u', 'b')):
    h = c['h'].to(DEV).requires_grad_('h' in grads)
    u = c['u'].to(DEV).requires_grad_('u' in grads) if with_u else None
    b = c['b'].to(DEV).requires_grad_('b' in grads) if with_b else None
    return h, u, b


def _grads(y, c, h, u, b):
    y.backward(c['g'].to(DEV))
    return [y.detach(), h.grad, u.grad if u is not None else None, b.grad if b is not None else None]


def _two_hop(vpn, c, graph, blocks, with_u, with_b, relu, grads=('h', 'u', 'b')):
    h, u, b = _leaves(c, with_u, with_b, grads)
    return _grads(vpn.gcn_aggregate2(h, u, b, graph, blocks, relu=relu), c, h, u, b)


def _composition(vpn, c, graph, with_u, with_b, relu):
    h, u, b = _leaves(c, with_u, with_b)
    f = vpn.ops.GcnAggregateFunction.apply
    t = f(h, u, graph.row_ptr, graph.col, graph.w, False)
    return _grads(f(t, b, graph.row_ptr, graph.col, graph.w, relu), c, h, u, b)


@pytest.mark.parametrize('C', [1, 3, 4, 6, 260])
@pytest.mark.parametrize('relu', [False, True])
def test_aggregate2_equals_two_one_hop_launches(vpn, C, relu):
    """y, dh and db bit for bit; du sums the same intermediate in another fixed order: against float64 at the aggregation
    tests' 1e-5, with the ReLU decisions of the GPU run (a pre-activation within rounding of 0 has no decidable sign)."""
    took = set()
    for name, (faces, n) in _meshes(vpn).items():
        graph, blocks = vpn.ops.gcn_graph(faces, n, DEV), vpn.ops.gcn_blocks(faces, n, DEV)
        took.add(blocks is None)
        assert (blocks is None) == (name in ('strip_max_plus_1', 'random_131')), name
        c = _case(C, n, C + 7 * relu + n)
        norm = R.gcn_norm(R.unique_edges(faces), n)
        for with_u, with_b in ((True, True), (False, False), (True, False), (False, True)):
            mine = _two_hop(vpn, c, graph, blocks, with_u, with_b, relu)
            ref = _composition(vpn, c, graph, with_u, with_b, relu)
            assert torch.equal(mine[0], ref[0]) and torch.equal(mine[1], ref[1]), (name, with_u, with_b)
            if with_b:
                assert torch.equal(mine[3], ref[3]), name
            if with_u:
                h64, u64 = c['h'].double(), c['u'].double().requires_grad_(True)
                mask = (mine[0] > 0).cpu() if relu else None
                y64 = P.aggregate2(h64, u64, c['b'].double() if with_b else None, norm, mask=mask)
                y64.backward(c['g'].double())
                assert rel_err(mine[0].cpu(), y64.detach()) <= 1e-5, name
                assert rel_err(mine[2].cpu(), u64.grad) <= 1e-5, (name, rel_err(mine[2].cpu(), u64.grad))
            again = _two_hop(vpn, c, graph, blocks, with_u, with_b, relu)
            for p, q in zip(mine, again):
                assert (p is None and q is None) or torch.equal(p, q), name
    assert took == {False, True}


def test_aggregate2_skips_gradients_nobody_needs(vpn):
    for name in ('two_irregular_and_lone', 'strip_max_plus_1'):              # the LDS launch and the fallback
        faces, n = _meshes(vpn)[name]
        graph, blocks = vpn.ops.gcn_graph(faces, n, DEV), vpn.ops.gcn_blocks(faces, n, DEV)
        c = _case(8, n, 3)
        full = _two_hop(vpn, c, graph, blocks, True, True, True)
        for grads in (('h',), ('u',), ('b',), ('h', 'b'), ('u', 'b')):
            part = _two_hop(vpn, c, graph, blocks, True, True, True, grads=grads)
            assert torch.equal(part[0], full[0])
            for i, k in ((1, 'h'), (2, 'u'), (3, 'b')):
                assert (part[i] is None) if k not in grads else torch.equal(part[i], full[i]), (name, grads, k)


def test_aggregate2_captures_into_a_graph(vpn):
    faces, n = _meshes(vpn)['triangles_70']
    graph, blocks = vpn.ops.gcn_graph(faces, n, DEV), vpn.ops.gcn_blocks(faces, n, DEV)
    c, fresh = _case(260, n, 1), _case(260, n, 2)
    sh, su, sb = _leaves(c, True, True)
    sg = c['g'].to(DEV)

    def step():
        y = vpn.gcn_aggregate2(sh, su, sb, graph, blocks, relu=True)
        return [y.detach()] + list(torch.autograd.grad((y * sg).sum(), [sh, su, sb]))

    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        strict = step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for p, q in zip(strict, eager):
        assert torch.equal(p, q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        captured = step()
    cg.replay()
    torch.cuda.synchronize()
    for p, q in zip(captured, eager):
        assert torch.equal(p, q)
    with torch.no_grad():
        sh.copy_(fresh['h'].to(DEV))
        su.copy_(fresh['u'].to(DEV))
    cg.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    for p, q in zip(replayed, step()):
        assert torch.equal(p, q)
    assert not torch.equal(replayed[0], eager[0])


# ---- the skinny projection

PROJECT_SHAPES = [(1, 4, 1), (70, 512, 3), (130, 65, 4), (257, 8, 2)]


def _project(vpn, x, th, g, grads=('x', 'theta')):
    xd, td = x.to(DEV).requires_grad_('x' in grads), th.to(DEV).requires_grad_('theta' in grads)
    out = vpn.gcn_project(xd, td)
    out.backward(g.to(DEV))
    return out.detach(), xd.grad, td.grad


@pytest.mark.parametrize('shape', PROJECT_SHAPES, ids=lambda s: '-'.join(map(str, s)))
def test_project_against_float64(vpn, shape):
    """Per element |T - T64| <= 2 K 2^-24 A, A the same product of magnitudes in float64 and K the reduction length (Ci
    for out and dx, R for dtheta): the bound tests/test_trunkconv.py derives for a chain of K fused multiply-adds whose
    partial sums are merged by fewer than K further additions."""
    Rr, Ci, Co = shape
    gen = torch.Generator().manual_seed(Rr + Ci + Co)
    x, th, g = torch.randn(Rr, Ci, generator=gen), torch.randn(Ci, Co, generator=gen), torch.randn(Rr, Co, generator=gen)
    out, dx, dth = _project(vpn, x, th, g)
    x64, t64, g64 = x.double(), th.double(), g.double()
    want = dict(out=(out, P.project(x64, t64), P.project(x64.abs(), t64.abs()), Ci),
                dx=(dx, g64 @ t64.t(), g64.abs() @ t64.abs().t(), Ci),
                dtheta=(dth, x64.t() @ g64, x64.abs().t() @ g64.abs(), Rr))
    for k, (got, ref, mag, K) in want.items():
        assert got.shape == ref.shape, k
        excess = ((got.cpu().double() - ref).abs() - 2 * K * 2.0 ** -24 * mag).max()
        print(shape, k, 'rel err %.2e' % rel_err(got.cpu(), ref), 'worst excess over the bound %.2e' % float(excess))
        assert float(excess) <= 0, (k, float(excess))
    again = _project(vpn, x, th, g)
    assert torch.equal(again[0], out) and torch.equal(again[1], dx) and torch.equal(again[2], dth)
    only_x, only_t = _project(vpn, x, th, g, grads=('x',)), _project(vpn, x, th, g, grads=('theta',))
    assert only_x[2] is None and torch.equal(only_x[1], dx) and only_t[1] is None and torch.equal(only_t[2], dth)
    # leading axes fold into rows
    if Rr % 2 == 0:
        o3 = vpn.gcn_project(x.to(DEV).view(2, Rr // 2, Ci), th.to(DEV))
        assert o3.shape == (2, Rr // 2, Co) and torch.equal(o3.view(Rr, Co), out)


@pytest.mark.parametrize('shape', PROJECT_SHAPES, ids=lambda s: '-'.join(map(str, s)))
def test_project_is_exact_on_small_integers(vpn, shape):
    """x in -3..3, theta and g in -2..2: every partial sum is an integer far below 2^24, so any order gives the float64 result."""
    Rr, Ci, Co = shape
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (Rr, Ci), generator=gen).float()
    th = torch.randint(-2, 3, (Ci, Co), generator=gen).float()
    g = torch.randint(-2, 3, (Rr, Co), generator=gen).float()
    out, dx, dth = _project(vpn, x, th, g)
    assert torch.equal(out.cpu().double(), x.double() @ th.double())
    assert torch.equal(dx.cpu().double(), g.double() @ th.double().t())
    assert torch.equal(dth.cpu().double(), x.double().t() @ g.double())


# ---- the model

def _run_collapsed(vpn, model, verts, faces, maps, glob, rgbs, Wout, monkeypatch):
    """_run_gpu for a collapsed model: the ReLU decisions are the three gcn_aggregate2 outputs (the layers' modules are
    not called, so test_gcn's forward hooks would see nothing)."""
    import vpn_amd.modules.gcn as M
    masks, real = [], M.gcn_aggregate2

    def recording(*a, **k):
        y = real(*a, **k)
        masks.append((y > 0).detach().cpu())
        return y

    monkeypatch.setattr(M, 'gcn_aggregate2', recording)
    out = _run_gpu(vpn, model, verts, faces, maps, glob, rgbs, Wout)
    monkeypatch.undo()
    assert len(masks) == 3
    model.relu_masks = masks
    return out


def _errors(out, ref, verts):
    e = {'out': rel_err(out[0] - verts, ref[0] - verts.double()), 'dverts': rel_err(out[3], ref[3]),
         'dglob': rel_err(out[5], ref[5])}
    e.update({k: rel_err(out[2][k], gr) for k, gr in ref[2].items()})
    e.update({'dmap%d' % i: rel_err(a, b) for i, (a, b) in enumerate(zip(out[4], ref[4]))})
    return e


@pytest.mark.parametrize('factored', [False, True])
def test_model_against_float64(vpn, factored, monkeypatch):
    """GCNModel(img_feature_dim=8 + 4) on a mesh of two strips (70 + 61 vertices: two blocks), B = 2, plain and collapsed
    from one state_dict.  Every output and gradient norm-wise against the float64 restatement, each run with its own ReLU
    decisions; the bar is the plain-versus-factored one, 2e-4, or 4 x the plain model's own error, whichever is larger."""
    from vpn_amd.modules.gcn import GCNModel
    gen = torch.Generator().manual_seed(7)
    B, N = 2, 131
    faces = torch.cat([P._strip(70), P._strip(61) + 70])
    verts = torch.rand(B, N, 3, generator=gen) - 0.5
    maps = [torch.randn(B, c, s, s, generator=gen) for c, s in [(2, 8), (6, 4)]]
    glob = torch.randn(B, 4, generator=gen)
    rgbs = torch.zeros(B, 3, 32, 32)
    rgbs[0, :, 3:27, 2:25] = 0.5
    rgbs[1, :, 6:30, 5:22] = 0.5
    Wout = torch.randn(B, N, 3, generator=gen)
    assert vpn.ops.gcn_blocks(faces, N, DEV).tolist() == [0, 70, 131]
    torch.manual_seed(7)
    plain = GCNModel(img_feature_dim=8 + 4, v_num=N, factored_input=factored)
    with torch.no_grad():                       # non-zero biases, so that u = b_a Theta_b, their gradients and the masks matter
        for k in range(1, 7):
            getattr(plain, 'conv%d' % k).bias.uniform_(-0.05, 0.05)
    coll = GCNModel(img_feature_dim=8 + 4, v_num=N, factored_input=factored, collapse_pairs=True)
    coll.load_state_dict(plain.state_dict())
    a = _run_gpu(vpn, plain, verts, faces, maps, glob, rgbs, Wout)
    ea = _errors(a, _run_ref(plain, verts, faces, maps, glob, rgbs, Wout, masks=plain.relu_masks), verts)
    b = _run_collapsed(vpn, coll, verts, faces, maps, glob, rgbs, Wout, monkeypatch)
    eb = _errors(b, _run_ref(coll, verts, faces, maps, glob, rgbs, Wout, masks=coll.relu_masks), verts)
    assert sorted(ea) == sorted(eb) and len(ea) == 3 + 18 + 2
    print('factored' if factored else 'plain input', 'worst error against float64: pairs in a row %.2e (%s), collapsed %.2e (%s)'
          % (max(ea.values()), max(ea, key=ea.get), max(eb.values()), max(eb, key=eb.get)))
    for k in ea:
        assert eb[k] <= max(2e-4, 4 * ea[k]), (k, eb[k], ea[k])


def test_collapsed_step_makes_no_host_sync(vpn):
    from vpn_amd.modules.gcn import GCNModel
    B, K = 2, 16
    gen = torch.Generator().manual_seed(4)
    model = GCNModel(img_feature_dim=60 + 32, factored_input=True, collapse_pairs=True).to(DEV)
    maps = [torch.randn(B, c, s, s, generator=gen).to(DEV) for c, s in [(4, 32), (8, 16), (16, 8), (32, 4)]]
    glob = torch.randn(B, 32, generator=gen).to(DEV)
    rgbs = torch.zeros(B, 3, 64, 64)
    rgbs[:, :, 8:50, 4:60] = 0.5
    rgbs = rgbs.to(DEV)

    def prims():
        v = [(torch.rand(B, 3, generator=gen) * 0.2 + 0.05).to(DEV) for _ in range(K)]
        q = [torch.rand(B, 4, generator=gen).to(DEV) for _ in range(K)]
        t = [((torch.rand(B, 3, generator=gen) - 0.5) * 0.8).to(DEV) for _ in range(K)]
        return v, q, t

    def step(v, q, t):
        per = [[] for _ in range(B)]
        for k in range(K):
            ms = vpn.Meshing.sphere_meshing(v[k], q[k], t[k])
            for b in range(B):
                per[b].append(ms[b])
        meshes = [vpn.Meshing.compose_meshes(m) for m in per]
        loss = model(meshes, rgbs, maps, glob).square().mean()
        loss.backward()
        return loss, meshes[0]

    _, mesh = step(*prims())                                     # warm-up: templates, layouts, the graph and block caches
    blocks = vpn.ops.gcn_blocks(mesh.faces, mesh.vertices.shape[0], DEV)
    assert blocks is not None and blocks.numel() == K + 1         # the reference's mesh: a block a sphere, in LDS
    args = prims()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss, _ = step(*args)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert bool(torch.isfinite(loss))
