"""GPU tests of the GCN refinement stage (csrc/gcn.hip, ops.Gcn*, modules/gcn.py) against the g7 fixtures captured from
the reference's gcn.py and against the float64 restatement of tests/gcn_ref.py."""
import os
import subprocess
import sys

import pytest
import torch

import gcn_ref as R
from conftest import ROOT, load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def vpn():
    import vpn_amd
    return vpn_amd


def composed_sphere_vertices(B, K, gen):
    from vpn_amd.modules.meshing import uv_sphere
    sv, sf = uv_sphere()
    verts = torch.stack([torch.cat([sv * (torch.rand(3, generator=gen) * 0.2 + 0.1) + (torch.rand(3, generator=gen) - 0.5) * 0.6
                                    for _ in range(K)]) for _ in range(B)])
    faces = torch.cat([sf + sv.shape[0] * k for k in range(K)])
    return verts, faces


def test_bounds_bit_exact(vpn):
    z = load_golden('g7_gcn_bounds')
    out = vpn.ops.gcn_bounds(z['imgs'].to(DEV)).cpu()
    assert torch.equal(out, z['bounds']), (out, z['bounds'])
    assert torch.equal(vpn.modules.GCNModel.get_bound_of_images(z['imgs'].to(DEV)).cpu(), z['bounds'])


def test_encoding_and_pooling_against_g7(vpn):
    from vpn_amd.modules.gcn import GCNModel
    z = load_golden('g7_gcn_encoding')
    enc = GCNModel.positional_encoding(z['verts'].to(DEV)).cpu()
    assert rel_err(enc, z['encoding']) <= 1e-5
    z = load_golden('g7_gcn_pooling')
    maps = [z['map%d' % i].to(DEV).requires_grad_(True) for i in range(4)]
    v = z['verts'].to(DEV).requires_grad_(True)
    bounds = GCNModel.get_bound_of_images(z['rgbs'].to(DEV))
    assert torch.equal(bounds.cpu(), z['bounds'])
    p = GCNModel.perceptual_feature_pooling(maps, v, bounds)
    assert rel_err(p.detach().cpu(), z['pooled']) <= 1e-5
    (p * z['W'].to(DEV)).sum().backward()
    assert rel_err(v.grad.cpu(), z['grad_verts']) <= 1e-4
    for i, m in enumerate(maps):
        assert rel_err(m.grad.cpu(), z['grad_map%d' % i]) <= 1e-4, i
    # the rows that hold an extent carry a sum over all vertices and set the norm-wise scale: the others, and they, each
    # element-wise against float64, no worse than 1e-3 nor than 4 x the fixture's own fp32 error (tests/gcn_input_ref.py)
    import gcn_input_ref as G
    fm = [z['map%d' % i] for i in range(4)]
    rows = dict(masked=G.undecidable_rows(z['verts'], z['bounds'], fm), extent=G.extent_rows(z['verts']))
    v64 = z['verts'].double().requires_grad_(True)
    (R.pooling([m.double() for m in fm], v64, z['bounds'].double()) * z['W'].double()).sum().backward()
    mine, own = G.split_errors(v.grad.cpu(), v64.grad, rows), G.split_errors(z['grad_verts'], v64.grad, rows)
    print('g7_gcn_pooling dverts split (O, E): kernel %.2e %.2e, fixture %.2e %.2e' % (mine + own))
    assert mine[0] <= G.split_bar(own[0]) and mine[1] <= G.split_bar(own[1]), (mine, own)


@pytest.mark.parametrize('C', [3, 64, 512, 1511])
@pytest.mark.parametrize('relu', [False, True])
def test_aggregation_against_float64(vpn, C, relu):
    gen = torch.Generator().manual_seed(C + relu)
    verts, faces = composed_sphere_vertices(2, 3, gen)
    B, N = 2, verts.shape[1]
    graph = vpn.ops.gcn_graph(faces, N, DEV)
    h = torch.randn(B, N, C, generator=gen)
    bias = torch.randn(C, generator=gen)
    g = torch.randn(B, N, C, generator=gen)
    hd, bd = h.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    y = vpn.ops.GcnAggregateFunction.apply(hd, bd, graph.row_ptr, graph.col, graph.w, relu)
    y.backward(g.to(DEV))
    norm = R.gcn_norm(R.unique_edges(faces), N)
    h64, b64 = h.double().requires_grad_(True), bias.double().requires_grad_(True)
    y64 = R.aggregate(h64, norm, b64)
    if relu:
        y64 = y64.relu()
    y64.backward(g.double())
    assert rel_err(y.detach().cpu(), y64) <= 1e-5
    assert rel_err(hd.grad.cpu(), h64.grad) <= 1e-5
    assert rel_err(bd.grad.cpu(), b64.grad) <= 1e-5


def _model_case(vpn, B, K, map_shapes, G, img, seed, use_pe=True):
    from vpn_amd.modules.gcn import GCNModel
    from vpn_amd.modules.meshing import TriangleMesh
    gen = torch.Generator().manual_seed(seed)
    verts, faces = composed_sphere_vertices(B, K, gen)
    N = verts.shape[1]
    maps = [torch.randn(B, c, s, s, generator=gen) for c, s in map_shapes]
    glob = torch.randn(B, G, generator=gen)
    rgbs = torch.zeros(B, 3, img, img)
    for b in range(B):
        y0, x0 = int(torch.randint(1, img // 4, (1,), generator=gen)), int(torch.randint(1, img // 4, (1,), generator=gen))
        rgbs[b, :, y0:img - y0, x0:img - 2 * x0] = 0.5
    torch.manual_seed(seed)
    model = GCNModel(img_feature_dim=sum(c for c, _ in map_shapes) + G, v_num=N, use_position_encoding=use_pe)
    with torch.no_grad():                       # non-zero biases, so that their gradients and the ReLU masks matter
        for k in range(1, 7):
            getattr(model, 'conv%d' % k).bias.uniform_(-0.05, 0.05)
    Wout = torch.randn(B, N, 3, generator=gen)
    return model, verts, faces, maps, glob, rgbs, Wout


def _run_gpu(vpn, model, verts, faces, maps, glob, rgbs, Wout):
    from vpn_amd.modules.meshing import TriangleMesh
    m = model.to(DEV)
    m.zero_grad()
    v = verts.to(DEV).requires_grad_(True)
    fd = faces.to(DEV)
    mp = [x.to(DEV).requires_grad_(True) for x in maps]
    g = glob.to(DEV).requires_grad_(True)
    meshes = [TriangleMesh(v[b], fd) for b in range(v.shape[0])]
    masks = []
    hooks = [getattr(m, 'conv%d' % k).register_forward_hook(lambda _m, _i, o: masks.append((o > 0).detach().cpu()))
             for k in (2, 4, 6)]
    try:
        out = m(meshes, rgbs.to(DEV), mp, g)
    finally:
        for h in hooks:
            h.remove()
    m.relu_masks = masks
    loss = (out * Wout.to(DEV)).sum()
    loss.backward()
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    return out.detach().cpu(), loss.detach().cpu(), grads, v.grad.cpu(), [x.grad.cpu() for x in mp], g.grad.cpu()


def _run_ref(model, verts, faces, maps, glob, rgbs, Wout, use_pe=True, masks=None):
    """float64 restatement; masks: the ReLU decisions the GPU run took.  A pre-activation within fp32 rounding of 0 has
    no decidable sign, and one flipped decision moves a weight gradient summed over 16k rows by ~1e-3 relative; the
    decisions are taken from the GPU run after checking that they differ from float64's only at such values."""
    params = {k: p.detach().cpu().double().requires_grad_(True) for k, p in model.state_dict().items()}
    v = verts.double().requires_grad_(True)
    mp = [x.double().requires_grad_(True) for x in maps]
    g = glob.double().requires_grad_(True)
    if masks is not None:
        pre = []
        with torch.no_grad():
            R.model(params, v, rgbs, mp, g, faces, use_pe, pre=pre)
        for m, p in zip(masks, pre):
            flip = m != (p > 0)
            assert float(p[flip].abs().max()) <= 1e-5 * float(p.abs().max()) if bool(flip.any()) else True
    out = R.model(params, v, rgbs, mp, g, faces, use_pe, masks=masks)
    loss = (out * Wout.double()).sum()
    loss.backward()
    return out.detach(), loss.detach(), {k: p.grad for k, p in params.items()}, v.grad, [x.grad for x in mp], g.grad


@pytest.mark.parametrize('case', ['small', 'small_no_pe', 'reference'])
def test_model_against_float64(vpn, case):
    if case == 'reference':
        args = dict(B=8, K=16, map_shapes=[(64, 32), (128, 16), (256, 8), (512, 4)], G=512, img=128, seed=5)
    else:
        args = dict(B=2, K=2, map_shapes=[(4, 32), (8, 16), (16, 8), (32, 4)], G=16, img=64, seed=3)
    use_pe = case != 'small_no_pe'
    model, verts, faces, maps, glob, rgbs, Wout = _model_case(vpn, use_pe=use_pe, **args)
    out = _run_gpu(vpn, model, verts, faces, maps, glob, rgbs, Wout)
    ref = _run_ref(model, verts, faces, maps, glob, rgbs, Wout, use_pe, masks=model.relu_masks)
    assert rel_err(out[0] - verts, ref[0] - verts.double()) <= 1e-4            # the deformation, not the vertices
    assert abs(float(out[1]) - float(ref[1])) <= 1e-4 * abs(float(ref[1]))
    for k, gr in ref[2].items():
        assert rel_err(out[2][k], gr) <= 1e-4, k
    assert rel_err(out[3], ref[3]) <= 1e-4
    for a, b in zip(out[4], ref[4]):
        assert rel_err(a, b) <= 1e-4
    assert rel_err(out[5], ref[5]) <= 1e-4


def test_checkpoint_layouts_give_identical_outputs(vpn):
    from vpn_amd.modules.gcn import GCNModel, to_pyg2_state_dict
    model, verts, faces, maps, glob, rgbs, Wout = _model_case(vpn, 2, 2, [(4, 32), (8, 16), (16, 8), (32, 4)], 16, 64, 11)
    sd = model.state_dict()
    outs = []
    for layout in (sd, to_pyg2_state_dict(sd)):
        m = GCNModel(img_feature_dim=60 + 16, v_num=verts.shape[1])
        m.load_state_dict(layout)
        outs.append(_run_gpu(vpn, m, verts, faces, maps, glob, rgbs, Wout)[0])
    assert torch.equal(outs[0], outs[1])


def test_new_kernels_are_deterministic(vpn):
    gen = torch.Generator().manual_seed(9)
    verts, faces = composed_sphere_vertices(4, 16, gen)
    B, N = verts.shape[:2]
    graph = vpn.ops.gcn_graph(faces, N, DEV)
    maps = [torch.randn(B, c, s, s, generator=gen).to(DEV) for c, s in [(64, 32), (128, 16), (256, 8), (512, 4)]]
    glob = torch.randn(B, 512, generator=gen).to(DEV)
    rgbs = torch.zeros(B, 3, 128, 128)
    rgbs[:, :, 20:100, 10:110] = 0.5
    rgbs = rgbs.to(DEV)
    h = torch.randn(B, N, 512, generator=gen).to(DEV)
    gy = torch.randn(B, N, 512, generator=gen).to(DEV)
    gx = torch.randn(B, N, 39 + 960 + 512, generator=gen).to(DEV)

    def run():
        v = verts.to(DEV).requires_grad_(True)
        mp = [m.clone().requires_grad_(True) for m in maps]
        g = glob.clone().requires_grad_(True)
        bounds = vpn.ops.gcn_bounds(rgbs)
        x = vpn.ops.GcnInputFunction.apply(v, bounds, g, 39, *mp)
        x.backward(gx)
        hh = h.clone().requires_grad_(True)
        b = torch.zeros(512, device=DEV).requires_grad_(True)
        y = vpn.ops.GcnAggregateFunction.apply(hh, b, graph.row_ptr, graph.col, graph.w, True)
        y.backward(gy)
        return [bounds, x, v.grad, g.grad, y, hh.grad, b.grad] + [m.grad for m in mp]

    a, b = run(), run()
    for i, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p, q), i


def test_step_makes_no_host_sync(vpn):
    from vpn_amd.modules.gcn import GCNModel
    B, K = 2, 16
    gen = torch.Generator().manual_seed(4)
    model = GCNModel(img_feature_dim=60 + 32).to(DEV)
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
        out = model(meshes, rgbs, maps, glob)
        loss = out.square().mean()
        loss.backward()
        return loss

    step(*prims())                                           # warm-up: templates, layouts, the graph cache
    args = prims()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss = step(*args)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert bool(torch.isfinite(loss))


def test_train_gcn_step_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'train_gcn_step.py'), '--steps', '5'],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith('step ')]
    assert len(lines) == 5, r.stdout
    for l in lines:
        cd, emd = float(l.split('CD Loss = ')[1].split(',')[0]), float(l.split('EMD Loss = ')[1])
        assert cd == cd and emd == emd and abs(cd) < float('inf') and abs(emd) < float('inf'), l
