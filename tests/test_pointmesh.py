"""The point-to-surface distance on the GPU (vpn_amd.point_mesh_distance, point_mesh_nearest, ops.PointMeshFunction,
PointMeshDistanceLoss, csrc/pointmesh.hip) against the float64 statement of tests/pointmesh_ref.py: parity on
the cases of tests/test_pointmesh_cpu.py, one triangle in every region, exact cases, reproducibility, no host
synchronisation, graph capture, the module, the example."""
import os
import subprocess
import sys

import pytest
import torch

import meshreg_ref as M
import pointmesh_ref as R
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def vpn():
    import vpn_amd
    return vpn_amd


def _run(vpn, points, verts, faces, upstream=R.UPSTREAM, need=(True, True)):
    """(out [2], dpoints or None, dverts or None) of one forward + backward on the GPU, on the host."""
    p = points.to(DEV).requires_grad_(need[0])
    v = verts.to(DEV).requires_grad_(need[1])
    out = vpn.point_mesh_distance(p, v, faces)
    assert out.shape == (2,) and out.dtype == torch.float32 and out.is_cuda
    leaves = [t for t, n in zip((p, v), need) if n]
    grads = list(torch.autograd.grad((out * torch.tensor(upstream, device=DEV)).sum(), leaves)) if leaves else []
    dp = grads.pop(0).cpu() if need[0] else None
    dv = grads.pop(0).cpu() if need[1] else None
    return out.detach().cpu(), dp, dv


def _nearest(vpn, points, verts, faces):
    dist_p, fop, dist_f, pof = vpn.point_mesh_nearest(points.to(DEV), verts.to(DEV), faces)
    B, P, F = points.shape[0], points.shape[1], faces.shape[0]
    assert dist_p.shape == (B, P) and fop.shape == (B, P) and dist_f.shape == (B, F) and pof.shape == (B, F)
    assert fop.dtype == torch.int32 and pof.dtype == torch.int32 and not dist_p.requires_grad
    assert 0 <= int(fop.min()) and int(fop.max()) < F and 0 <= int(pof.min()) and int(pof.max()) < P
    return dist_p.cpu(), fop.cpu(), dist_f.cpu(), pof.cpu()


@pytest.mark.parametrize('name,B,P', R.CASES, ids=lambda v: str(v))
def test_parity_with_float64(vpn, name, B, P):
    """out within 1e-4 relative of float64; dist_p and dist_f within 1e-4 (conftest.rel_err); for EVERY query the float64
    distance of the pair the GPU's index names exceeds the float64 minimum by at most 1e-4 of the sample's largest minimum;
    dpoints and dverts for upstream (0.3, -2) against the float64 gradient at the GPU's indices within max(1e-4, 4 x own), own
    the fp32 restatement's error at the same indices.  Measured on an MI355X, worst over the cases: out 3.7e-7, distances
    9.6e-7, index excess 2.1e-16, dpoints 2.1e-5 against own 2.0e-5 (two_components; 2.0e-5 against 4.7e-5 on fan_70), dverts
    3.0e-5 against own 2.4e-5 (two_components)."""
    points, verts, faces = R.case_inputs(name, B, P)
    dp64, _, df64, _, table, out64 = R.reference64(name, B, P)
    out, dpoints, dverts = _run(vpn, points, verts, faces)
    dist_p, fop, dist_f, pof = _nearest(vpn, points, verts, faces)
    err_out = [abs(float(out[k]) - float(out64[k])) / float(out64[k]) for k in range(2)]
    err_d = [rel_err(dist_p, dp64), rel_err(dist_f, df64)]
    excess = [float(R.index_excess(table, dp64, fop, 2).max()), float(R.index_excess(table, df64, pof, 1).max())]
    g64 = R.gradient(points, verts, faces, fop, pof, R.UPSTREAM)
    g32 = R.gradient(points, verts, faces, fop, pof, R.UPSTREAM, torch.float32)
    own = [rel_err(a, b) for a, b in zip(g32, g64)]
    err_g = [rel_err(dpoints, g64[0]), rel_err(dverts, g64[1])]
    print('%s B %d P %d: out %.1e %.1e  distances %.1e %.1e  index excess %.1e %.1e  dpoints %.1e (own %.1e)  dverts %.1e (own %.1e)'
          % (name, B, P, *err_out, *err_d, *excess, err_g[0], own[0], err_g[1], own[1]))
    assert torch.isfinite(out).all() and torch.isfinite(dpoints).all() and torch.isfinite(dverts).all()
    assert max(err_out) <= 1e-4, err_out
    assert max(err_d) <= 1e-4, err_d
    assert max(excess) <= 1e-4, excess
    for k in range(2):
        assert err_g[k] <= max(1e-4, 4 * own[k]), (k, err_g[k], own[k])
    # the means are the means of what point_mesh_nearest reports
    assert abs(float(out[0]) - float(dist_p.double().mean())) <= 1e-5 * float(dist_p.double().mean())
    assert abs(float(out[1]) - float(dist_f.double().mean())) <= 1e-5 * float(dist_f.double().mean())


def test_one_triangle_in_every_region(vpn):
    """One point against one scalene triangle per sample (F = 1, P = 1), several in the face region, the three edge regions and
    the three corner regions, above and below the plane: the value and both gradients of every sample within 1e-4 of float64,
    relative to that sample's own largest entry (a well-shaped triangle and distances of 0.0125 and more: the closest point is
    good to about 1e-7 of the coordinates, 1e-5 of the shortest p - c)."""
    points, verts, faces, regions = R.one_triangle()
    N = points.shape[0]
    assert sorted(set(regions.tolist())) == list(range(7))
    out, dpoints, dverts = _run(vpn, points, verts, faces)
    dist_p, fop, dist_f, pof = _nearest(vpn, points, verts, faces)
    assert int(fop.abs().max()) == 0 and int(pof.abs().max()) == 0 and torch.equal(dist_p, dist_f)
    p64, v64 = points.double(), verts.double()
    d64, _, region64 = R.closest(p64[:, 0], v64[:, 0], v64[:, 1], v64[:, 2])
    assert torch.equal(region64, regions)
    gp64, gv64 = R.gradient(points, verts, faces, fop, pof, R.UPSTREAM)
    worst = [0.0, 0.0, 0.0]
    for i in range(N):
        e = [abs(float(dist_p[i, 0]) - float(d64[i])) / float(d64[i]), rel_err(dpoints[i], gp64[i]), rel_err(dverts[i], gv64[i])]
        assert max(e) <= 1e-4, (i, R.REGIONS[int(regions[i])], e)
        worst = [max(a, b) for a, b in zip(worst, e)]
    print('one triangle, %d points: value %.1e  dpoints %.1e  dverts %.1e' % (N, *worst))
    assert abs(float(out[0]) - float(d64.mean())) <= 1e-4 * float(d64.mean())


def test_exact_cases(vpn):
    """Coordinates that are small multiples of 1/4: fp32 and float64 agree to the bit."""
    tri = [[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]
    # a point between two disjoint parallel triangles takes the lower face; of two points equidistant from a face the lower
    verts = torch.tensor([tri + [[x, y, 1.0] for x, y, _ in tri]])
    faces = torch.tensor([[0, 1, 2], [3, 4, 5]])
    points = torch.tensor([[[0.25, 0.25, 0.5], [0.25, 0.25, -0.5]]])
    dist_p, fop, dist_f, pof = _nearest(vpn, points, verts, faces)
    assert dist_p[0].tolist() == [0.25, 0.25] and fop[0].tolist() == [0, 0]
    assert dist_f[0].tolist() == [0.25, 0.25] and pof[0].tolist() == [0, 0]
    dist_p, fop, dist_f, pof = _nearest(vpn, points, verts, faces.flip(0))         # face 0 is now the upper triangle
    assert dist_p[0].tolist() == [0.25, 0.25] and fop[0].tolist() == [0, 1]
    assert dist_f[0].tolist() == [0.25, 0.25] and pof[0].tolist() == [0, 0]
    # a point on a face: distance exactly 0, exactly 0 added to every gradient
    out, dpoints, dverts = _run(vpn, torch.tensor([[[0.25, 0.25, 0.0]]]), verts[:, :3].contiguous(), faces[:1])
    assert out.tolist() == [0.0, 0.0] and float(dpoints.abs().max()) == 0.0 and float(dverts.abs().max()) == 0.0
    # a collinear face is its segment, three coincident vertices are a point; the third face is sound
    verts = torch.tensor([[[0.0, 0, 0], [2, 0, 0], [1, 0, 0], [0, 0, 2], [0, 2, 0], [2, 2, 0]]])
    faces = torch.tensor([[0, 1, 2], [3, 3, 3], [0, 4, 5]])
    points = torch.tensor([[[1.0, 1, 1], [0, 0, 3], [0.5, 1, 0], [3, 0, 0]]])
    dist_p, fop, dist_f, pof = _nearest(vpn, points, verts, faces)
    dp64, fop64, df64, pof64, _ = R.nearest(points, verts, faces)
    assert dist_p[0].tolist() == [1.0, 1.0, 0.0, 1.0] == dp64[0].tolist() and fop[0].tolist() == [2, 1, 2, 0] == fop64[0].tolist()
    assert dist_f[0].tolist() == [1.0, 1.0, 0.0] == df64[0].tolist() and pof[0].tolist() == [2, 1, 2] == pof64[0].tolist()
    out, dpoints, dverts = _run(vpn, points, verts, faces)
    gp64, gv64 = R.gradient(points, verts, faces, fop, pof, R.UPSTREAM)
    assert torch.isfinite(dpoints).all() and torch.isfinite(dverts).all()
    assert torch.allclose(dpoints.double(), gp64, rtol=1e-6, atol=1e-7) and torch.allclose(dverts.double(), gv64, rtol=1e-6, atol=1e-7)


def test_each_gradient_alone_and_neither(vpn):
    points, verts, faces = R.case_inputs('uv_sphere', 3, 257)
    out, dpoints, dverts = _run(vpn, points, verts, faces)
    out_p, only_p, none_v = _run(vpn, points, verts, faces, need=(True, False))
    out_v, none_p, only_v = _run(vpn, points, verts, faces, need=(False, True))
    assert none_v is None and none_p is None
    assert torch.equal(out_p, out) and torch.equal(out_v, out) and torch.equal(only_p, dpoints) and torch.equal(only_v, dverts)
    plain = vpn.point_mesh_distance(points.to(DEV), verts.to(DEV), faces)
    assert not plain.requires_grad and plain.grad_fn is None and torch.equal(plain.cpu(), out)     # nothing saved, nothing to run


def test_faces_on_the_device_and_as_int32(vpn):
    points, verts, faces = R.case_inputs('uv_sphere', 3, 257)
    a = _run(vpn, points, verts, faces)
    na = _nearest(vpn, points, verts, faces)
    for f in (faces.to(DEV), faces.int(), faces.int().to(DEV)):
        b = _run(vpn, points, verts, f)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert all(torch.equal(x, y) for x, y in zip(na, _nearest(vpn, points, verts, f)))


def test_runs_are_bit_equal(vpn):
    points, verts, faces = R.case_inputs('composed', 1, 300)
    a = _run(vpn, points, verts, faces) + _nearest(vpn, points, verts, faces)
    b = _run(vpn, points, verts, faces) + _nearest(vpn, points, verts, faces)
    assert len(a) == 7 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_no_host_sync_and_graph_replay(vpn):
    points, verts, faces = R.case_inputs('composed', 1, 300)
    fd = faces.to(DEV)
    up = torch.tensor(R.UPSTREAM, device=DEV)
    sp = points.to(DEV).requires_grad_(True)                              # the static inputs of the capture
    sv = verts.to(DEV).requires_grad_(True)

    def step():
        out = vpn.point_mesh_distance(sp, sv, fd)
        return [out.detach()] + list(torch.autograd.grad((out * up).sum(), [sp, sv])) + list(vpn.point_mesh_nearest(sp, sv, fd))

    eager = [t.clone() for t in step()]                                   # warm-up: the incidence table, library handles
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        strict = step()                                                   # a second call on a cached incidence
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for p, q in zip(strict, eager):
        assert torch.equal(p, q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for p, q in zip(captured, eager):
        assert torch.equal(p, q)
    with torch.no_grad():
        sv.mul_(1.25).add_(0.01)
        sp.add_(0.02)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    again = step()
    for p, q in zip(replayed, again):
        assert torch.equal(p, q)
    assert not torch.equal(replayed[0], eager[0])


def test_module_with_a_zero_weight(vpn):
    points, verts, faces = R.case_inputs('uv_sphere', 3, 257)
    _, _, _, _, _, out64 = R.reference64('uv_sphere', 3, 257)
    for w in ((1.0, 0.0), (0.0, 0.5), (0.7, 0.5)):
        loss = vpn.PointMeshDistanceLoss(*w)
        p, v = points.to(DEV).requires_grad_(True), verts.to(DEV).requires_grad_(True)
        total = loss(p, v, faces)
        total.backward()
        want = w[0] * float(out64[0]) + w[1] * float(out64[1])
        assert abs(float(total.detach()) - want) <= 1e-4 * abs(want)
        _, fop, _, pof = _nearest(vpn, points, verts, faces)
        gp64, gv64 = R.gradient(points, verts, faces, fop, pof, w)
        assert rel_err(p.grad.cpu(), gp64) <= 1e-4 and rel_err(v.grad.cpu(), gv64) <= 1e-4
        assert loss.last.is_cuda and not loss.last.requires_grad and loss.last.shape == (2,)
        assert abs(float(loss.last[0]) - float(out64[0])) <= 1e-4 * float(out64[0])       # both parts are reported whatever the weights
        assert abs(float(loss.last[1]) - float(out64[1])) <= 1e-4 * float(out64[1])


def test_gradient_reaches_the_gcn_parameters(vpn):
    from vpn_amd.modules.gcn import GCNModel
    from vpn_amd.modules.meshing import TriangleMesh
    B, N = 2, 16
    gen = torch.Generator().manual_seed(16)
    faces, _ = M.strip(N)
    i = torch.arange(N, dtype=torch.float32)
    verts = torch.stack([0.05 * i - 0.4, 0.1 * (i % 2), 0.03 * torch.sin(0.7 * i)], 1)[None].repeat(B, 1, 1)
    torch.manual_seed(16)
    model = GCNModel(img_feature_dim=4 + 8 + 4, v_num=N).to(DEV)
    maps = [torch.randn(B, c, s, s, generator=gen).to(DEV) for c, s in [(4, 8), (8, 4)]]
    glob = torch.randn(B, 4, generator=gen).to(DEV)
    rgbs = torch.zeros(B, 3, 32, 32)
    rgbs[:, :, 4:28, 6:26] = 0.5
    fd = faces.to(DEV)
    meshes = [TriangleMesh(verts[b].to(DEV), fd) for b in range(B)]
    predict_vertices = model(meshes, rgbs.to(DEV), maps, glob)
    points = (torch.rand(B, 40, 3, generator=gen) - 0.5).to(DEV)
    loss = vpn.PointMeshDistanceLoss(1.0, 0.5)(points, predict_vertices, fd)
    loss.backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values()), [k for k, g in grads.items() if g is None]
    assert float(grads['fc.2.bias'].abs().max()) > 0 and float(grads['conv1.weight'].abs().max()) > 0


def test_train_gcn_step_example_runs_with_surface_loss():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'train_gcn_step.py'), '--surface-loss', '1,1',
                        '--steps', '2', '--batch', '2'], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith('step ')]
    assert len(lines) == 2 and all('Surface Loss = ' in l for l in lines), r.stdout
    for l in lines:
        value = float(l.split('Surface Loss = ')[1].split(' ')[0])
        assert value == value and abs(value) < float('inf') and value > 0, l
