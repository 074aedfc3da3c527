"""The mesh regularisers on the GPU (vpn_amd.mesh_regularizers, ops.MeshRegFunction, MeshRegularizationLoss,
csrc/meshreg.hip) against the float64 statement of tests/meshreg_ref.py: parity on every mesh of
tests/test_meshreg_cpu.py, degenerate geometry, reproducibility, no host synchronisation, graph capture, the module."""
import os
import subprocess
import sys

import pytest
import torch

import meshreg_ref as M
from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
UPSTREAM = (0.3, -2.0, 5.0)
ALL_AND_EACH = (M.TERMS,) + tuple((t,) for t in M.TERMS)


@pytest.fixture(scope='module')
def vpn():
    import vpn_amd
    return vpn_amd


def _run(vpn, verts, faces, l0, terms, upstream=UPSTREAM):
    """(values [3], dverts) of one forward + backward on the GPU, on the host."""
    v = verts.to(DEV).requires_grad_(True)
    out = vpn.mesh_regularizers(v, faces, l0, terms)
    assert out.shape == (3,) and out.dtype == torch.float32 and out.is_cuda
    (dv,) = torch.autograd.grad((out * torch.tensor(upstream, device=DEV)).sum(), v)
    return out.detach().cpu(), dv.cpu()


def _check(got, want, terms, bar_grad, what):
    (out, dv), (out64, dv64) = got, want
    assert torch.isfinite(out).all() and torch.isfinite(dv).all(), what
    for k, t in enumerate(M.TERMS):
        if t not in terms:
            assert float(out[k]) == 0.0, (what, t)
        else:
            assert abs(float(out[k]) - float(out64[k])) <= 1e-4 * abs(float(out64[k])), (what, t, float(out[k]), float(out64[k]))
    if float(dv64.abs().max()) > 0:
        err = rel_err(dv, dv64)
        print('%s: dverts rel err %.2e (bar %.2e)' % (what, err, bar_grad))
        assert err <= bar_grad, (what, err, bar_grad)
    else:
        assert float(dv.abs().max()) == 0.0, what


CASES = [(name, B) for name in sorted(M.MESHES) for B in (1, 3)] + [('composed', 2)]


@pytest.mark.parametrize('name,B', CASES, ids=lambda v: str(v))
def test_parity_with_float64(vpn, name, B):
    """Values and dverts within 1e-4 of float64 (conftest.rel_err), l0 = 0 and 0.05, all terms and each alone, upstream
    gradient (0.3, -2, 5).  The normal term alone: max(1e-4, 4 x own), own the fp32 restatement's error on the same input."""
    faces, n = M.mesh(name)
    verts = M.vertices(name, B)
    for l0 in (0.0, 0.05):
        for terms in ALL_AND_EACH:
            want = M.reference64(name, B, l0, terms, UPSTREAM)
            bar = 1e-4
            if terms == ('normal',) and float(want[1].abs().max()) > 0:
                bar = max(1e-4, 4 * rel_err(M.reference32(name, B, l0, terms, UPSTREAM)[1], want[1]))
            _check(_run(vpn, verts, faces, l0, terms), want, terms, bar, '%s B %d l0 %g %s' % (name, B, l0, '+'.join(terms)))


def test_faces_on_the_device_and_as_int32(vpn):
    faces, n = M.mesh('uv_sphere')
    verts = M.vertices('uv_sphere', 3)
    a = _run(vpn, verts, faces, 0.05, M.TERMS)
    for f in (faces.to(DEV), faces.int(), faces.int().to(DEV)):
        b = _run(vpn, verts, f, 0.05, M.TERMS)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_degenerate_geometry(vpn):
    """A zero-area face, a zero-length edge with l0 > 0, two coincident vertices: finite, and the restatement's values."""
    v, f, l0 = M.degenerate()
    for terms in ALL_AND_EACH:
        _check(_run(vpn, v, f, l0, terms), M.reference(v, f, l0, terms, UPSTREAM), terms, 1e-4, 'degenerate ' + '+'.join(terms))
    out, dv = _run(vpn, v, f, l0, ('edge',), (1.0, 1.0, 1.0))
    topo = M.topology(f, 6)
    # vertex 5 coincides with 4: of its two edges only (3, 5) pulls
    d = (v[0, 5] - v[0, 3]).double()
    want = (2.0 / len(topo['edges'])) * (1 - l0 / float(d.norm())) * d
    assert torch.allclose(dv[0, 5].double(), want, rtol=1e-5, atol=1e-7)


def test_a_term_that_is_off_ignores_its_upstream_gradient(vpn):
    faces, n = M.mesh('uv_sphere')
    verts = M.vertices('uv_sphere', 1)
    a = _run(vpn, verts, faces, 0.0, ('lap',), (float('nan'), 1.0, float('inf')))
    b = _run(vpn, verts, faces, 0.0, ('lap',), (0.0, 1.0, 0.0))
    assert torch.equal(a[1], b[1]) and torch.isfinite(a[1]).all()
    out, dv = _run(vpn, verts, faces, 0.0, ())
    assert float(out.abs().max()) == 0.0 and float(dv.abs().max()) == 0.0


def test_runs_are_bit_equal(vpn):
    faces, n = M.mesh('composed')
    verts = M.vertices('composed', 2)
    a, b = _run(vpn, verts, faces, 0.05, M.TERMS), _run(vpn, verts, faces, 0.05, M.TERMS)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_no_gradient_wanted_saves_nothing(vpn):
    faces, n = M.mesh('uv_sphere')
    v = M.vertices('uv_sphere', 2).to(DEV)
    out = vpn.mesh_regularizers(v, faces)
    assert not out.requires_grad
    want = _run(vpn, v.cpu(), faces, 0.0, M.TERMS)[0]
    assert torch.equal(out.cpu(), want)


def test_no_host_sync_and_graph_replay(vpn):
    faces, n = M.mesh('composed')
    fd = faces.to(DEV)
    up = torch.tensor(UPSTREAM, device=DEV)
    sv = M.vertices('composed', 2).to(DEV).requires_grad_(True)          # the static input of the capture

    def step():
        out = vpn.mesh_regularizers(sv, fd, 0.05)
        return [out.detach()] + list(torch.autograd.grad((out * up).sum(), [sv]))

    eager = [t.clone() for t in step()]                                   # warm-up: the topology, library handles
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        strict = step()                                                   # a second call on a cached topology
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
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    again = step()
    for p, q in zip(replayed, again):
        assert torch.equal(p, q)
    assert not torch.equal(replayed[0], eager[0])


def test_module_is_the_weighted_restatement(vpn):
    faces, n = M.mesh('uv_sphere')
    verts = M.vertices('uv_sphere', 3)
    w = (1.0, 0.0, 0.5)
    loss = vpn.MeshRegularizationLoss(*w, edge_target=0.05)
    assert loss.terms == ('edge', 'normal')
    v = verts.to(DEV).requires_grad_(True)
    total = loss(v, faces)
    total.backward()
    out64, dv64 = M.reference(verts, faces, 0.05, ('edge', 'normal'), w)
    want = float((out64 * torch.tensor(w, dtype=torch.float64)).sum())
    assert abs(float(total.detach()) - want) <= 1e-4 * abs(want)
    assert rel_err(v.grad.cpu(), dv64) <= 1e-4
    assert loss.last.is_cuda and not loss.last.requires_grad and float(loss.last[1]) == 0.0       # the dropped term
    assert abs(float(loss.last[0]) - float(out64[0])) <= 1e-4 * float(out64[0])
    assert abs(float(loss.last[2]) - float(out64[2])) <= 1e-4 * float(out64[2])


def test_gradient_reaches_the_gcn_parameters(vpn):
    from vpn_amd.modules.gcn import GCNModel
    from vpn_amd.modules.meshing import TriangleMesh
    B, N = 2, 16
    gen = torch.Generator().manual_seed(16)
    faces, _ = M.strip(N)
    verts = M.vertices('strip_7', 1).new_zeros(B, N, 3)
    i = torch.arange(N, dtype=torch.float32)
    verts[:] = torch.stack([0.05 * i - 0.4, 0.1 * (i % 2), 0.03 * torch.sin(0.7 * i)], 1)
    torch.manual_seed(16)
    model = GCNModel(img_feature_dim=4 + 8 + 4, v_num=N).to(DEV)
    maps = [torch.randn(B, c, s, s, generator=gen).to(DEV) for c, s in [(4, 8), (8, 4)]]
    glob = torch.randn(B, 4, generator=gen).to(DEV)
    rgbs = torch.zeros(B, 3, 32, 32)
    rgbs[:, :, 4:28, 6:26] = 0.5
    fd = faces.to(DEV)
    meshes = [TriangleMesh(verts[b].to(DEV), fd) for b in range(B)]
    predict_vertices = model(meshes, rgbs.to(DEV), maps, glob)
    loss = vpn.MeshRegularizationLoss(1.0, 0.5, 0.1)(predict_vertices, fd)
    loss.backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values()), [k for k, g in grads.items() if g is None]
    assert float(grads['fc.2.bias'].abs().max()) > 0 and float(grads['conv1.weight'].abs().max()) > 0


def test_train_gcn_step_example_runs_with_mesh_reg():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'train_gcn_step.py'), '--mesh-reg', '0.1,0.5,0.01',
                        '--steps', '2', '--batch', '2'], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith('step ')]
    assert len(lines) == 2 and all('Mesh Reg' in l for l in lines), r.stdout
