"""GPU tests of the triangle-mesh path (csrc/mesh.hip: vpn_mesh_raster_fwd/bwd, vpn_mesh_sample_fwd/bwd) against float64 per
pixel, per tile, per vertex and per draw, on the cases of tests/mesh_ref.py: faces whose inflated box ends a hair inside or
outside a tile, three different cameras in one batch, images taller than wide and smaller than a tile, face and vertex counts
around the 64-face pass and the 256-lane projection block, a face across the near plane, a 200-face fan, 40 coincident faces,
indices outside [0, P) in a batch of two, and for the sampler one to three chunks of the prefix-sum kernel with faces of no
area at the head, in the middle and at the tail, and draws at 0 and 1 - 2^-24.

Bars (mesh_ref.py): forward |alpha - alpha64| <= 2e-5 + n_culled(tile) 1.2e-7 per pixel; backward norm-wise 1e-4 with
test_mesh_path.py's widening, and element-wise per sample at most 4 times the fp32 oracle's own error (never below 1e-4).
The one-tile-at-a-time backward is held to the float64 union of the faces the tile keeps (mesh_ref.tile_reference says why).
Sampler: the face is the float64 statement's, or its neighbour across a prefix sum within 4 ulp32(total) of the target; the
draws that DIFFER are capped at 0.1 % of a case (draws that merely come that close are not: the planted rows sit on the
first and last prefix sum on purpose, and about 2 of 1000 uniform draws over 2049 faces do by chance).
Every figure is printed before it is asserted (run with -s); DESIGN.md 4.5 records the worst ones.

Measured on an MI355X (kernel [fp32 oracle], worst over the cases): alpha 8.1e-6 [8.7e-6], the worst pixel at 0.41 of its bar;
element-wise ratio kernel : oracle 3.85 (shape_40x56_F63_P3, 63 coincident faces under the oblique camera), 1.20 over the
border cases, 1.16 over the single tiles; run to run 1.8e-7; sampler: no face differs, points 8.0e-8, gradient 9.9e-7.
What these tests found, fixed in csrc/mesh.hip: with the camera and the projection in fp32 two samples under the camera
(1.6, -35, 250) were 6.18 and 4.44 times as far from float64 as the fp32 oracle (1.5e-4 against 1.6e-5, 1.7e-4 against
3.8e-5); both project kernels now work in fp64 and round once (0.30 and 1.14)."""
import pytest
import torch

import mesh_ref as M

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope='module')
def vpn():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU (no CPU fallback exists)')
    import vpn_amd
    vpn_amd._lib.lib()
    return vpn_amd


def _forward(c, verts=None, faces=None):
    from vpn_amd.ops import MeshRasterFunction, faces_i32
    v = (c.verts if verts is None else verts).to(DEV).requires_grad_(True)
    a = MeshRasterFunction.apply(v, faces_i32(c.faces if faces is None else faces, torch.device(DEV)), c.cam.to(DEV), c.H, c.W, c.sigma)
    return v, a


def _grad(c, Wt, **kw):
    v, a = _forward(c, **kw)
    (a * Wt.to(DEV)).sum().backward()
    return a.detach().cpu(), v.grad.cpu()


def _hold_grad(label, got, g32, g64):
    """The two backward bars; prints every figure first.  Returns the worst ratio kernel / oracle of the element-wise bar."""
    en_cpu, ee_cpu = M.grad_errors(g32, g64)
    en, ee = M.grad_errors(got, g64)
    ratio = max(e / max(ec, M.ELEM_FLOOR / M.ELEM_MARGIN) for e, ec in zip(ee, ee_cpu))
    msg = '%-28s norm-wise %.2e [%.2e]  element-wise %s  [%s]  ratio %.2f' % (
        label, en, en_cpu, ' '.join('%.1e' % e for e in ee), ' '.join('%.1e' % e for e in ee_cpu), ratio)
    print(msg)
    assert bool(torch.isfinite(got).all()), label
    assert en <= M.norm_bar(en_cpu), msg
    assert all(e <= M.elem_bar(ec) for e, ec in zip(ee, ee_cpu)), msg
    return ratio


# ------------------------------------------------------------------------------------------------ raster, whole image
@pytest.mark.parametrize('name', [c.name for c in M.raster_cases()])
def test_raster_per_pixel_and_per_vertex(vpn, name):
    c, r = M.case_by_name(name), M.raster_reference(name)
    a, g = _grad(c, r['Wt'])
    a64 = r[F64][0]
    d = (a.double() - a64).abs()
    bar = M.ALPHA_BAR + r['n_culled'].double() * M.CULL_A
    print('%-28s alpha %.2e [%.2e]  worst pixel at %.2f of its bar' % (name, float(d.max()), float((r[F32][0] - a64).abs().max()),
                                                                      float((d / bar).max())))
    assert bool(torch.isfinite(a).all()) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    assert bool((d <= bar).all()), (name, float(d.max()), torch.nonzero(d > bar)[:4].tolist())
    assert torch.equal(_forward(c)[1].detach().cpu(), a)                # two forward calls are bit-equal
    _hold_grad(name, g, r[F32][1], r[F64][1])


def test_stack_saturates_to_one(vpn):
    c, r = M.stack(), M.raster_reference(M.stack().name)
    a = _forward(c)[1].detach().cpu()
    sat = (1.0 - r[F64][0]) < 2.0 ** -25
    assert int(sat.sum()) > 100 and bool((a[sat] == 1.0).all())


@pytest.mark.parametrize('name', ['fan_200', 'stack_40'])
def test_backward_run_to_run(vpn, name):
    """The backward adds with atomics and is not bitwise reproducible: two calls agree within twice the norm-wise bar."""
    c, r = M.case_by_name(name), M.raster_reference(name)
    g1, g2 = _grad(c, r['Wt'])[1], _grad(c, r['Wt'])[1]
    e = M.rel_err(g1, g2)
    print('%-28s run to run %.2e' % (name, e))
    assert e <= 2 * M.norm_bar(M.rel_err(r[F32][1], r[F64][1]))


# ------------------------------------------------------------------------------------------------ raster, one tile at a time
@pytest.mark.parametrize('name', M.TILE_CASES)
def test_backward_per_tile(vpn, name):
    """Upstream weights on ONE tile at a time (one forward, 16 backward calls): both bars per tile, and exactly zero where
    the float64 gradient is exactly zero.  A (tile, face) pair dropped from the scatter, the early exit of a tile without
    upstream gradient taken wrongly, and another sample's camera in mesh_project_bwd_kernel all show here."""
    c, r = M.case_by_name(name), M.tile_reference(name)
    v, a = _forward(c)
    worst, zeros = 0.0, 0
    for t in range(r['tiles']):
        got = torch.autograd.grad((a * (r['Wt'] * (r['tile_of_pixel'] == t)).to(DEV)).sum(), v, retain_graph=True)[0].cpu()
        g32, g64 = r[F32][t], r[F64][t]
        for b in range(got.shape[0]):
            if float(g64[b].abs().max()) == 0.0:
                zeros += 1
                assert float(got[b].abs().max()) == 0.0, (name, t, b)
            else:
                worst = max(worst, _hold_grad('%s tile %d sample %d' % (name, t, b), got[b:b + 1], g32[b:b + 1], g64[b:b + 1]))
    print('%-28s worst ratio over the tiles %.2f, %d (tile, sample) pairs exactly zero' % (name, worst, zeros))
    assert zeros > 0 and zeros < r['tiles'] * got.shape[0]


# ------------------------------------------------------------------------------------------------ near plane, bad indices
def test_near_plane(vpn):
    c, r = M.near_plane(), M.raster_reference(M.near_plane().name)
    a, g = _grad(c, r['Wt'])
    drawn, dead, shared = (list(c.meta[k]) for k in ('drawn', 'dead', 'shared'))
    # the straddling face and the face behind the eye add nothing: the drawn faces alone give the same bits
    assert torch.equal(_forward(c, faces=c.faces[drawn])[1].detach().cpu(), a)
    assert float(g[0, dead].abs().max()) == 0.0
    # the shared vertices carry the drawn face's gradient alone (float64 of the drawn faces only), held at their own scale
    v64 = c.verts.double().requires_grad_(True)
    (M.O.mesh_raster(v64, c.faces[drawn], c.cam.double(), c.H, c.W, c.sigma) * r['Wt'].double()).sum().backward()
    assert M.rel_err(v64.grad, r[F64][1]) <= 1e-12
    _hold_grad('near_plane shared vertices', g[:, shared], r[F32][1][:, shared], v64.grad[:, shared])
    _hold_grad('near_plane vertices 3, 4, 5', g[:, 3:6], r[F32][1][:, 3:6], v64.grad[:, 3:6])


def test_bad_indices_stay_in_their_sample(vpn):
    """(Forward and backward against the clamped statement: test_raster_per_pixel_and_per_vertex[bad_indices].)  Sample 0
    does not change when sample 1's vertices do: forward bit for bit, backward within the run-to-run allowance."""
    c, r = M.bad_indices(), M.raster_reference(M.bad_indices().name)
    a, g = _grad(c, r['Wt'])
    other = c.verts.clone()
    other[1] = other[1].flip(0) * 1.3 + 0.05
    a2, g2 = _grad(c, r['Wt'], verts=other)
    e = M.rel_err(g2[0], g[0])
    print('bad_indices: sample 0 backward after sample 1 changed %.2e; sample 1 alpha moved by %.2e' % (e, float((a2[1] - a[1]).abs().max())))
    assert torch.equal(a2[0], a[0]) and float((a2[1] - a[1]).abs().max()) > 0.1
    assert e <= 2 * M.NORM_BAR


# ------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize('mode', ['explicit', 'philox'])
@pytest.mark.parametrize('name', [c.name for c in M.sampler_meshes()])
def test_sampler_per_draw_and_per_vertex(vpn, name, mode):
    from vpn_amd.ops import MeshSampleFunction, faces_i32
    c = next(x for x in M.sampler_meshes() if x.name == name)
    B, P = c.verts.shape[:2]
    F = c.faces.shape[0]
    f = M.clamp_faces(c.faces, P)
    vg = c.verts.to(DEV).requires_grad_(True)
    pts, idx = MeshSampleFunction.apply(vg, faces_i32(c.faces, torch.device(DEV)), c.n, c.u.to(DEV) if mode == 'explicit' else None,
                                        M.SAMPLE_SEED, M.SAMPLE_BASE)
    bary = pts.grad_fn.saved_tensors[2].cpu()
    g = torch.stack([M.sample_weights(c, b) for b in range(B)])
    (pts * g.to(DEV)).sum().backward()
    assert idx.dtype == torch.int32 and not idx.requires_grad and pts.shape == (B, c.n, 3)
    for b in range(B):
        u = M.sampler_uniforms(c, mode, b)
        v64 = c.verts[b].double()
        st = M.sample_statement(v64, f, u)
        got = idx[b].cpu().long()
        assert int(got.min()) >= 0 and int(got.max()) <= F - 1
        differ = got != st.face
        p64, w64 = M.bary_points(v64, f, got, u)                        # of the face the KERNEL chose: every draw is compared
        ep = float((pts[b].detach().cpu().double() - p64).abs().max())
        eb = float((bary[b].double().sum(1) - 1.0).abs().max())
        eg = M.elem_rel_err(vg.grad[b].cpu(), M.bary_scatter(P, f, got, w64, g[b]))
        print('%-16s %-8s b %d: differ %d (at %s ulp)  points %.2e  |sum bary - 1| %.2e  grad %.2e' %
              (name, mode, b, int(differ.sum()), ['%.2f' % x for x in st.dist[differ].tolist()], ep, eb, eg))
        assert bool(M.face_allowed(st, got).all()), (got[~M.face_allowed(st, got)][:8], st.face[~M.face_allowed(st, got)][:8])
        assert bool((st.dist[differ] <= M.SAMPLE_ULPS).all()) and int(differ.sum()) <= M.SAMPLE_CAP * c.n
        if name == 'all_degenerate':
            assert bool((got == F - 1).all())
        else:
            assert not bool(torch.isin(got, torch.tensor(c.meta['planted'], dtype=torch.long)).any())
        assert ep <= M.POINT_BAR and eb <= 2.0 ** -23 and eg <= M.SAMPLE_GRAD_BAR
