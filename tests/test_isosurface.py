"""GPU checks of the outer-surface extraction (csrc/isosurface.hip) at small shapes: the primitive field
against float64 and against the occupancy kernel, surface nets fed the GPU's own field against the fp32 restatement of
tests/isosurface_ref.py (counts, open edges, faces and padding exact, vertices bit for bit) and the float64 one (1e-6), the
cross-checks with the ragged sampler and the winding number, and SurfaceEvaluationMeter.update_surface / update_primitives."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import isosurface_ref as IR
import occupancy_ref as OR
import surfeval_ref as SR
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAMES5 = ['airplane', 'rifle', 'display', 'table', 'telephone']
FIXTURES = ['ellipsoid', 'cuboid', 'union3', 'two_apart']


# ---- the field

def _field_check(params, kinds, queries):
    from vpn_amd import ops
    got = ops.primitive_field(params.to(DEV), list(kinds), queries.to(DEV))
    want = IR.prim_field(params, kinds, queries)
    g = got.cpu().double()
    finite = torch.isfinite(want)
    assert torch.equal(torch.isfinite(g), finite) and not torch.isnan(g).any()
    err = float(((g - want).abs() / (1 + want.abs()))[finite].max())
    occ = ops.primitive_occupancy(params.to(DEV), list(kinds), queries.to(DEV))
    assert torch.equal((got <= 0).to(torch.uint8), occ)                           # every query, bit for bit
    return got, err


def test_field_against_float64_and_the_occupancy_kernel():
    from vpn_amd import ops
    c = OR.prim_case()                                                           # K = 3, B = 3, the 8^3 lattice plus 257 drawn queries
    got, err = _field_check(c['params'], c['kinds'], c['queries'])
    print('field, K = 3: worst |f32 - f64| / (1 + |f64|) = %.2e' % err)
    assert err <= 1e-4 and int((got <= 0).sum()) > 60
    # shared and per-sample queries: the same bits
    per = c['queries'][None].expand(3, -1, -1).contiguous().to(DEV)
    assert torch.equal(ops.primitive_field(c['params'].to(DEV), list(c['kinds']), per), got)
    # K = 300: two stagings of the pose records
    g = torch.Generator().manual_seed(11)
    params = torch.cat([0.05 + 0.2 * torch.rand(2, 300, 3, generator=g), torch.rand(2, 300, 4, generator=g) * 2 - 1,
                        0.8 * (torch.rand(2, 300, 3, generator=g) - 0.5)], 2).float()
    kinds = tuple(int(k) for k in torch.randint(0, 2, (300,), generator=g))
    queries = (torch.rand(2, 257, 3, generator=g) * 1.6 - 0.8).float()
    got, err = _field_check(params, kinds, queries)
    print('field, K = 300: worst |f32 - f64| / (1 + |f64|) = %.2e' % err)
    assert err <= 1e-4 and 0 < int((got <= 0).sum()) < got.numel()


def test_field_skips_nan_primitives_and_is_inf_when_none_is_left():
    from vpn_amd import ops
    c = OR.prim_case()
    params, q = c['params'].clone(), c['queries'][:64].clone()
    params[0, 0, 0] = float('nan')                                               # sample 0: the cuboid is skipped everywhere
    params[1, :, 7] = float('nan')                                               # sample 1: nothing is left
    q[5, 1] = float('nan')                                                       # a NaN query: nothing is left in any sample
    got = ops.primitive_field(params.to(DEV), list(c['kinds']), q.to(DEV)).cpu()
    want = IR.prim_field(params, c['kinds'], q)
    assert not torch.isnan(got).any() and torch.equal(torch.isinf(got), torch.isinf(want))
    assert bool(torch.isinf(got[1]).all()) and bool((got[1] > 0).all()) and bool(torch.isinf(got[:, 5]).all())
    two = IR.prim_field(c['params'][:1, 1:], c['kinds'][1:], q)                  # sample 0 without its cuboid
    ok = torch.isfinite(two[0])
    assert float(((got[0].double() - two[0]).abs() / (1 + two[0].abs()))[ok].max()) <= 1e-4 and int(ok.sum()) == 63
    occ = ops.primitive_occupancy(params.to(DEV), list(c['kinds']), q.to(DEV)).cpu()
    assert torch.equal((got <= 0).to(torch.uint8), occ)


# ---- surface nets

def _compare(field, coords, level=0.0, max_verts=None, max_faces=None, f64=True):
    """field [B,Nz,Ny,Nx] fp32 on the host (what the kernels read): the extraction against the fp32 restatement, exactly, and
    against the float64 one.  Returns (IsoSurface, [restatement per sample], worst distance to float64)."""
    from vpn_amd import ops
    field = torch.as_tensor(field)
    dev_coords = tuple(torch.as_tensor(c).to(DEV) for c in coords)
    surface = ops.isosurface(field.to(DEV), dev_coords, level, max_verts, max_faces)
    verts, faces, counts = surface.verts.cpu().numpy(), surface.faces.cpu().numpy(), surface.counts.cpu().numpy()
    worst, refs = 0.0, []
    for b in range(field.shape[0]):
        ref = IR.surface_nets(field[b].numpy(), coords, level, np.float32)
        want_v, want_f, want_c = IR.padded(ref, verts.shape[1], faces.shape[1])
        assert counts[b].tolist() == want_c.tolist(), (b, counts[b].tolist(), want_c.tolist())
        assert np.array_equal(faces[b], want_f)
        assert np.array_equal(verts[b].view(np.int32), want_v.view(np.int32))     # bit for bit, padding included
        if f64 and not want_c[3] and want_c[0]:
            hi = IR.surface_nets(field[b].numpy(), coords, level, np.float64)
            worst = max(worst, float(np.abs(verts[b][:want_c[0]].astype(np.float64) - hi['verts']).max()))
        refs.append(ref)
    assert worst <= 1e-6
    return surface, refs, worst


def _gpu_field(name, dims, lo=-0.5, hi=0.5):
    """The GPU's own field of a case on a lattice: (field fp32 [1,Nz,Ny,Nx] on the host, (cx, cy, cz) numpy)."""
    from vpn_amd import ops
    cx, cy, cz, q = ops.lattice(dims, lo, hi)
    params, kinds = IR.case_params(name)
    f = ops.primitive_field(params.to(DEV), list(kinds), q.to(DEV)).cpu()
    return f.view(1, cz.numel(), cy.numel(), cx.numel()), (cx.numpy(), cy.numpy(), cz.numpy())


def test_hand_field_on_a_5_4_3_lattice():
    field, coords = IR.hand_field()
    surface, refs, worst = _compare(field[None], coords)
    assert surface.counts.cpu().tolist() == [[22, 40, 0, 0]] and surface.dims == (5, 4, 3)
    assert surface.verts.shape == (1, 8 * 25, 3) and surface.faces.shape == (1, 16 * 25, 3)      # the default capacities
    _compare(field[None], coords, level=1.25)


@pytest.mark.parametrize('name', FIXTURES)
def test_fixtures_at_12_cubed(name):
    """1331 cells: six workgroups, the last one partial."""
    field, coords = _gpu_field(name, 12)
    surface, refs, worst = _compare(field, coords)
    print('%s at 12^3: %s, worst distance to float64 %.2e' % (name, surface.counts.cpu().tolist()[0], worst))
    assert refs[0]['n_open'] == 0 and refs[0]['faces'].shape[0] > 100 and IR.unmatched_edges(surface.faces.cpu().numpy()[0]).shape[0] == 0


def test_batch_with_an_empty_and_an_all_inside_sample():
    a, coords = _gpu_field('union3', 12)
    b, _ = _gpu_field('two_apart', 12)
    field = torch.cat([a, torch.full_like(a, 0.5), b, torch.full_like(a, -0.5)])
    surface, refs, _ = _compare(field, coords)
    counts = surface.counts.cpu().tolist()
    assert counts[1] == [0, 0, 0, 0] and counts[3] == [0, 0, 0, 0] and counts[0][0] != counts[2][0] and min(counts[0][1], counts[2][1]) > 0
    assert not surface.verts[1].any() and not surface.faces[3].any()


def test_more_workgroups_than_one_scan_chunk():
    """42^3 nodes: 68921 cells in 270 workgroups, so a work-item of the scan owns two rows."""
    a, coords = _gpu_field('ellipsoid', 42)
    b, _ = _gpu_field('union3', 42)
    surface, refs, worst = _compare(torch.cat([a, b]), coords)
    print('42^3: %s, worst distance to float64 %.2e' % (surface.counts.cpu().tolist(), worst))
    assert all(r['n_open'] == 0 for r in refs) and refs[0]['verts'].shape[0] > 2000


def test_unequal_dimensions_and_a_level():
    field, coords = _gpu_field('union3', (13, 9, 11), (-0.5, -0.4, -0.45), (0.5, 0.4, 0.45))
    surface, refs, _ = _compare(field, coords)
    assert surface.dims == (13, 9, 11) and refs[0]['faces'].shape[0] > 50
    from vpn_amd import Meshing
    params, kinds = IR.case_params('union3')                                     # the same through union_meshes, bounds per axis
    union = Meshing.union_meshes(params.to(DEV), list(kinds), resolution=(13, 9, 11), bounds=((-0.5, -0.4, -0.45), (0.5, 0.4, 0.45)))
    assert torch.equal(union.verts, surface.verts) and torch.equal(union.faces, surface.faces) and torch.equal(union.counts, surface.counts)
    field, coords = _gpu_field('ellipsoid', 12)
    counts = [_compare(field, coords, level=level)[0].counts.cpu().tolist()[0] for level in (-0.3, 0.0, 0.25)]
    assert counts[0][0] < counts[1][0] < counts[2][0] and all(c[2] == 0 and c[3] == 0 for c in counts)


def test_nan_and_inf_nodes():
    field, coords = _gpu_field('union3', 12)
    f = field.clone()
    inside = np.argwhere(f[0].numpy() < -0.5)
    assert len(inside) >= 2
    # a -inf node deep inside, NaN and +inf nodes outside: every neighbour of a clamped node is finite, where the fp32 and the
    # float64 statement agree
    f[0][tuple(inside[0])] = -float('inf')
    f[0, 1, 1, 1], f[0, 10, 2, 3], f[0, 2, 9, 9] = float('nan'), float('inf'), float('nan')
    f[0, 5, 5, 0] = float('nan')
    surface, refs, _ = _compare(f, coords)
    base = IR.surface_nets(field[0].numpy(), coords, 0.0, np.float32)
    assert np.array_equal(refs[0]['faces'], base['faces'])                        # outside stays outside, inside stays inside
    # neighbours clamped to opposite ends: s_a - s_b overflows in fp32 and t = 0; the fp32 statement alone is compared
    g = field.clone()
    g[0, 6, 6, 6], g[0, 6, 6, 7], g[0, 6, 7, 6] = -float('inf'), float('nan'), float('inf')
    g[0, 0, 0, 0] = -float('inf')                                                # a corner of the lattice: open edges
    surface, refs, _ = _compare(g, coords, f64=False)
    assert refs[0]['n_open'] == 3 and refs[0]['t_min'] == 0.0


def test_capacity_exactly_the_count_and_one_below():
    a, coords = _gpu_field('ellipsoid', 12)
    b, _ = _gpu_field('two_apart', 12)
    field = torch.cat([a, b])
    ref =[IR.surface_nets(field[k].numpy(), coords, 0.0, np.float32) for k in (0, 1)]
    nv, nf = [r['verts'].shape[0] for r in ref], [r['faces'].shape[0] for r in ref]
    assert nv[0] > nv[1] and nf[0] > nf[1]
    exact, _, _ = _compare(field, coords, max_verts=nv[0], max_faces=nf[0])
    assert exact.counts.cpu().tolist() == [[nv[0], nf[0], 0, 0], [nv[1], nf[1], 0, 0]]
    for cap in ((nv[0] - 1, nf[0]), (nv[0], nf[0] - 1)):
        short, _, _ = _compare(field, coords, max_verts=cap[0], max_faces=cap[1])
        assert short.counts.cpu().tolist() == [[nv[0], nf[0], 0, 1], [nv[1], nf[1], 0, 0]]      # the true counts; sample 1 fits
        assert not short.verts[0].any() and not short.faces[0].any() and short.faces[1].any()


def test_two_runs_are_bit_equal():
    from vpn_amd import Meshing
    params, kinds = IR.case_params('assembly35')
    p = torch.cat([params, IR.case_params('assembly15')[0]]).to(DEV)
    one, two = Meshing.union_meshes(p, list(kinds), resolution=24), Meshing.union_meshes(p, list(kinds), resolution=24)
    assert torch.equal(one.verts, two.verts) and torch.equal(one.faces, two.faces) and torch.equal(one.counts, two.counts)
    assert int(one.counts[:, 1].min()) > 0 and not one.counts[:, 3].any()


# ---- cross-checks with what exists

def test_winding_number_of_the_padded_layout_equals_the_inside_flags():
    from vpn_amd import ops
    field, coords = _gpu_field('union3', 16)
    surface, refs, _ = _compare(field, coords)
    nodes = ops.lattice(16, device=DEV)[3]
    w = ops.ragged_winding_number(surface.arrays(), nodes).cpu()
    assert float((w - w.round()).abs().max()) <= 1e-3
    assert np.array_equal((w[0] > 0.5).numpy(), refs[0]['inside'].ravel())
    assert torch.equal(ops.mesh_occupancy(surface.arrays(), None, nodes).cpu()[0].bool(), w[0] > 0.5)
    assert torch.equal(ops.ragged_winding_number(surface.to_mesh_batch(), nodes).cpu() > 0.5, w > 0.5)


def test_ragged_sampler_never_draws_a_padding_face():
    from vpn_amd import ops
    fields = [_gpu_field(name, 12) for name in FIXTURES]
    surface, refs, _ = _compare(torch.cat([f for f, _ in fields]), fields[0][1])
    a = surface.arrays()
    points, fidx, bary = ops.ragged_sample(*a, 4096, seed=7, return_faces=True)
    counts = surface.counts.cpu()
    assert fidx.shape == (4, 1, 4096) and int(fidx.min()) >= 0
    assert bool((fidx[:, 0].cpu() < counts[:, 1:2]).all())
    # a drawn point lies on its face: within the box of the mesh's real vertices
    for b in range(4):
        v = surface.verts[b, :int(counts[b, 0])]
        assert bool((points[b, 0] >= v.min(0).values - 1e-6).all()) and bool((points[b, 0] <= v.max(0).values + 1e-6).all())
    normals = ops.ragged_face_normals(a.verts, a.faces, a.vert_offset, a.face_offset, fidx)
    assert float((normals.norm(dim=-1) - 1).abs().max()) <= 1e-5                # a padding face would give (0,0,0)


def test_signed_distance_remeshes_two_overlapping_icospheres_as_one_solid():
    from vpn_amd import ops
    v, f = SR.icosphere(2)
    verts = torch.cat([v * 0.25 - torch.tensor([0.1, 0.0, 0.0]), v * 0.22 + torch.tensor([0.12, 0.03, 0.0])]).float()[None].to(DEV)
    faces = torch.cat([f, f + v.shape[0]]).to(DEV)
    cx, cy, cz, nodes = ops.lattice(16, device=DEV)
    w_in = ops.winding_number(verts, faces, nodes)[0].cpu()
    assert int((w_in > 1.5).sum()) > 5                                           # the input counts the overlap twice
    sd = ops.mesh_signed_distance(verts, faces, nodes)
    assert sd.shape == (1, 4096) and torch.equal(sd[0].cpu() < 0, w_in > 0.5)
    surface = ops.isosurface(sd.view(1, 16, 16, 16), (cx, cy, cz))
    counts = surface.counts.cpu().tolist()[0]
    assert counts[1] > 100 and counts[2] == 0 and counts[3] == 0
    w_out = ops.ragged_winding_number(surface.arrays(), nodes)[0].cpu()
    assert float((w_out - w_out.round()).abs().max()) <= 1e-3 and set(w_out.round().int().tolist()) == {0, 1}
    assert torch.equal(w_out > 0.5, w_in > 0.5)                                  # the same solid, its interior faces gone
    per_sample = ops.mesh_signed_distance(verts, faces, nodes[None].contiguous())
    assert torch.equal(per_sample, sd)


# ---- the meter

def _meter_inputs():
    """Three batches of (params [3,K,10], gt points [3,300,3], gt normals, class indices) on the device; K = 16 assemblies and,
    in batch 1, a sample whose primitives lie outside the lattice (an empty surface)."""
    g = torch.Generator().manual_seed(21)
    base = torch.cat([IR.case_params('assembly35')[0], IR.case_params('assembly15')[0]])
    kinds = IR.case_params('assembly35')[1]
    out = []
    for k in range(3):
        params = torch.cat([base, base[:1]]).clone()
        params[:, :, 7:10] += 0.01 * k
        if k == 1:
            params[2, :, 7:10] += 5.0
        gt = (torch.rand(3, 300, 3, generator=g) - 0.5) * 0.8
        idx = torch.tensor([(2 * k + b) % 5 for b in range(3)], dtype=torch.int32, device=DEV)
        out.append((params.to(DEV), gt.to(DEV), torch.nn.functional.normalize(gt, dim=-1).to(DEV), idx))
    return list(kinds), out


def test_update_primitives_is_its_steps_and_counts_unusable_samples_as_invalid():
    from vpn_amd import Meshing, SurfaceEvaluationMeter, ops
    kinds, batches = _meter_inputs()
    a, b, c = (SurfaceEvaluationMeter(NAMES5, DEV) for _ in range(3))
    for k, (params, gt, gtn, idx) in enumerate(batches):
        rows_a = a.update_primitives(params, kinds, gt, idx, resolution=16, n=256, seed=40 + k, mesh_base=3, gt_normals=gtn)
        surface = Meshing.union_meshes(params, kinds, resolution=16)
        rows_b = b.update_surface(surface, gt, idx, n=256, seed=40 + k, mesh_base=3, gt_normals=gtn)
        # and by hand: lattice -> field -> isosurface -> ragged sampler -> normals -> update
        cx, cy, cz, q = ops.lattice(16, device=DEV)
        s2 = ops.isosurface(ops.primitive_field(params, kinds, q).view(3, 16, 16, 16), (cx, cy, cz))
        assert torch.equal(s2.verts, surface.verts) and torch.equal(s2.faces, surface.faces) and torch.equal(s2.counts, surface.counts)
        arr = s2.arrays()
        points, fidx, _ = ops.ragged_sample(*arr, 256, seed=40 + k, mesh_base=3, return_faces=True)
        normals = ops.ragged_face_normals(arr.verts, arr.faces, arr.vert_offset, arr.face_offset, fidx)[:, 0].contiguous()
        unusable = (s2.counts[:, 1] == 0) | (s2.counts[:, 3] != 0)
        rows_c = c.update(points[:, 0].contiguous(), gt, torch.where(unusable, torch.full_like(idx, -1), idx), normals, gtn)
        assert torch.equal(rows_a, rows_b) and torch.equal(rows_a, rows_c)
        assert unusable.cpu().tolist() == [False, False, k == 1]
    assert torch.equal(a.state, b.state) and torch.equal(a.state, c.state)
    res = a.result()
    assert res['n_samples'] == 9 and res['n_batches'] == 3 and res['n_invalid'] == 1 and sum(res['class_n']) == 8
    assert res['normal_consistency'] is not None and 0 < res['cd'] < 1
    # an overflowing sample: capacities between the two assemblies' counts
    params, gt, gtn, idx = batches[0]
    counts = Meshing.union_meshes(params, kinds, resolution=16).counts.cpu()
    assert int(counts[0, 1]) != int(counts[1, 1])
    cap = (int(counts[:2, 1].min()) + int(counts[:2, 1].max())) // 2
    over = SurfaceEvaluationMeter(NAMES5, DEV)
    over.update_primitives(params, kinds, gt, idx, resolution=16, n=64, seed=1, max_faces=cap)
    big = int(counts[:, 1].argmax())
    res = over.result()
    want_invalid = int((counts[:, 1] > cap).sum())
    assert res['n_invalid'] == want_invalid >= 1 and sum(res['class_n']) == 3 - want_invalid and res['class_n'][int(idx[big])] == 0


def test_determinism_no_host_sync_and_graph_replay():
    from vpn_amd import SurfaceEvaluationMeter, ops
    kinds, batches = _meter_inputs()
    kt = ops.kinds_tensor(kinds, DEV)

    def run(meter, items):
        return [meter.update_primitives(p, kt, gt, idx, resolution=16, n=256, seed=9, gt_normals=gtn).clone() for p, gt, gtn, idx in items]

    one, two = SurfaceEvaluationMeter(NAMES5, DEV), SurfaceEvaluationMeter(NAMES5, DEV)
    rows_1 = run(one, batches)                                                   # also the warm-up of every code object and table
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        rows_2 = run(two, batches)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(rows_1, rows_2)) and torch.equal(one.state, two.state)
    # one capture, three replays against three eager updates
    meter = SurfaceEvaluationMeter(NAMES5, DEV)
    sp, sgt, sgtn, sidx = (t.clone() for t in batches[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(meter, [(sp, sgt, sgtn, sidx)])                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    meter.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rows = run(meter, [(sp, sgt, sgtn, sidx)])
    assert meter.result()['n_batches'] == 0                                      # capturing ran nothing
    for k, (p, gt, gtn, idx) in enumerate(batches):
        sp.copy_(p)
        sgt.copy_(gt)
        sgtn.copy_(gtn)
        sidx.copy_(idx)
        graph.replay()
        assert torch.equal(rows[0], rows_1[k])
    torch.cuda.synchronize()
    assert torch.equal(meter.state, one.state) and meter.result()['n_invalid'] == 1


def test_update_and_update_mesh_are_untouched_by_a_surface_update():
    from vpn_amd import SurfaceEvaluationMeter
    p, q = [t.to(DEV) for t in SR.clouds('clustered')]
    verts, faces = OR.ellipsoids(1, 3).to(DEV), SR.icosphere(1)[1].int().to(DEV)
    ref, meter = SurfaceEvaluationMeter(NAMES5, DEV), SurfaceEvaluationMeter(NAMES5, DEV)
    want = [ref.update(p, q, [0, 1, 2]).clone(), ref.update_mesh(verts, faces, q, [0, 1, 2], n=128, seed=5).clone()]
    kinds, batches = _meter_inputs()
    params, gt, gtn, idx = batches[0]
    got = [meter.update(p, q, [0, 1, 2]).clone()]
    state = meter.state.clone()
    other = SurfaceEvaluationMeter(NAMES5, DEV)
    other.update_primitives(params, kinds, gt, idx, resolution=12, n=64, seed=2)
    assert torch.equal(meter.state, state)
    got.append(meter.update_mesh(verts, faces, q, [0, 1, 2], n=128, seed=5).clone())
    assert all(torch.equal(x, y) for x, y in zip(got, want)) and torch.equal(meter.state, ref.state)


@pytest.mark.parametrize('flags', [[], ['--gcn']])
def test_eval_step_example_scores_the_outer_surface(flags, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'eval_step.py'), '--batches', '2', '--epoch', '3', '--surface',
                        '--outer', '--outer-resolution', '16', '--dump', str(tmp_path)] + flags,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if 'surface cd = ' in l]
    assert lines and lines[-1].startswith('total'), r.stdout
    assert float(lines[-1].split('surface cd = ')[1].split(',')[0]) > 0.0
    text = (tmp_path / 'union_000.obj').read_text().splitlines()              # sample 0's union mesh
    n_verts, faces = sum(l.startswith('v ') for l in text), [l.split()[1:] for l in text if l.startswith('f ')]
    assert n_verts > 0 and faces and all(1 <= int(i) <= n_verts for f in faces for i in f)
