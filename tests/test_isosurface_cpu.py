"""CPU checks of the outer-surface extraction (ops.primitive_field, ops.lattice, ops.isosurface, ops.IsoSurface,
ops.mesh_signed_distance, Meshing.union_meshes, SurfaceEvaluationMeter.update_surface; csrc/isosurface.hip):
the restatement of tests/isosurface_ref.py against plain loops, the properties of a closed oriented mesh on the fixtures and
on two K = 16 assemblies in float64, the known inward bias, the argument contract of the Python layer and of the C entries,
and the kernels' resources."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import isosurface_ref as IR
from kernel_resources import kernel_resources

CLOSED = ['ellipsoid', 'cuboid', 'union3', 'two_apart', 'assembly35', 'assembly15']


def _extract(name, N, dtype=np.float64):
    field, coords = IR.case_field(name, N)
    return IR.surface_nets(field.astype(np.float32), coords, 0.0, dtype)


# ---- the restatement against plain loops

def test_restatement_equals_plain_loops_on_the_hand_field():
    field, coords = IR.hand_field()
    for level in (0.0, 1.25):
        got = IR.surface_nets(field, coords, level)
        verts, faces, n_open = IR.surface_nets_plain(field, coords, level)
        assert got['verts'].shape == (len(verts), 3) and got['faces'].tolist() == faces and got['n_open'] == n_open
        assert float(np.abs(got['verts'] - np.array(verts)).max()) <= 1e-15
        low = IR.surface_nets(field, coords, level, np.float32)
        assert low['verts'].dtype == np.float32 and low['faces'].tolist() == faces and low['n_open'] == n_open
        assert float(np.abs(low['verts'].astype(np.float64) - got['verts']).max()) <= 1e-6
    got = IR.surface_nets(field, coords, 0.0)
    assert got['verts'].shape[0] == 22 and got['faces'].shape[0] == 40 and got['n_open'] == 0
    assert bool(got['inside'][1, 2, 3]) and got['t_min'] == 0.0                  # the node that is inside by exactly 0
    assert IR.unmatched_edges(got['faces']).shape[0] == 0
    # the level moves nodes across: at 1.25 the solid reaches the lattice boundary
    assert IR.surface_nets(field, coords, 1.25)['n_open'] > 0


def test_padded_layout_and_overflow_of_the_restatement():
    field, coords = IR.hand_field()
    got = IR.surface_nets(field, coords, 0.0, np.float32)
    v, f, c = IR.padded(got, 30, 50)
    assert c.tolist() == [22, 40, 0, 0] and not v[22:].any() and not f[40:].any() and np.array_equal(f[:40], got['faces'])
    for cap in ((21, 50), (30, 39)):
        v, f, c = IR.padded(got, *cap)
        assert c.tolist() == [22, 40, 0, 1] and not v.any() and not f.any()
    assert IR.padded(got, 22, 40)[2].tolist() == [22, 40, 0, 0]


# ---- closed, oriented, and the solid it bounds

@pytest.mark.parametrize('N', [12, 16])
@pytest.mark.parametrize('name', CLOSED)
def test_extracted_mesh_is_closed_oriented_and_bounds_the_inside_nodes(name, N):
    """In float64.  The Euler characteristic of the mesh (vertices - undirected edges + faces, components over the mesh's
    edges) is 2 per component for all six cases (4 for two_apart).  The K = 16 assemblies are the first seed-1234 draws that
    isosurface_ref.assembly's rule admits: a rule on the inside flags of the lattice, not on a mesh.  The lattice's own count
    (one vertex per mixed cell, one edge per mixed lattice face plus one diagonal per quad, two triangles per quad) must give
    the same two numbers as the mesh."""
    r = _extract(name, N)
    verts, faces, inside = r['verts'], r['faces'], r['inside']
    assert r['n_open'] == 0
    assert IR.unmatched_edges(faces).shape[0] == 0
    assert 0.0 <= r['t_min'] and r['t_max'] <= 1.0
    assert faces.min() >= 0 and faces.max() < verts.shape[0] and len(np.unique(faces)) == verts.shape[0]
    chi, components = IR.euler_and_components(verts.shape[0], faces)
    print('%s N %d: %d vertices, %d faces, Euler characteristic %d over %d components, t in [%.4f, %.4f]'
          % (name, N, verts.shape[0], faces.shape[0], chi, components, r['t_min'], r['t_max']))
    assert chi == 2 * components
    if name in IR.COMPONENTS:
        assert components == IR.COMPONENTS[name]
    assert (chi, components) == IR.lattice_topology(inside)
    # the winding number of the mesh at EVERY lattice node: an integer, and 1 exactly at the inside nodes
    w = IR.winding_at(verts, faces, IR.lattice(N)[3])
    assert float(np.abs(w - np.round(w)).max()) <= 1e-9
    assert np.array_equal(w > 0.5, inside.ravel())
    assert IR.mesh_volume(verts, faces) > 0


def test_a_solid_that_crosses_the_lattice_boundary_leaves_open_edges_there():
    for N in (12, 16):
        r = _extract('crossing', N)
        assert r['n_open'] > 0
        bad = IR.unmatched_edges(r['faces'])
        assert bad.shape[0] > 0
        # the cell of every vertex on an unmatched edge touches a boundary face of the lattice
        cell_of_vertex = np.nonzero(r['cell_vertex'] >= 0)[0]
        nc = N - 1
        cells = cell_of_vertex[np.unique(bad)]
        cx, cy, cz = cells % nc, (cells // nc) % nc, cells // (nc * nc)
        on_boundary = (cx == 0) | (cx == nc - 1) | (cy == 0) | (cy == nc - 1) | (cz == 0) | (cz == nc - 1)
        assert bool(on_boundary.all())


def test_surface_nets_pull_the_ellipsoid_inwards_at_second_order():
    """The share of 4/3 pi a b c the mesh keeps: 87.1 %, 92.6 %, 98.2 % at N = 12, 16, 32."""
    kept = {N: IR.mesh_volume(*[_extract('ellipsoid', N)[k] for k in ('verts', 'faces')]) / IR.ELLIPSOID_VOLUME for N in (12, 16, 32)}
    print('ellipsoid volume kept: ' + ', '.join('N = %d: %.1f %%' % (N, 100 * v) for N, v in kept.items()))
    assert all(v < 1.0 for v in kept.values())
    assert 1 - kept[32] < 1 - kept[16] < 1 - kept[12]
    assert (1 - kept[32]) <= 0.3 * (1 - kept[16])                               # halving the step quarters the deficit, with some slack


def test_fp32_restatement_stays_within_1e6_of_float64_on_every_case():
    worst = 0.0
    for name in CLOSED:
        for N in (12, 16):
            a, b = _extract(name, N, np.float32), _extract(name, N)
            assert np.array_equal(a['faces'], b['faces']) and a['n_open'] == b['n_open']
            worst = max(worst, float(np.abs(a['verts'].astype(np.float64) - b['verts']).max()))
    print('fp32 restatement against float64: %.2e' % worst)
    assert worst <= 1e-6


def test_field_restatement_is_the_occupancy_restatement():
    import occupancy_ref as OR
    c = OR.prim_case()
    f = IR.prim_field(c['params'], c['kinds'], c['queries'])
    occ, _ = OR.prim_occupancy(c['params'], c['kinds'], c['queries'])
    assert torch.equal(f <= 0, occ.bool())
    bad = c['params'].clone()
    bad[0, :, 0] = 0.0                                                           # 0 / 0 at x = t: every m a NaN there
    q = torch.cat([bad[0, 0, 7:10][None], c['queries'][:3]])
    f = IR.prim_field(bad, c['kinds'], q)
    assert f[0, 0] == math.inf and not torch.isnan(f).any()


# ---- the Python layer

def test_lattice_is_grid_queries_and_takes_unequal_dimensions():
    from vpn_amd import ops
    for R, lo, hi in ((4, -0.5, 0.5), (5, -0.3, 0.7), (16, -0.5, 0.5)):
        cx, cy, cz, q = ops.lattice(R, lo, hi)
        assert torch.equal(q, ops.grid_queries(R, lo, hi)) and torch.equal(cx, cy) and torch.equal(cy, cz)
        assert torch.equal(cx, torch.from_numpy(IR.lattice(R, lo, hi)[0]))
    cx, cy, cz, q = ops.lattice((5, 4, 3), (-0.5, 0.0, -1.0), (0.5, 2.0, 1.0))
    want = IR.lattice((5, 4, 3), (-0.5, 0.0, -1.0), (0.5, 2.0, 1.0))
    assert (cx.numel(), cy.numel(), cz.numel()) == (5, 4, 3) and q.shape == (60, 3) and q.dtype == torch.float32
    assert all(torch.equal(a, torch.from_numpy(b)) for a, b in zip((cx, cy, cz, q), want))
    assert q[1].tolist() == [cx[1].item(), cy[0].item(), cz[0].item()] and q[5].tolist() == [cx[0].item(), cy[1].item(), cz[0].item()]
    for bad in ((1, -0.5, 0.5), ((4, 4), -0.5, 0.5), (300, -0.5, 0.5), (4, 0.5, 0.5), (4, 0.0, float('inf')), ((4, 1, 4), 0.0, 1.0)):
        with pytest.raises(ValueError):
            ops.lattice(*bad)


def test_ops_contract_is_checked_before_any_launch():
    import vpn_amd
    from vpn_amd import Meshing, SurfaceEvaluationMeter, ops
    prm, kinds, q = torch.zeros(2, 3, 10), [1, 0, 0], torch.zeros(5, 3)
    with pytest.raises(ValueError, match=r'primitive_field: params must be float32 \[B,K,10\]'):
        ops.primitive_field(prm[0], kinds, q)
    with pytest.raises(ValueError, match='primitive_field: 2 kinds for 3 primitives'):
        ops.primitive_field(prm, kinds[:2], q)
    with pytest.raises(ValueError, match=r'primitive_field: queries must be float32 \[Q,3\] or \[B,Q,3\]'):
        ops.primitive_field(prm, kinds, q.double())
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.primitive_field(prm, kinds, q)
    field, coords = torch.zeros(2, 3, 4, 5), (torch.zeros(5), torch.zeros(4), torch.zeros(3))
    with pytest.raises(ValueError, match=r'field must be float32 \[B,Nz,Ny,Nx\]'):
        ops.isosurface(field[0], coords)
    with pytest.raises(ValueError, match=r'field must be float32 \[B,Nz,Ny,Nx\]'):
        ops.isosurface(field.double(), coords)
    with pytest.raises(ValueError, match='at least 2'):
        ops.isosurface(field[:, :1], (coords[0], coords[1], coords[2][:1]))
    with pytest.raises(ValueError, match='coords must be'):
        ops.isosurface(field, coords[:2])
    with pytest.raises(ValueError, match=r'cy must be float32 \[4\]'):
        ops.isosurface(field, (coords[0], coords[0], coords[2]))
    with pytest.raises(ValueError, match=r'cz must be float32 \[3\]'):
        ops.isosurface(field, (coords[0], coords[1], coords[2].double()))
    with pytest.raises(ValueError, match='level must be finite'):
        ops.isosurface(field, coords, level=float('nan'))
    with pytest.raises(ValueError, match='capacities must be'):
        ops.isosurface(field, coords, max_verts=0)
    with pytest.raises(ValueError, match='capacities must be'):
        ops.isosurface(field, coords, max_faces=(1 << 24) + 1)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.isosurface(field, coords)
    with pytest.raises(RuntimeError, match='GPU only'):
        Meshing.union_meshes(prm, kinds, resolution=4)
    with pytest.raises(ValueError, match=r'params \[B,K,10\] expected'):
        Meshing.union_meshes(prm[0], kinds)
    with pytest.raises(ValueError, match=r'bounds must be \(lo, hi\)'):
        Meshing.union_meshes(prm, kinds, resolution=4, bounds=0.5)
    with pytest.raises(ValueError, match='lo must be one number or three'):
        Meshing.union_meshes(prm, kinds, resolution=4, bounds=((-0.5, -0.5), 0.5))
    with pytest.raises(RuntimeError, match='GPU only'):                           # one number or one per axis, as ops.lattice
        Meshing.union_meshes(prm, kinds, resolution=(5, 4, 3), bounds=((-0.5, -0.4, -0.3), (0.5, 0.4, 0.3)))
    v, f = torch.zeros(2, 4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(ValueError, match=r'verts must be float32 \[B,P,3\]'):
        ops.mesh_signed_distance(v[0], f, q)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.mesh_signed_distance(v, f, q)
    meter = SurfaceEvaluationMeter(['a', 'b'], 'cpu')
    with pytest.raises(TypeError, match='IsoSurface'):
        meter.update_surface(v, torch.zeros(2, 8, 3), [0, 1], seed=1)
    host = ops.IsoSurface(torch.zeros(2, 6, 3), torch.zeros(2, 8, 3, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), (3, 3, 3))
    with pytest.raises(RuntimeError, match='GPU only'):
        meter.update_surface(host, torch.zeros(2, 8, 3), [0, 1], seed=1)
    with pytest.raises(RuntimeError, match='GPU only'):
        meter.update_primitives(prm, kinds, torch.zeros(2, 8, 3), [0, 1], resolution=4, seed=1)
    assert not meter.state.any()
    for name in ('primitive_field', 'lattice', 'isosurface', 'IsoSurface', 'mesh_signed_distance'):
        assert getattr(vpn_amd, name) is getattr(ops, name), name


def test_padded_arrays_and_trimmed_meshes_of_an_isosurface_on_the_host():
    """The tables of arrays() follow from the capacities alone; meshes() and to_mesh_batch() trim by the counts."""
    from vpn_amd import MeshBatch, ops
    from vpn_amd.modules.dataset import chunk_table
    B, max_verts, max_faces = 3, 7, 600
    verts = torch.arange(B * max_verts * 3, dtype=torch.float32).reshape(B, max_verts, 3)
    faces = torch.zeros(B, max_faces, 3, dtype=torch.int32)
    faces[0, :2] = torch.tensor([[0, 1, 2], [0, 2, 3]])
    faces[2, :1] = torch.tensor([[4, 5, 6]])
    counts = torch.tensor([[4, 2, 0, 0], [9, 700, 0, 1], [7, 1, 3, 0]], dtype=torch.int32)
    s = ops.IsoSurface(verts, faces, counts, (5, 4, 3))
    a = s.arrays()
    assert len(s) == 3 and isinstance(a, ops.PaddedMeshArrays) and len(a) == 6
    assert a.verts.shape == (B * max_verts, 3) and a.faces.shape == (B * max_faces, 3) and a.verts.data_ptr() == verts.data_ptr()
    assert a.vert_offset.tolist() == [0, 7, 14, 21] and a.face_offset.tolist() == [0, 600, 1200, 1800]
    rows, offset = chunk_table([max_faces] * B)
    assert a.chunks.tolist() == [list(r) for r in rows] and a.chunk_offset.tolist() == offset
    assert all(t.dtype == torch.int32 for t in a[2:]) and a.face_counts == [600] * 3 and a.vert_counts == [7] * 3 and a.num_meshes == 3
    assert s.arrays().chunks is a.chunks                                         # cached per shape
    meshes = s.meshes()
    assert [m.vertices.shape[0] for m in meshes] == [4, 0, 7] and [m.faces.shape[0] for m in meshes] == [2, 0, 1]
    assert meshes[2].faces.tolist() == [[4, 5, 6]] and meshes[2].faces.dtype == torch.int64
    assert torch.equal(meshes[0].vertices, verts[0, :4])
    with pytest.raises(ValueError, match='mesh 1 has no vertices'):
        s.to_mesh_batch()
    ok = ops.IsoSurface(verts[[0, 2]], faces[[0, 2]], counts[[0, 2]], (5, 4, 3)).to_mesh_batch()
    assert isinstance(ok, MeshBatch) and ok.face_counts == [2, 1] and ok.vert_counts == [4, 7]


# ---- the C entries and the kernels

def test_entries_were_added_without_an_abi_change():
    import vpn_amd._lib as lib
    L = lib.lib()
    assert L.vpn_abi_version() == lib.ABI_VERSION == 9
    for name in ('vpn_primitive_field', 'vpn_isosurface_workspace', 'vpn_isosurface'):
        assert name in lib.SIGNATURES and hasattr(L, name), name
    big = lib.CONSTANTS['VPN_OCCUPANCY_MAX_ITEMS'] + 1
    ws = L.vpn_isosurface_workspace
    # a row of four ints per workgroup of 256 cells, then one table entry per cell, rounded up to 16 bytes
    want = lambda B, cells: (B * ((cells + 255) // 256 * 16 + cells * 4) + 15) // 16 * 16
    assert ws(1, 2, 2, 2) == 32 and ws(3, 12, 12, 12) == want(3, 1331) and ws(2, 42, 42, 42) == want(2, 68921) == 2 * (270 * 16 + 68921 * 4) + 8
    assert ws(0, 2, 2, 2) == 0 and ws(1, 1, 2, 2) == 0 and ws(1, 2, 2, 1) == 0 and ws(65536, 2, 2, 2) == 0 and ws(1, 2, 2, big) == 0
    assert ws(1, 256, 256, 256) == want(1, 255 ** 3) and ws(1, 257, 256, 256) == 0
    # sizes and limits are looked at before any pointer is followed: host buffers stand in for device memory
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd16 = ctypes.c_void_p(p.value + 8)
    assert p.value % 16 == 0

    def field(params=p, kinds=p, queries=p, f=p, B=1, K=2, Q=4):
        return L.vpn_primitive_field(params, kinds, queries, 1, B, K, Q, f, None)

    for bad in (dict(params=None), dict(kinds=None), dict(queries=None), dict(f=None), dict(B=0), dict(K=0), dict(Q=0), dict(Q=-2)):
        assert field(**bad) == -1, bad
    for too in (dict(B=65536), dict(Q=big), dict(K=lib.CONSTANTS['VPN_MAX_PRIMS'] + 1)):
        assert field(**too) == -2, too

    def iso(fld=p, cx=p, cy=p, cz=p, level=0.0, B=1, Nx=3, Ny=3, Nz=3, mv=8, mf=8, work=p, nbytes=32768, verts=p, faces=p, counts=p):
        return L.vpn_isosurface(fld, cx, cy, cz, level, B, Nx, Ny, Nz, mv, mf, work, nbytes, verts, faces, counts, None)

    need = ws(1, 3, 3, 3)
    for bad in (dict(fld=None), dict(cx=None), dict(cy=None), dict(cz=None), dict(work=None), dict(verts=None), dict(faces=None),
                dict(counts=None), dict(level=float('nan')), dict(level=float('inf')), dict(B=0), dict(Nx=1), dict(Ny=1), dict(Nz=0),
                dict(mv=0), dict(mf=-1), dict(nbytes=need - 1), dict(work=odd16)):
        assert iso(**bad) == -1, bad
    for too in (dict(B=65536), dict(Nx=4097, Ny=4096), dict(Nx=65536, Ny=65536, Nz=65536), dict(mv=big), dict(mf=big)):
        assert iso(**too) == -2, too
    assert not any(buf)                                                       # nothing was written


def test_kernels_use_no_scratch_and_no_atomics():
    from kernel_resources import load_build
    b = load_build()
    assert 'isosurface.hip' in b.SOURCES and b.PER_FILE['isosurface.hip'] == ['-ffp-contract=off']
    rows = kernel_resources('isosurface.hip')
    kernels = ('prim_field_kernel', 'iso_count_kernel', 'iso_scan_kernel', 'iso_vertex_kernel', 'iso_face_kernel')
    for k in kernels:
        hits = [v for name, v in rows.items() if k in name]
        assert len(hits) == 1, (k, list(rows))
        assert hits[0]['ScratchSize'] == 0, (k, hits[0])
    assert len(rows) == len(kernels), list(rows)
    for name in ('isosurface.hip', 'occupancy_prim.h'):
        src = open(os.path.join(b.CSRC, name)).read()
        assert 'atomic' not in src.split('#include', 1)[1], name
