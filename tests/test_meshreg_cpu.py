"""CPU checks of the mesh regularisers (vpn_amd.mesh_regularizers, ops.mesh_topology, ops.MeshRegFunction,
MeshRegularizationLoss, csrc/meshreg.hip): the host-built topology against the plain-Python one of
tests/meshreg_ref.py, the conditioning of the inputs the GPU test uses, the argument contract, the C entries and the
kernels' resources."""
import pytest
import torch

import meshreg_ref as M
from conftest import rel_err
from kernel_resources import kernel_resources

NAMES = sorted(M.MESHES)


def _check_tables(topo, ref, faces, n):
    """ops.MeshTopology `topo` says what the restatement's topology `ref` says, table by table."""
    h = topo.host
    assert all(t.dtype == torch.int32 and t.is_contiguous() for t in h.values())
    assert torch.equal(h['faces'].long(), faces.long())
    assert [tuple(e) for e in h['edges'].tolist()] == ref['edges'] and topo.E == len(ref['edges'])
    ptr, nbr = h['nbr_ptr'].tolist(), h['nbr'].tolist()
    assert len(ptr) == n + 1 and ptr[0] == 0 and ptr[-1] == len(nbr) == 2 * topo.E
    assert [nbr[ptr[i]:ptr[i + 1]] for i in range(n)] == ref['neighbours']
    assert [tuple(p) for p in topo.pairs.tolist()] == ref['pairs'] and topo.n_pairs == len(ref['pairs'])
    assert (topo.n_boundary, topo.n_nonmanifold) == (ref['n_boundary'], ref['n_nonmanifold'])
    assert topo.n_flipped == sum(s < 0 for _, _, s in ref['pairs'])
    # adj: every pair stands in both faces, at the slot of the shared edge, and nothing else does
    adj, fl = h['adj'].tolist(), faces.tolist()
    want = [[-1, -1, -1] for _ in fl]
    for f, g, s in ref['pairs']:
        for me, other in ((f, g), (g, f)):
            slots = [j for j in range(3) if {fl[me][j], fl[me][(j + 1) % 3]} <= set(fl[other]) and fl[me][j] != fl[me][(j + 1) % 3]]
            assert len(slots) == 1, (me, other)
            want[me][slots[0]] = 2 * other + (s < 0)
    assert adj == want
    # vf: per vertex the (face, corner) of every face that has a pair
    vp, vf = h['vf_ptr'].tolist(), h['vf'].tolist()
    paired = [f for f in range(len(fl)) if max(want[f]) >= 0]
    per = [sorted(4 * f + c for f in paired for c in range(3) if fl[f][c] == i) for i in range(n)]
    assert len(vp) == n + 1 and vp[0] == 0 and [vf[vp[i]:vp[i + 1]] for i in range(n)] == per


@pytest.mark.parametrize('name', NAMES)
def test_topology_equals_the_restatement(name):
    from vpn_amd import ops
    faces, n = M.mesh(name)
    topo = ops.mesh_topology(faces, n, 'cpu')
    _check_tables(topo, M.topology(faces, n), faces, n)
    assert topo.F == faces.shape[0] and topo.n == n


def test_topology_of_the_named_meshes():
    from vpn_amd import ops
    t = {name: ops.mesh_topology(*M.mesh(name), 'cpu') for name in NAMES}
    tet = t['tetrahedron']
    assert (tet.n, tet.E, tet.n_pairs, tet.n_flipped, tet.n_boundary, tet.n_nonmanifold) == (4, 6, 6, 0, 0, 0)
    fl = t['tetrahedron_flipped']
    assert (fl.E, fl.n_pairs, fl.n_flipped) == (6, 6, 3)
    assert all((s < 0) == (1 in (f, g)) for f, g, s in fl.pairs.tolist())            # exactly the pairs of the flipped face
    st = t['strip_7']                                                                # 5 faces: 4 inner edges, 7 on the rim
    assert (st.E, st.n_pairs, st.n_boundary, st.n_flipped, st.n_nonmanifold) == (11, 4, 7, 0, 0)
    ir = t['irregular']
    assert ir.n_nonmanifold == 3 and ir.host['nbr_ptr'][9] == ir.host['nbr_ptr'][8]     # the triple face; vertex 8 has deg 0
    assert (3, 4) in [tuple(e) for e in ir.host['edges'].tolist()]                   # the edge of the face with a repeated index
    assert ir.host['adj'][4].tolist() == [-1, -1, -1] and ir.host['adj'][0].tolist() == [-1, -1, -1]
    fan = t['fan_70']
    assert int(fan.host['nbr_ptr'][1]) == 70 and (fan.E, fan.n_pairs, fan.n_boundary) == (140, 70, 70)
    sp = t['uv_sphere']
    assert (sp.n, sp.E, sp.F, sp.n_pairs, sp.n_boundary, sp.n_flipped, sp.n_nonmanifold) == (128, 378, 252, 378, 0, 0, 0)
    two = t['two_components']
    assert (two.E, two.n_pairs, two.n_boundary) == (6 + 7, 6 + 2, 5)
    assert all((f < 4) == (g < 4) for f, g, _ in two.pairs.tolist())                  # no pair across the components


def test_topology_is_cached_by_content_and_checks_indices():
    from vpn_amd import ops
    faces, n = M.mesh('irregular')
    t = ops.mesh_topology(faces, n, 'cpu')
    assert ops.mesh_topology(faces.clone(), n, 'cpu') is t
    assert ops.mesh_topology(faces.int(), n, 'cpu') is not None
    assert ops.mesh_topology(faces, n + 1, 'cpu') is not t
    with pytest.raises(ValueError, match='index vertex 5'):
        ops.mesh_topology(torch.tensor([[0, 1, 5]]), 4, 'cpu')
    with pytest.raises(ValueError, match='index vertex -1'):
        ops.mesh_topology(torch.tensor([[0, 1, -1]]), 4, 'cpu')


CONDITIONING = [(name, B) for name in NAMES for B in (1, 3)] + [('composed', 2)]


@pytest.mark.parametrize('name,B', CONDITIONING, ids=lambda v: str(v))
@pytest.mark.parametrize('l0', [0.0, 0.05])
def test_inputs_of_the_gpu_test_are_well_conditioned(name, B, l0):
    """The restatement in fp32 against itself in float64 on the inputs tests/test_meshreg.py uses: rel_err <= 1e-4 on every
    value and gradient, so that the bar of the GPU test measures the kernels and not the inputs.  Measured here ("own"
    errors, worst over all cases): values 6.2e-7 (normal, strip_7); edge gradient 3.4e-7 (fan_70), Laplacian gradient
    6.0e-6 (strip_130), normal gradient 4.9e-6 (uv_sphere, B = 1); the composed mesh at B = 2: 1.2e-7, 8.7e-7, 1.8e-6."""
    faces, _ = M.mesh(name)
    for terms in (M.TERMS,) + tuple((t,) for t in M.TERMS):
        v64, g64 = M.reference64(name, B, l0, terms)
        v32, g32 = M.reference32(name, B, l0, terms)
        for k in range(3):
            assert abs(float(v32[k]) - float(v64[k])) <= 1e-4 * abs(float(v64[k])), (terms, k, v32, v64)
        if float(g64.abs().max()) > 0:
            assert rel_err(g32, g64) <= 1e-4, (terms, rel_err(g32, g64))


def test_degenerate_geometry_has_the_stated_values():
    """A zero-area face, a zero-length edge with l0 > 0, two coincident vertices: finite values, and the stated ones."""
    v, f, l0 = M.degenerate()
    v = v.double()
    topo = M.topology(f, 6)
    out, dv = M.reference(v, f, l0)
    assert torch.isfinite(out).all() and torch.isfinite(dv).all()
    n = torch.cross(v[0, f[:, 1]] - v[0, f[:, 0]], v[0, f[:, 2]] - v[0, f[:, 0]], dim=-1)
    assert n[0].abs().max() == 0 and n[3].abs().max() == 0 and n[1].abs().max() > 0
    # a pair with a zero-area face has cos = 0: its term is exactly 1
    dead = [(a, b) for a, b, _ in topo['pairs'] if a in (0, 3) or b in (0, 3)]
    assert dead and len(dead) < len(topo['pairs'])
    e_only, de = M.reference(v, f, l0, ('edge',))
    lengths = [float((v[0, a] - v[0, b]).norm()) for a, b in topo['edges']]
    assert 0.0 in lengths                                                         # edge (4, 5)
    assert abs(float(e_only[0]) - sum((x - l0) ** 2 for x in lengths) / len(lengths)) < 1e-12
    # the zero-length edge pulls neither end: with only that edge different, 4 and 5 get the gradients of their other edges
    want4 = sum((2 / len(lengths)) * (1 - l0 / float((v[0, 4] - v[0, j]).norm())) * (v[0, 4] - v[0, j])
                for j in topo['neighbours'][4] if j != 5)
    assert torch.allclose(de[0, 4], want4, atol=1e-12)


def test_contract_is_checked_before_any_launch():
    """On CPU tensors: one ValueError per rule, from shapes and dtypes alone; a valid call has no CPU path."""
    import vpn_amd
    from vpn_amd import ops
    faces, n = M.mesh('tetrahedron')
    v = torch.zeros(2, n, 3)
    with pytest.raises(ValueError, match=r'verts must be \[B,V,3\]'):
        vpn_amd.mesh_regularizers(v[0], faces)
    with pytest.raises(ValueError, match=r'verts must be \[B,V,3\]'):
        vpn_amd.mesh_regularizers(torch.zeros(2, n, 2), faces)
    with pytest.raises(ValueError, match='verts must be float32'):
        vpn_amd.mesh_regularizers(v.double(), faces)
    with pytest.raises(ValueError, match=r'faces must be \[F,3\]'):
        vpn_amd.mesh_regularizers(v, faces[None].expand(2, -1, -1))
    with pytest.raises(ValueError, match=r'faces must be \[F,3\]'):
        vpn_amd.mesh_regularizers(v, faces[:0])
    with pytest.raises(ValueError, match='faces must be int32 or int64'):
        vpn_amd.mesh_regularizers(v, faces.float())
    with pytest.raises(ValueError, match='index vertex 3'):
        vpn_amd.mesh_regularizers(v[:, :3].contiguous(), faces)
    with pytest.raises(ValueError, match='unknown term'):
        vpn_amd.mesh_regularizers(v, faces, terms=('edge', 'cotangent'))
    for bad in (-0.1, float('nan'), float('inf'), '0'):
        with pytest.raises(ValueError, match='edge_target'):
            vpn_amd.mesh_regularizers(v, faces, edge_target=bad)
    for terms in (M.TERMS, ('lap',), ()):
        with pytest.raises(RuntimeError, match='GPU only'):
            vpn_amd.mesh_regularizers(v, faces, 0.05, terms)
    with pytest.raises(RuntimeError, match='GPU only'):
        vpn_amd.MeshRegularizationLoss(1.0, 0.0, 0.5)(v, faces)
    topo = ops.mesh_topology(faces, n, 'cpu')                               # the Function guards itself: a topology of another size
    with pytest.raises(ValueError, match=r'float32 \[B,4,3\] for this topology'):
        ops.MeshRegFunction.apply(torch.zeros(2, n + 1, 3), topo, 0.0, 7)
    with pytest.raises(ValueError, match='terms is a mask'):
        ops.MeshRegFunction.apply(v, topo, 0.0, 8)
    assert vpn_amd.MeshRegFunction is ops.MeshRegFunction and vpn_amd.mesh_topology is ops.mesh_topology
    assert ops.meshreg_terms_mask(M.TERMS) == 7 and ops.meshreg_terms_mask('lap') == 2 and ops.meshreg_terms_mask(()) == 0
    loss = vpn_amd.MeshRegularizationLoss(1.0, 0.0, 0.5, edge_target=0.1)
    assert loss.terms == ('edge', 'normal') and loss.weights == (1.0, 0.0, 0.5) and loss.edge_target == 0.1 and loss.last is None
    assert vpn_amd.modules.loss.MeshRegularizationLoss is vpn_amd.MeshRegularizationLoss


def test_entries_were_added_without_an_abi_change():
    import ctypes
    import vpn_amd._lib as lib
    L = lib.lib()
    assert L.vpn_abi_version() == lib.ABI_VERSION == 9
    for name in ('vpn_meshreg_workspace', 'vpn_meshreg_fwd', 'vpn_meshreg_bwd'):
        assert name in lib.SIGNATURES and hasattr(L, name), name
    H = lib.CONSTANTS
    assert (H['VPN_MESHREG_EDGE'], H['VPN_MESHREG_LAP'], H['VPN_MESHREG_NORMAL'], H['VPN_MESHREG_CHUNK']) == (1, 2, 4, 256)
    # three sums per (sample, 256-item chunk of the longest of vertices, edges, faces)
    assert L.vpn_meshreg_workspace(8, 2048, 6048, 4032) == 8 * 24 * 3 * 4
    assert L.vpn_meshreg_workspace(2, 256, 0, 1) == 2 * 1 * 3 * 4 and L.vpn_meshreg_workspace(2, 257, 0, 1) == 2 * 2 * 3 * 4
    assert L.vpn_meshreg_workspace(0, 4, 6, 4) == 0 and L.vpn_meshreg_workspace(1, 4, -1, 4) == 0
    assert L.vpn_meshreg_workspace(1, H['VPN_MESHREG_MAX_ITEMS'] + 1, 6, 4) == 0 and L.vpn_meshreg_workspace(65536, 4, 6, 4) == 0
    fwd_null = (None,) * 6 + (1, 4, 6, 4, 6, 0.0, 7) + (None,) * 5
    bwd_null = (None,) * 10 + (1, 4, 6, 4, 6, 0.0, 7) + (None,) * 2
    assert L.vpn_meshreg_fwd(*fwd_null) == -1 and L.vpn_meshreg_bwd(*bwd_null) == -1
    # sizes and limits are looked at before any pointer is followed: host buffers stand in for device memory
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(B=1, V=4, E=6, F=4, P=6, l0=0.0, terms=7):
        return L.vpn_meshreg_fwd(p, p, p, p, p, p, B, V, E, F, P, l0, terms, p, p, p, p, None)

    def bwd(B=1, V=4, E=6, F=4, P=6, l0=0.0, terms=7):
        return L.vpn_meshreg_bwd(p, p, p, p, p, p, p, p, p, p, B, V, E, F, P, l0, terms, p, None)

    for call in (fwd, bwd):
        for bad in (dict(B=0), dict(V=0), dict(F=0), dict(E=-1), dict(P=-1), dict(terms=8), dict(terms=-1), dict(l0=-1.0),
                    dict(l0=float('nan')), dict(l0=float('inf'))):
            assert call(**bad) == -1, (call.__name__, bad)
        for big in (dict(B=65536), dict(V=H['VPN_MESHREG_MAX_ITEMS'] + 1), dict(E=H['VPN_MESHREG_MAX_ITEMS'] + 1),
                    dict(F=H['VPN_MESHREG_MAX_ITEMS'] + 1)):
            assert call(**big) == -2, (call.__name__, big)


def test_kernels_use_no_scratch():
    from kernel_resources import load_build
    b = load_build()
    assert 'meshreg.hip' in b.SOURCES and 'meshreg.hip' not in b.PER_FILE
    rows = kernel_resources('meshreg.hip')
    for k in ('meshreg_fwd_kernel', 'meshreg_final_kernel', 'meshreg_bwd_kernel'):
        hits = [v for name, v in rows.items() if k in name]
        assert len(hits) == 1, (k, list(rows))
        assert hits[0]['ScratchSize'] == 0, (k, hits[0])
    assert len(rows) == 3, list(rows)
