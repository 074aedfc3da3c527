"""CPU checks of the point-to-surface distance (vpn_amd.point_mesh_distance, point_mesh_nearest, ops.mesh_incidence,
ops.PointMeshFunction, PointMeshDistanceLoss, csrc/pointmesh.hip): the restatement of tests/pointmesh_ref.py
against a plain-Python closest-point routine, the incidence table against plain loops, the argument contract, the C entries,
the kernels' resources and the conditioning of the inputs the GPU test uses."""
import math

import pytest
import torch

import meshreg_ref as M
import pointmesh_ref as R
from conftest import rel_err
from kernel_resources import kernel_resources

NAMES = sorted(M.MESHES)


def _closest_plain(p, a, b, c):
    """Ericson, Real-Time Collision Detection 5.1.5, on Python floats: (squared distance, closest point, region)."""
    sub = lambda x, y: [x[k] - y[k] for k in range(3)]
    dot = lambda x, y: sum(x[k] * y[k] for k in range(3))
    at = lambda q, region: (dot(sub(p, q), sub(p, q)), q, region)
    ab, ac, ap = sub(b, a), sub(c, a), sub(p, a)
    d1, d2 = dot(ab, ap), dot(ac, ap)
    if d1 <= 0 and d2 <= 0:
        return at(a, R.CORNER0)
    bp = sub(p, b)
    d3, d4 = dot(ab, bp), dot(ac, bp)
    if d3 >= 0 and d4 <= d3:
        return at(b, R.CORNER1)
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        v = d1 / (d1 - d3)
        return at([a[k] + v * ab[k] for k in range(3)], R.EDGE0)
    cp = sub(p, c)
    d5, d6 = dot(ab, cp), dot(ac, cp)
    if d6 >= 0 and d5 <= d6:
        return at(c, R.CORNER2)
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        w = d2 / (d2 - d6)
        return at([a[k] + w * ac[k] for k in range(3)], R.EDGE2)
    va = d3 * d6 - d5 * d4
    if va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        return at([b[k] + w * (c[k] - b[k]) for k in range(3)], R.EDGE1)
    den = 1.0 / (va + vb + vc)
    v, w = vb * den, vc * den
    return at([a[k] + ab[k] * v + ac[k] * w for k in range(3)], R.FACE)


def test_restatement_equals_a_plain_closest_point_routine_in_every_region():
    points, verts, faces, regions = R.one_triangle()
    assert sorted(set(regions.tolist())) == list(range(7))
    p, v = points.double(), verts.double()
    d, w, region = R.closest(p[:, 0], v[:, 0], v[:, 1], v[:, 2])
    assert torch.equal(region, regions)
    for i in range(p.shape[0]):
        want_d, want_c, want_region = _closest_plain(p[i, 0].tolist(), *v[i].tolist())
        assert want_region == int(regions[i]), i
        assert abs(float(d[i]) - want_d) <= 1e-13 * want_d, (i, float(d[i]), want_d)
        c = (w[i, :, None] * v[i]).sum(0)
        assert max(abs(float(c[k]) - want_c[k]) for k in range(3)) <= 1e-13, i
        assert abs(float(w[i].sum()) - 1) <= 1e-15 and float(w[i].min()) >= 0
    # a few pairs of the random inputs too, through the table
    pts, vs, fs = R.case_inputs('irregular', 1, 64)
    table = R.pair_table(pts.double(), vs.double(), fs)
    for i in range(0, 64, 7):
        for f in (3, 5, 6, 7):                       # the faces with area
            want = _closest_plain(pts[0, i].double().tolist(), *vs[0, fs[f]].double().tolist())[0]
            assert abs(float(table[0, i, f]) - want) <= 1e-12 * max(want, 1e-3), (i, f)


def test_degenerate_faces_are_their_segment_and_point():
    v = torch.tensor([[[0.0, 0, 0], [2, 0, 0], [1, 0, 0], [0, 0, 2]]], dtype=torch.float64)
    p = torch.tensor([[[1.0, 1, 1], [3, 0, 0], [0, 0, 3]]], dtype=torch.float64)
    table = R.pair_table(p, v, torch.tensor([[0, 1, 2], [3, 3, 3], [2, 2, 0]]))
    assert table[0].tolist() == [[2.0, 3.0, 2.0], [1.0, 13.0, 4.0], [9.0, 1.0, 9.0]]
    dp, dv = R.gradient(p, v, torch.tensor([[0, 1, 2], [3, 3, 3]]), torch.tensor([[0, 0, 1]]), torch.tensor([[1, 2]]))
    assert torch.isfinite(dp).all() and torch.isfinite(dv).all()


def test_gradient_is_the_derivative_of_the_statement():
    """The explicit gradient at the restatement's own indices against central differences of its two means."""
    pts, vs, fs = R.case_inputs('two_components', 1, 64)
    pts, vs = pts.double(), vs.double()
    _, fop, _, pof, _ = R.nearest(pts, vs, fs)
    dp, dv = R.gradient(pts, vs, fs, fop, pof, R.UPSTREAM)

    def value(a, b):
        dist_p, _, dist_f, _, _ = R.nearest(a, b, fs)
        return R.UPSTREAM[0] * float(dist_p.mean()) + R.UPSTREAM[1] * float(dist_f.mean())

    h = 1e-6
    for x, g, which in ((pts, dp, 0), (vs, dv, 1)):
        num = torch.zeros_like(x)
        for i in range(x.shape[1]):
            for k in range(3):
                keep = float(x[0, i, k])
                x[0, i, k] = keep + h
                hi = value(pts, vs)
                x[0, i, k] = keep - h
                lo = value(pts, vs)
                x[0, i, k] = keep
                num[0, i, k] = (hi - lo) / (2 * h)
        assert rel_err(g, num) <= 1e-6, (which, rel_err(g, num))


@pytest.mark.parametrize('name', NAMES)
def test_incidence_equals_plain_loops(name):
    from vpn_amd import ops
    faces, n = M.mesh(name)
    inc = ops.mesh_incidence(faces, n, 'cpu')
    h = inc.host
    assert all(t.dtype == torch.int32 and t.is_contiguous() for t in h.values())
    assert torch.equal(h['faces'].long(), faces.long()) and inc.F == faces.shape[0] and inc.n == n
    fl = faces.tolist()
    per = [sorted(4 * f + c for f in range(len(fl)) for c in range(3) if fl[f][c] == i) for i in range(n)]
    ptr, vf = h['vf_ptr'].tolist(), h['vf'].tolist()
    assert len(ptr) == n + 1 and ptr[0] == 0 and ptr[-1] == len(vf) == 3 * len(fl)
    assert [vf[ptr[i]:ptr[i + 1]] for i in range(n)] == per


def test_incidence_is_cached_by_content_and_leaves_the_topology_alone():
    from vpn_amd import ops
    faces, n = M.mesh('irregular')
    inc = ops.mesh_incidence(faces, n, 'cpu')
    assert ops.mesh_incidence(faces.clone(), n, 'cpu') is inc and ops.mesh_incidence(faces, n + 1, 'cpu') is not inc
    assert inc.host['vf_ptr'][9] == inc.host['vf_ptr'][8]                      # vertex 8 is in no face
    assert inc.host['vf'][inc.host['vf_ptr'][3]:inc.host['vf_ptr'][4]].tolist() == [4 * 3 + 1, 4 * 4 + 0, 4 * 4 + 1]   # face (3, 3, 4) counts per corner
    topo = ops.mesh_topology(faces, n, 'cpu')
    assert sorted(topo.host) == ['adj', 'edges', 'faces', 'nbr', 'nbr_ptr', 'vf', 'vf_ptr']
    assert topo.host['vf'].numel() < inc.host['vf'].numel()                    # MeshTopology.vf lists the faces with a pair only
    with pytest.raises(ValueError, match='index vertex 5'):
        ops.mesh_incidence(torch.tensor([[0, 1, 5]]), 4, 'cpu')
    with pytest.raises(ValueError, match='index vertex -1'):
        ops.mesh_incidence(torch.tensor([[0, 1, -1]]), 4, 'cpu')


def test_contract_is_checked_before_any_launch():
    """On CPU tensors: one ValueError per rule, from shapes and dtypes alone; a valid call has no CPU path."""
    import vpn_amd
    from vpn_amd import ops
    faces, n = M.mesh('tetrahedron')
    v, p = torch.zeros(2, n, 3), torch.zeros(2, 5, 3)
    for fn in (vpn_amd.point_mesh_distance, vpn_amd.point_mesh_nearest):
        with pytest.raises(ValueError, match=r'points must be \[B,P,3\]'):
            fn(p[0], v, faces)
        with pytest.raises(ValueError, match=r'verts must be \[B,V,3\]'):
            fn(p, torch.zeros(2, n, 2), faces)
        with pytest.raises(ValueError, match=r'points must be \[B,P,3\]'):
            fn(p[:, :0], v, faces)
        with pytest.raises(ValueError, match='points must be float32'):
            fn(p.double(), v, faces)
        with pytest.raises(ValueError, match='verts must be float32'):
            fn(p, v.half(), faces)
        with pytest.raises(ValueError, match='one batch size'):
            fn(p[:1], v, faces)
        with pytest.raises(ValueError, match=r'faces must be \[F,3\]'):
            fn(p, v, faces[None].expand(2, -1, -1))
        with pytest.raises(ValueError, match=r'faces must be \[F,3\]'):
            fn(p, v, faces[:0])
        with pytest.raises(ValueError, match='faces must be int32 or int64'):
            fn(p, v, faces.float())
        with pytest.raises(ValueError, match='index vertex 3'):
            fn(p, v[:, :3].contiguous(), faces)
        with pytest.raises(RuntimeError, match='GPU only'):
            fn(p, v, faces)
    with pytest.raises(RuntimeError, match='GPU only'):
        vpn_amd.PointMeshDistanceLoss(1.0, 0.5)(p, v, faces)
    inc = ops.mesh_incidence(faces, n, 'cpu')                                # the Function guards itself: an incidence of another size
    with pytest.raises(ValueError, match=r'verts float32 \[B,4,3\] for this incidence'):
        ops.PointMeshFunction.apply(p, torch.zeros(2, n + 1, 3), inc)
    assert vpn_amd.PointMeshFunction is ops.PointMeshFunction and vpn_amd.mesh_incidence is ops.mesh_incidence
    loss = vpn_amd.PointMeshDistanceLoss(1.0, 0.0)
    assert loss.weights == (1.0, 0.0) and loss.last is None and vpn_amd.PointMeshDistanceLoss().weights == (1.0, 1.0)
    assert vpn_amd.modules.loss.PointMeshDistanceLoss is vpn_amd.PointMeshDistanceLoss


def test_entries_were_added_without_an_abi_change():
    import ctypes
    import vpn_amd._lib as lib
    L = lib.lib()
    assert L.vpn_abi_version() == lib.ABI_VERSION == 9
    for name in ('vpn_pointmesh_workspace', 'vpn_pointmesh_fwd', 'vpn_pointmesh_bwd'):
        assert name in lib.SIGNATURES and hasattr(L, name), name
    H = lib.CONSTANTS
    assert (H['VPN_POINTMESH_TILE'], H['VPN_POINTMESH_MIN_SLICE'], H['VPN_POINTMESH_MAX_SLICES']) == (256, 128, 64)
    big = H['VPN_POINTMESH_MAX_ITEMS'] + 1
    # words: 16 a face record, two a partial minimum per (slice, point) and per (tile, face), two sums per 256-item chunk.
    # B = 8, P = 2048, F = 4032: 8 tiles, 16 slices of 252 faces; the sphere at B = 3, P = 257: 2 tiles, 2 slices of 126
    assert L.vpn_pointmesh_workspace(8, 2048, 2048, 4032) == 4 * (8 * 4032 * 16 + 8 * 16 * 2048 * 2 + 8 * 8 * 4032 * 2 + 8 * 16 * 2)
    assert L.vpn_pointmesh_workspace(3, 257, 128, 252) == 4 * (3 * 252 * 16 + 3 * 2 * 257 * 2 + 3 * 2 * 252 * 2 + 3 * 2 * 2)
    assert L.vpn_pointmesh_workspace(1, 1, 4, 4) == 4 * (4 * 16 + 2 + 4 * 2 + 2)
    assert L.vpn_pointmesh_workspace(0, 4, 4, 4) == 0 and L.vpn_pointmesh_workspace(1, 4, 0, 4) == 0
    assert L.vpn_pointmesh_workspace(1, big, 4, 4) == 0 and L.vpn_pointmesh_workspace(65536, 4, 4, 4) == 0
    roomy = 1 << 40
    fwd_null = (None,) * 3 + (1, 4, 4, 4, None, roomy) + (None,) * 6
    bwd_null = (None,) * 8 + (1, 4, 4, 4, None, roomy) + (None,) * 3
    assert L.vpn_pointmesh_fwd(*fwd_null) == -1 and L.vpn_pointmesh_bwd(*bwd_null) == -1
    # sizes and limits are looked at before any pointer is followed: host buffers stand in for device memory
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(B=1, P=4, V=4, F=4, ws=roomy):
        return L.vpn_pointmesh_fwd(p, p, p, B, P, V, F, p, ws, p, p, p, p, p, None)

    def bwd(B=1, P=4, V=4, F=4, ws=roomy):
        return L.vpn_pointmesh_bwd(p, p, p, p, p, p, p, p, B, P, V, F, p, ws, p, p, None)

    for call in (fwd, bwd):
        for bad in (dict(B=0), dict(P=0), dict(V=0), dict(F=0), dict(B=-1), dict(ws=0)):
            assert call(**bad) == -1, (call.__name__, bad)
        for too in (dict(B=65536), dict(P=big), dict(V=big), dict(F=big)):
            assert call(**too) == -2, (call.__name__, too)
    assert fwd(ws=L.vpn_pointmesh_workspace(1, 4, 4, 4) - 1) == -1 and bwd(ws=4 * 9 * 4 - 1) == -1
    assert L.vpn_pointmesh_bwd(p, p, p, p, p, p, None, None, 1, 4, 4, 4, p, roomy, p, p, None) == -1      # dverts without its table


def test_kernels_use_no_scratch():
    from kernel_resources import load_build
    b = load_build()
    assert 'pointmesh.hip' in b.SOURCES and 'pointmesh.hip' not in b.PER_FILE
    rows = kernel_resources('pointmesh.hip')
    kernels = ('pointmesh_prep_kernel', 'pointmesh_pair_kernel', 'pointmesh_merge_kernel', 'pointmesh_final_kernel',
               'pointmesh_bwd_face_kernel', 'pointmesh_bwd_point_kernel', 'pointmesh_bwd_gather_kernel')
    for k in kernels:
        hits = [v for name, v in rows.items() if k in name]
        assert len(hits) == 1, (k, list(rows))
        assert hits[0]['ScratchSize'] == 0, (k, hits[0])
    assert len(rows) == len(kernels), list(rows)


@pytest.mark.parametrize('name,B,P', R.CASES, ids=lambda v: str(v))
def test_inputs_of_the_gpu_test_are_well_conditioned(name, B, P):
    """The restatement in fp32 against itself in float64 on the inputs tests/test_pointmesh.py uses stays within a quarter of
    each 1e-4 bar of that test: the two means, dist_p and dist_f by rel_err, and the index rule (the float64 distance of the
    pair an fp32 index names over the float64 minimum, as a fraction of the sample's largest minimum)."""
    dp64, fop64, df64, pof64, table, out64 = R.reference64(name, B, P)
    dp32, fop32, df32, pof32, _, out32 = R.reference32(name, B, P)
    quarter = 0.25e-4
    errs = [abs(float(out32[k]) - float(out64[k])) / float(out64[k]) for k in range(2)]
    errs += [rel_err(dp32, dp64), rel_err(df32, df64)]
    errs += [float(R.index_excess(table, dp64, fop32, 2).max()), float(R.index_excess(table, df64, pof32, 1).max())]
    print('%s B %d P %d: means %.1e %.1e, distances %.1e %.1e, index excess %.1e %.1e' % ((name, B, P) + tuple(errs)))
    assert max(errs) <= quarter, errs
    assert float(R.index_excess(table, dp64, fop64, 2).abs().max()) == 0 and float(R.index_excess(table, df64, pof64, 1).abs().max()) == 0
    inputs = R.case_inputs(name, B, P)
    own = [rel_err(a, b) for a, b in zip(R.gradient(*inputs, fop32, pof32, R.UPSTREAM, torch.float32),
                                         R.gradient(*inputs, fop32, pof32, R.UPSTREAM))]
    print('    own gradient error at the fp32 indices: dpoints %.1e dverts %.1e' % tuple(own))
    assert all(math.isfinite(e) for e in own)


def test_every_region_occurs_among_the_records_of_the_gpu_test():
    seen = set(R.one_triangle()[3].tolist())
    assert seen == set(range(7))                                            # the one-triangle case alone has all seven
    random = set()
    for name, B, P in R.CASES:
        pts, vs, fs = R.case_inputs(name, B, P)
        _, fop, _, pof, _, _ = R.reference64(name, B, P)
        for _, _, region, _ in R.records(pts.double(), vs.double(), fs, fop, pof):
            random |= set(region.flatten().tolist())
    assert {R.FACE, R.EDGE0, R.EDGE1, R.EDGE2} <= random, random            # the parity cases: the face and every edge at least
