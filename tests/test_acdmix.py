"""GPU checks of the ACD-mix stage (csrc/acdmix.hip, ops.acd_mix_points, modules/augmentation.acd_mix_data).

The two kernels against tests/acdmix_ref.py: keep, out, support, outside, src and count are compared with np.array_equal --
every decision of the specification is a comparison of values rounded per operation, so there is no tolerance to choose.
The restatement is fed the GPU's own candidates: they come from the mesh sampler (csrc/mesh.hip), which is built with
contraction allowed and is not what is under test here.  The one bound in this file is the one of test_reconstruct.py for
sampled points: within gamma_3 sum_k |w_k v_k| of the exact combination of the recorded face, gamma_3 = 3 u / (1 - 3 u),
u = 2^-24.  'max' is both limits of the kernels at once (G = 64, D = 256)."""
import functools

import numpy as np
import pytest
import torch

import acdmix_ref as AR
import reconstruct_ref as RR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F = np.float32
MARGIN = 1e-3
SHAPES = {'b': (3, 16, 114, 1000, 700), 'max': (2, 64, 256, 4096, 2048)}           # (S, G, D, nc, n_out)


def _template(D, seed):
    """(directions [D,3], faces [Ft,3]) as host tensors: a face list over D vertices is all the sampler needs."""
    rng = np.random.default_rng(seed)
    faces = np.stack([rng.permutation(D)[:3] for _ in range(2 * D - 4)]).astype(np.int64)
    return torch.from_numpy(RR.random_dirs(D, seed)), torch.from_numpy(faces)


def _random_draws(S, O, G, rng):
    return dict(coin=rng.integers(0, 2, (S, O)).astype(np.int32), u_num=rng.random((S, O), dtype=F),
                scale=(F(0.8) + rng.random((S, O), dtype=F) * F(0.4)).astype(F), turn=rng.integers(0, 5, (S, O)).astype(np.int32),
                shift=((rng.random((S, O), dtype=F) - F(0.5)) / F(5)).astype(F),
                u_hull=(rng.integers(0, 4, (S, G)) / 4).astype(F))                 # few distinct keys: equal keys do occur


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs of a named case, the GPU's outputs (as numpy) and the restatement's, computed once."""
    from vpn_amd import ops
    S, G, D, nc, n_out = SHAPES[name]
    rng = np.random.default_rng(100 + G)
    tv, tf = _template(D, 3)
    dirs = (tv / tv.norm(dim=1, keepdim=True)).numpy()                           # hull_template's normalisation
    centre = (rng.random((S, G, 3)) - 0.5) * np.array([0.8, 0.8, 0.5])
    radii = 0.08 + rng.random((S, G, 3)) * 0.2
    verts = np.stack([np.stack([AR.ellipsoid_hull(centre[s, g], radii[s, g], dirs) for g in range(G)]) for s in range(S)])
    draws = _random_draws(S, 2, G, rng)
    H = G // 2
    v = torch.from_numpy(verts).to(DEV)
    points, count, parts = ops.acd_mix_points(v[:, :H], v[:, H:], draws['coin'], draws['u_num'], draws['scale'], draws['turn'],
                                              draws['shift'], draws['u_hull'], n_out, 1234, 5, n_cand=nc, margin=MARGIN, template=(tv, tf))
    torch.cuda.synchronize()
    gpu = {k: t.cpu().numpy() for k, t in parts.items()}
    gpu.update(points=points.cpu().numpy(), count=count.cpu().numpy())
    group = np.array([0] * H + [1] * H, np.int32)
    ref_out, ref_keep = AR.hull_augment(verts, group, **draws)
    ref = AR.union_surface(gpu['hulls'], gpu['keep'], dirs, gpu['cand'], gpu['cand_hull'], MARGIN, n_out)
    return dict(verts=verts, dirs=dirs, draws=draws, gpu=gpu, ref_out=ref_out, ref_keep=ref_keep, ref=ref, template=(tv, tf))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _assert_union(got, want):
    names = ('support', 'outside', 'points', 'src', 'count')
    for n, g, w in zip(names, got, want):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == w.dtype and g.shape == w.shape, n
        assert np.array_equal(_bits(g) if g.dtype == np.float32 else g, _bits(w) if w.dtype == np.float32 else w), n


@pytest.mark.parametrize('name', ['b', 'max'])
def test_kernels_equal_the_restatement_bit_for_bit(name):
    c = _case(name)
    S, G, D, nc, n_out = SHAPES[name]
    gpu = c['gpu']
    print('%s: kept %s of %d hulls, count %s of %d candidates' % (name, gpu['keep'].sum(1).tolist(), G, gpu['count'].tolist(), nc))
    assert gpu['keep'].dtype == np.int32 and np.array_equal(gpu['keep'], c['ref_keep'])
    assert np.array_equal(_bits(gpu['hulls']), _bits(c['ref_out']))
    assert 0 < gpu['keep'].sum() < S * G                               # the cut-out did cut, and not everything
    assert gpu['cand'].shape == (S, nc, 3) and gpu['cand_hull'].min() >= 0 and gpu['cand_hull'].max() < G
    _assert_union([gpu[k] for k in ('support', 'outside', 'points', 'src', 'count')], c['ref'])
    assert (gpu['count'] > 0).all() and (gpu['count'] < nc).any()      # the filter did reject, and not everything


def test_lattice_ties_at_the_margin():
    """(1, 2, 6, 64, 32): axis directions, dyadic hulls, candidates and margin: dot(p, d) == support - margin happens, and
    equality is inside."""
    from vpn_amd import ops
    dirs = AR.lattice_dirs()
    hulls = np.stack([AR.box_hull([-0.5, -0.5, -0.25], [0.25, 0.25, 0.25], dirs), AR.box_hull([0.0, -0.25, -0.5], [0.5, 0.5, 0.5], dirs)])[None]
    draws = dict(coin=[[0, 0]], u_num=[[0.0, 0.0]], scale=[[1.0, 0.5]], turn=[[0, 3]], shift=[[0.125, -0.25]], u_hull=[[0.0, 0.0]])
    cand = (RR.lattice_cloud(4) * F(2.0))[None]                        # 64 points with coordinates in {-0.5, -0.25, 0, 0.25}
    own = ((np.arange(64, dtype=np.int32) // 4) % 2)[None]             # the hull follows the parity of the y index
    margin = 0.125
    out, keep = ops.hull_augment(torch.from_numpy(hulls).to(DEV), [0, 1], **draws)
    ref_out, ref_keep = AR.hull_augment(hulls, [0, 1], **draws)
    assert np.array_equal(keep.cpu().numpy(), ref_keep) and ref_keep.tolist() == [[1, 1]]
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref_out))
    got = ops.union_surface(out, keep, torch.from_numpy(dirs).to(DEV), torch.from_numpy(cand).to(DEV), torch.from_numpy(own).to(DEV), 32, margin)
    want = AR.union_surface(ref_out, ref_keep, dirs, cand, own, margin, 32)
    val = RR.dot(cand[0][:, None, :], dirs[None])
    ties = sum(int((val == (want[0][0, h] - F(margin))[None]).sum()) for h in range(2))
    print('lattice: %d exact ties, count %d' % (ties, int(want[4][0])))
    assert ties >= 10 and 0 < int(want[4][0]) < 64
    _assert_union(got, want)


def test_fewer_survivors_than_slots_and_a_sample_with_every_hull_cut():
    from vpn_amd import ops
    c = _case('b')
    S, G, D, nc, n_out = SHAPES['b']
    gpu = c['gpu']
    t = lambda a: torch.from_numpy(a).to(DEV)
    keep = gpu['keep'].copy()
    keep[1] = 0                                                        # sample 1: every hull cut
    more = nc + 37                                                     # more slots than candidates: count < n_out everywhere
    got = ops.union_surface(t(gpu['hulls']), t(keep), t(c['dirs']), t(gpu['cand']), t(gpu['cand_hull']), more, MARGIN)
    want = AR.union_surface(gpu['hulls'], keep, c['dirs'], gpu['cand'], gpu['cand_hull'], MARGIN, more)
    _assert_union(got, want)
    count, src = want[4], want[3]
    assert count[1] == 0 and src[1].tolist() == [i % nc for i in range(more)] and not want[1][1].any()
    assert 0 < count[0] < more and np.array_equal(src[0, count[0]:2 * count[0]], src[0, :count[0]][:more - count[0]])


def test_oversize_is_refused_before_any_launch():
    from vpn_amd import ops
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    with pytest.raises(RuntimeError, match=r'code -2'):
        ops.hull_augment(z(1, 65, 4, 3), [0] * 65, [[0]], [[0.0]], [[1.0]], [[2]], [[0.0]], [[0.0] * 65])
    with pytest.raises(RuntimeError, match=r'code -2'):
        ops.union_surface(z(1, 2, 257, 3), z(1, 2, dt=torch.int32), z(257, 3), z(1, 8, 3), z(1, 8, dt=torch.int32), 8)
    with pytest.raises(RuntimeError, match=r'code -2'):
        ops.union_surface(z(1, 2, 4, 3), z(1, 2, dt=torch.int32), z(4, 3), z(1, 16385, 3), z(1, 16385, dt=torch.int32), 8)
    torch.cuda.synchronize()


# ---- the stage

S, V, SIZE, N, UNION, NEW, HULLS = 2, 3, 32, 1024, 1024, 2048, 8


@functools.lru_cache(maxsize=None)
def _inputs():
    """Two ellipsoid clouds per sample, centres one semi-axis apart, and every draw of the stage on the device."""
    ra, rb = (0.4, 0.3, 0.25), (0.3, 0.35, 0.3)
    p1 = np.stack([AR.ellipsoid_points((0.0, 0.0, 0.0), ra, N, 11 + s) for s in range(S)])
    p2 = np.stack([AR.ellipsoid_points((0.4, 0.0, 0.0), rb, N, 21 + s) for s in range(S)])
    g = torch.Generator().manual_seed(4)
    t = lambda a: a.to(DEV)
    draws = dict(coin=t(torch.tensor([[0, 1], [1, 0]], dtype=torch.int32)), u_num=t(torch.rand(S, 2, generator=g)),
                 scale=t(0.8 + torch.rand(S, 2, generator=g) * 0.4), turn=t(torch.tensor([[2, 0], [1, 3]], dtype=torch.int32)),
                 shift=t((torch.rand(S, 2, generator=g) - 0.5) / 5), u_hull=t(torch.rand(S, 2 * HULLS, generator=g)),
                 colors=t(torch.rand(S, HULLS, 3, generator=g)),
                 cams=t(torch.stack([3.0 + torch.rand(S, V, generator=g) * 2, (torch.rand(S, V, generator=g) - 0.5) * 90,
                                     torch.rand(S, V, generator=g) * 360], -1)))
    torch.cuda.synchronize()
    return torch.from_numpy(p1).to(DEV), torch.from_numpy(p2).to(DEV), draws


def _stage(**kw):
    import vpn_amd
    p1, p2, draws = _inputs()
    return vpn_amd.acd_mix_data(p1, p2, views=V, img_size=SIZE, num_points=NEW, union_points=UNION, seed=77, gt_seed=78, **draws, **kw)


def test_acd_mix_data():
    import vpn_amd
    from vpn_amd import PhongRenderer, TriangleMesh, VertexRenderer
    p1, p2, draws = _inputs()
    rgba, centred, gt_points, dists, elevs, azims, parts = _stage(return_parts=True)
    P = HULLS * 128
    assert rgba.shape == (S, V, 4, SIZE, SIZE) and centred.shape == (S, V, P, 3) and gt_points.shape == (S, V, NEW, 3)
    assert dists.shape == elevs.shape == azims.shape == (S, V)
    assert all(t.dtype == torch.float32 and not t.requires_grad for t in (rgba, centred, gt_points, dists, elevs, azims))
    assert float(rgba.min()) >= 0.0 and float(rgba.max()) <= 1.0
    assert float(rgba[:, :, 3].max()) > 0.5 and float(rgba[:, :, :3].max()) > 0.0          # the meshes are in the picture
    assert torch.equal(torch.stack([dists, elevs, azims], -1), draws['cams'])
    faces, uv, texture, verts = parts['faces'], parts['uv'], parts['texture'], parts['verts']
    assert faces.shape == (HULLS * 252, 3) and uv.shape == (S, P, 2) and texture.shape == (S, 3, 1, HULLS) and verts.shape == (S, P, 3)
    # the overlap condition: nc = 2 n_out, and the restatement alone (on the GPU's candidates) leaves count >= n_out
    assert parts['cand'].shape == (S, 2 * UNION, 3)
    dirs = vpn_amd.ops.hull_template(2 * HULLS, 'cpu')[0].numpy()
    h1 = vpn_amd.acd(p1 / p1.amax(dim=(1, 2), keepdim=True), HULLS)
    h2 = vpn_amd.acd(p2 / p2.amax(dim=(1, 2), keepdim=True), HULLS)
    merged = torch.cat([h1, h2], 1).cpu().numpy()
    d = {k: draws[k].cpu().numpy() for k in ('coin', 'u_num', 'scale', 'turn', 'shift', 'u_hull')}
    ref_out, ref_keep = AR.hull_augment(merged, [0] * HULLS + [1] * HULLS, **d)
    assert np.array_equal(parts['keep'].cpu().numpy(), ref_keep) and np.array_equal(_bits(parts['hulls'].cpu().numpy()), _bits(ref_out))
    ref = AR.union_surface(ref_out, ref_keep, dirs, parts['cand'].cpu().numpy(), parts['cand_hull'].cpu().numpy(), MARGIN, UNION)
    print('stage: kept %s, count %s of %d candidates (n_out %d)' % (ref_keep.sum(1).tolist(), ref[4].tolist(), 2 * UNION, UNION))
    assert (ref[4] >= UNION).all()                                     # padding cannot hide a filter that rejects too much
    assert (ref[4] < 2 * UNION).all()                                  # ... and the objects do overlap
    _assert_union([parts[k] for k in ('support', 'outside')] + [parts['cloud'], parts['src'], parts['count']], ref)
    # RGBA is PhongRenderer.render and triangle_alpha, mesh by mesh and view by view
    cams = draws['cams'].cpu()
    for s in range(S):
        mesh = TriangleMesh.from_tensors(verts[s], faces)
        for v in range(V):
            dist, elev, azim = (float(x) for x in cams[s, v])
            rgb, _alpha, _n = PhongRenderer.render(mesh, dist, elev, azim, uv[s:s + 1], texture[s:s + 1], img_size=SIZE)
            alpha, _ = VertexRenderer.triangle_alpha(mesh, dist, elev, azim, SIZE, SIZE)
            assert torch.equal(rgba[s, v, :3], rgb[0].permute(2, 0, 1)) and torch.equal(rgba[s, v, 3], alpha[0])
            want = vpn_amd.obj_to_view_points(verts[s:s + 1], draws['cams'][s, v:v + 1, 0].contiguous(), draws['cams'][s, v:v + 1, 1].contiguous(),
                                              draws['cams'][s, v:v + 1, 2].contiguous())
            assert torch.equal(centred[s, v], want[0])
    # every ground-truth point is the barycentric combination of its recorded face of the view-centred mesh
    vv = centred.reshape(S * V, P, 3).cpu().double()
    f = faces.cpu().long()
    fi, w = parts['face_idx'].reshape(S * V, NEW).cpu().long(), parts['bary'].reshape(S * V, NEW, 3).cpu().double()
    assert int(fi.min()) >= 0 and int(fi.max()) < f.shape[0]
    assert float(w.min()) >= 0.0 and float((w.sum(-1) - 1).abs().max()) <= 4 * 2.0 ** -24
    corners = torch.stack([vv[b][f[fi[b]]] for b in range(S * V)])
    terms = w[..., None] * corners
    err = (gt_points.reshape(S * V, NEW, 3).cpu().double() - terms.sum(2)).abs()
    u = 2.0 ** -24
    bound = 3 * u / (1 - 3 * u) * terms.abs().sum(2)
    print('gt points: max |point - combination| %.3e, largest bound %.3e' % (float(err.max()), float(bound.max())))
    assert bool((err <= bound).all())
    # all draws given: the call repeats itself bit for bit
    again = _stage()
    assert all(torch.equal(x, y) for x, y in zip(again, (rgba, centred, gt_points, dists, elevs, azims)))


def test_default_draws_follow_the_seed_in_the_stated_order():
    import vpn_amd
    from vpn_amd.modules import augmentation as A
    p1, p2, _ = _inputs()
    kw = dict(views=V, img_size=SIZE, num_points=64, union_points=256)
    torch.manual_seed(31)
    a = vpn_amd.acd_mix_data(p1, p2, **kw)
    torch.manual_seed(31)
    b = vpn_amd.acd_mix_data(p1, p2, **kw)
    torch.manual_seed(32)
    c = vpn_amd.acd_mix_data(p1, p2, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[3], c[3])
    dists, elevs, azims = a[3:]
    assert 3.0 <= float(dists.min()) and float(dists.max()) <= 5.0 and -45.0 <= float(elevs.min()) and float(elevs.max()) <= 45.0
    assert 0.0 <= float(azims.min()) and float(azims.max()) <= 360.0                       # generate.py:153-155
    torch.manual_seed(31)
    d = A._augment_draws(S, 2, HULLS, None, None, None, None, None, None)                  # acd.py:114-119, object after object
    colors = torch.stack([torch.rand(3) for _ in range(S * HULLS)]).reshape(S, HULLS, 3)   # one colour per hull, mesh after mesh
    cams = []
    for _ in range(S * V):                                                                 # generate.py:153-155, view after view
        cams.append((3.0 + torch.rand(1).item() * 2, (torch.rand(1).item() - 0.5) * 90, torch.rand(1).item() * 360))
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    gt_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    e = vpn_amd.acd_mix_data(p1, p2, colors=colors, cams=torch.tensor(cams, dtype=torch.float32).reshape(S, V, 3), seed=seed, gt_seed=gt_seed,
                             **d, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, e))


def test_stage_makes_no_host_synchronisation():
    want = _stage()                                                    # warm-up: code objects, cached constants
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = _stage()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_stage_captured_into_a_graph_replays_the_eager_bytes():
    want = _stage()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = _stage()
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, want))
