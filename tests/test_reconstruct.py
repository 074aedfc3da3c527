"""GPU checks of the cloud -> mesh step (csrc/reconstruct.hip, ops.hull_meshes, modules/augmentation.py).

The kernels against tests/reconstruct_ref.py: labels, counts, centres, support and verts are compared with torch.equal /
np.array_equal -- every decision of the specification is an arg-max with a tie rule and every centre an exact integer
mean, so there is no tolerance to choose.  The one bound in this file is for the re-sampled points: the sampler
(csrc/mesh.hip) evaluates w0 a + w1 b + w2 c in fp32, with or without fused multiply-adds; either way the result is
within gamma_3 (sum_k |w_k v_k|), gamma_3 = 3 u / (1 - 3 u), u = 2^-24, of the exact combination of the same fp32 weights
and vertices (three roundings at most on the way of any term: the standard bound of a length-3 inner product), and that is
what is asserted.  'max' is both limits of the kernels at once (n = 8192, H = 32: 128 KiB of LDS, above the default limit)."""
import functools

import numpy as np
import pytest
import torch

import reconstruct_ref as RR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ITERS = 8


def _cloud(B, n, seed):
    return np.random.default_rng(seed).random((B, n, 3), dtype=np.float32) - np.float32(0.5)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(points, dirs, H) of a named input and the restatement's outputs, computed once."""
    if name == 'identical':                        # 8 copies of one point, H = 4: clusters 1..3 stay empty
        pts, H, dirs = np.tile(np.array([[[0.25, -0.125, 0.5]]], np.float32), (1, 8, 1)), 4, RR.random_dirs(114, 3)
    elif name == 'lattice':                        # exact ties in distances and support values
        pts, H, dirs = RR.lattice_cloud(6)[None], 5, RR.AXIS_DIRS
    elif name == 'few':                            # n < H
        pts, H, dirs = _cloud(2, 5, 11), 8, RR.random_dirs(114, 3)
    else:
        B, n, H, D = {'a': (1, 100, 3, 114), 'b': (3, 257, 16, 114), 'c': (2, 2048, 16, 114), 'max': (1, 8192, 32, 114),
                      'one': (2, 130, 1, 114)}[name]
        pts, dirs = _cloud(B, n, 5 + n), RR.random_dirs(D, 3)
    lab, cen, cnt = RR.cluster_points(pts, H, ITERS)
    verts, sup = RR.support_hulls(pts, lab, cen, dirs)
    return pts, dirs, H, lab, cen, cnt, verts, sup


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'max', 'one', 'few', 'identical', 'lattice'])
def test_kernels_equal_the_restatement_bit_for_bit(name):
    from vpn_amd import ops
    pts, dirs, H, lab, cen, cnt, verts, sup = _case(name)
    p = torch.from_numpy(pts).to(DEV)
    g_lab, g_cen, g_cnt = ops.cluster_points(p, H, ITERS)
    g_verts, g_sup = ops.support_hulls(p, g_lab, g_cen, torch.from_numpy(dirs).to(DEV))
    print('%s: counts %s' % (name, g_cnt.cpu().tolist()))
    assert g_lab.dtype == torch.int32 and g_cnt.dtype == torch.int32 and g_sup.dtype == torch.int32
    assert np.array_equal(g_cnt.cpu().numpy(), cnt)
    assert np.array_equal(g_lab.cpu().numpy(), lab)
    assert np.array_equal(g_cen.cpu().numpy().view(np.int32), cen.view(np.int32))
    assert np.array_equal(g_sup.cpu().numpy(), sup)
    assert np.array_equal(g_verts.cpu().numpy().view(np.int32), verts.view(np.int32))
    if name == 'identical':
        D = dirs.shape[0]
        assert cnt.tolist() == [[8, 0, 0, 0]] and (sup[0, D:] == -1).all() and (sup[0, :D] == 0).all()
        assert (g_verts.cpu().numpy()[0] == pts[0, 0]).all()           # the centre of an empty cluster is its seed
    if name == 'few':
        assert (cnt <= 1).sum() == cnt.size and (sup == -1).any()


def test_zero_lloyd_rounds_and_the_default_template():
    from vpn_amd import ops
    pts = _cloud(2, 200, 21)
    lab, cen, cnt = RR.cluster_points(pts, 4, 0)
    p = torch.from_numpy(pts).to(DEV)
    g = ops.cluster_points(p, 4, 0)
    assert np.array_equal(g[0].cpu().numpy(), lab) and np.array_equal(g[1].cpu().numpy(), cen) and np.array_equal(g[2].cpu().numpy(), cnt)
    verts, faces, labels, support = ops.hull_meshes(p, 4, ITERS)
    dirs, want_faces = ops.hull_template(4, 'cpu')
    lab, cen, cnt = RR.cluster_points(pts, 4, ITERS)
    want_verts, want_sup = RR.support_hulls(pts, lab, cen, dirs.numpy())
    assert verts.shape == (2, 4 * 128, 3) and faces.shape == (4 * 252, 3) and faces.dtype == torch.int32 and faces.is_cuda
    assert torch.equal(faces.cpu(), want_faces) and np.array_equal(labels.cpu().numpy(), lab)
    assert np.array_equal(support.cpu().numpy(), want_sup) and np.array_equal(verts.cpu().numpy(), want_verts)
    assert ops.hull_meshes(p, 4, ITERS)[1] is faces                    # one upload


def test_oversize_is_refused_before_any_launch():
    from vpn_amd import ops
    dirs = torch.from_numpy(RR.random_dirs(8, 0)).to(DEV)
    big = torch.zeros(1, 8193, 3, device=DEV)
    with pytest.raises(RuntimeError, match=r'code -2'):
        ops.cluster_points(big, 4)
    with pytest.raises(RuntimeError, match=r'code -2'):
        ops.cluster_points(big[:, :64], 33)
    with pytest.raises(RuntimeError, match=r'code -2'):
        ops.support_hulls(big, torch.zeros(1, 8193, dtype=torch.int32, device=DEV), torch.zeros(1, 4, 3, device=DEV), dirs)
    with pytest.raises(RuntimeError, match=r'code -2'):
        ops.support_hulls(big[:, :64], torch.zeros(1, 64, dtype=torch.int32, device=DEV), torch.zeros(1, 33, 3, device=DEV), dirs)
    torch.cuda.synchronize()


B, N, HULLS, SIZE, NEW = 3, 256, 4, 32, 2048


@functools.lru_cache(maxsize=None)
def _batch():
    from vpn_amd import ops
    g = torch.Generator().manual_seed(9)
    pts = (torch.rand(B, N, 3, generator=g) - 0.5).to(DEV) * 0.6
    idx = ops.partner_indices(torch.tensor([1, 2, 0]), B, DEV)
    colors = torch.rand(B, HULLS, 3, generator=g).to(DEV)
    torch.cuda.synchronize()
    return pts, idx, colors


def _stage(**kw):
    import vpn_amd
    pts, idx, colors = _batch()
    return vpn_amd.point_mixup_data(pts, ratio=0.4, indices=idx, colors=colors, seed=77, hull_num=HULLS, img_size=SIZE,
                                    num_points=NEW, **kw)


def test_meshes_to_imgs_equals_the_per_mesh_renders():
    import vpn_amd
    from vpn_amd import PhongRenderer, VertexRenderer
    pts, _idx, colors = _batch()
    meshes, uvs, textures = vpn_amd.points_to_meshes_and_colors(pts, hull_num=HULLS, colors=colors)
    assert len(meshes) == len(uvs) == len(textures) == B
    assert uvs[0].shape == (1, HULLS * 128, 2) and textures[0].shape == (1, 3, 1, HULLS)
    uv_ref, tex_ref = RR.atlas(HULLS, 128, colors[1].cpu().numpy())
    assert np.array_equal(uvs[1][0].cpu().numpy(), uv_ref) and np.array_equal(textures[1][0].cpu().numpy(), tex_ref)
    rgbs, sils = vpn_amd.meshes_to_imgs(meshes, uvs, textures, img_size=SIZE)
    assert rgbs.shape == (B, 3, SIZE, SIZE) and sils.shape == (B, 1, SIZE, SIZE)
    for b in range(B):
        rgb, _alpha, _n = PhongRenderer.render(meshes[b], 1, 0, 0, uvs[b], textures[b], img_size=SIZE)
        alpha, _ = VertexRenderer.triangle_alpha(meshes[b], 1, 0, 0, SIZE, SIZE)
        assert torch.equal(rgbs[b], rgb[0].permute(2, 0, 1)) and torch.equal(sils[b, 0], alpha[0])
        assert torch.equal(_alpha[0, ..., 0], alpha[0])
    assert float(sils.max()) > 0.5 and float(rgbs.max()) > 0.0         # the meshes are in the picture
    # mixed topologies: the per-mesh loop, the same pictures
    other, ouv, otex = vpn_amd.points_to_meshes_and_colors(pts[:1], hull_num=2, colors=colors[:1, :2])
    r2, s2 = vpn_amd.meshes_to_imgs(meshes[:2] + other, uvs[:2] + ouv, textures[:2] + otex, img_size=SIZE)
    assert r2.shape == (3, 3, SIZE, SIZE) and torch.equal(r2[:2], rgbs[:2]) and torch.equal(s2[:2], sils[:2])


def test_point_mixup_data():
    import vpn_amd
    rgbs, sils, new_points, parts = _stage(return_parts=True)
    assert rgbs.shape == (B, 3, SIZE, SIZE) and sils.shape == (B, 1, SIZE, SIZE) and new_points.shape == (B, NEW, 3)
    assert rgbs.dtype == sils.dtype == new_points.dtype == torch.float32
    assert not (rgbs.requires_grad or sils.requires_grad or new_points.requires_grad)
    assert float(rgbs.min()) >= 0.0 and float(rgbs.max()) <= 1.0 and float(sils.min()) >= 0.0 and float(sils.max()) <= 1.0
    # the stage is its parts: mix-up, hulls, atlas
    pts, idx, colors = _batch()
    mixed = vpn_amd.mixup_points(pts, ratio=0.4, indices=idx)
    assert torch.equal(parts['mixed'], mixed)
    verts, faces, labels, support = vpn_amd.hull_meshes(mixed, HULLS)
    assert torch.equal(parts['verts'], verts) and torch.equal(parts['support'], support) and parts['faces'] is faces
    lab, cen, _cnt = RR.cluster_points(mixed.cpu().numpy(), HULLS, ITERS)
    assert np.array_equal(labels.cpu().numpy(), lab)
    # every new point is the barycentric combination of its recorded face (bound: the module text)
    v = verts.cpu().double()
    f = faces.cpu().long()
    fi, w = parts['face_idx'].cpu().long(), parts['bary'].cpu().double()
    assert int(fi.min()) >= 0 and int(fi.max()) < f.shape[0]
    assert float(w.min()) >= 0.0 and float((w.sum(-1) - 1).abs().max()) <= 4 * 2.0 ** -24
    corners = torch.stack([v[b][f[fi[b]]] for b in range(B)])          # [B,NEW,3 corners,3]
    terms = w[..., None] * corners
    err = (new_points.cpu().double() - terms.sum(2)).abs()
    u = 2.0 ** -24
    bound = 3 * u / (1 - 3 * u) * terms.abs().sum(2)
    print('new points: max |point - combination| %.3e, largest bound %.3e' % (float(err.max()), float(bound.max())))
    assert bool((err <= bound).all())
    # all draws given: the call repeats itself bit for bit
    again = _stage()
    assert torch.equal(again[0], rgbs) and torch.equal(again[1], sils) and torch.equal(again[2], new_points)
    # the defaults follow torch.manual_seed, and another seed draws otherwise
    kw = dict(hull_num=HULLS, img_size=SIZE, num_points=64)
    torch.manual_seed(31)
    a = vpn_amd.point_mixup_data(pts, **kw)
    torch.manual_seed(31)
    b = vpn_amd.point_mixup_data(pts, **kw)
    torch.manual_seed(32)
    c = vpn_amd.point_mixup_data(pts, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[2], c[2])
    # ... in the reference's order: ratio, partners, one colour per hull mesh after mesh, then the key of the surface samples
    torch.manual_seed(31)
    ratio, perm = torch.rand(1).item(), torch.randperm(B)
    cols = torch.stack([torch.rand(3) for _ in range(B * HULLS)]).reshape(B, HULLS, 3)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    d = vpn_amd.point_mixup_data(pts, ratio=ratio, indices=perm, colors=cols, seed=seed, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, d))
    # the data-set form: the same pictures and the meshes themselves
    r, s, meshes = vpn_amd.generate_point_mixup_data(pts, ratio=0.4, indices=idx, colors=colors, hull_num=HULLS, img_size=SIZE)
    assert torch.equal(r, rgbs) and torch.equal(s, sils) and len(meshes) == B
    assert torch.equal(meshes[2].vertices, verts[2]) and meshes[0].faces is faces


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
