"""CPU checks of the cloud -> mesh step: the properties of the specification on its numpy restatement
(tests/reconstruct_ref.py), the C ABI entries, and the reference's names in modules/augmentation.py.  No GPU call is made."""
import ctypes
import functools
import inspect

import numpy as np
import pytest
import torch

import reconstruct_ref as RR

H, ITERS = 5, 4


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == 'lattice':
        pts, dirs = RR.lattice_cloud(6)[None], RR.AXIS_DIRS
    else:
        pts = (np.random.default_rng(7).random((2, 301, 3), dtype=np.float32) - np.float32(0.5))
        dirs = RR.random_dirs(37, seed=1)
    lab, cen, cnt = RR.cluster_points(pts, H, ITERS)
    verts, sup = RR.support_hulls(pts, lab, cen, dirs)
    return pts, dirs, lab, cen, cnt, verts, sup


@pytest.mark.parametrize('name', ['lattice', 'random'])
def test_restatement_properties(name):
    pts, dirs, lab, cen, cnt, verts, sup = _case(name)
    B, n, _ = pts.shape
    D = dirs.shape[0]
    assert lab.dtype == np.int32 and lab.shape == (B, n) and lab.min() >= 0 and lab.max() < H      # labels partition the cloud
    assert cnt.dtype == np.int32 and (cnt.sum(1) == n).all()
    for b in range(B):
        assert np.array_equal(np.bincount(lab[b], minlength=H), cnt[b])
        for h in range(H):
            members = np.nonzero(lab[b] == h)[0]
            s = sup[b, h * D:(h + 1) * D]
            v = verts[b, h * D:(h + 1) * D]
            if members.size == 0:
                assert (s == -1).all() and (v == cen[b, h]).all()
                continue
            assert np.isin(s, members).all()                           # a cloud point of the right cluster
            assert np.array_equal(v, pts[b, s])
            val = pts[b, members].astype(np.float64) @ dirs.astype(np.float64).T          # [m,D] in fp64
            chosen = np.einsum('dk,dk->d', pts[b, s].astype(np.float64), dirs.astype(np.float64))
            assert float((val.max(0) - chosen).max()) <= 1e-6          # no member exceeds the chosen support value
    assert np.isfinite(cen).all()


def test_lattice_ties_go_to_the_lowest_index():
    pts, dirs, lab, cen, cnt, verts, sup = _case('lattice')
    D = dirs.shape[0]
    ties = 0
    for h in range(H):
        members = np.nonzero(lab[0] == h)[0]
        val = RR.dot(pts[0, members][:, None, :], dirs[None])
        for d in range(D):
            top = members[val[:, d] == val[:, d].max()]
            ties += top.size > 1
            assert sup[0, h * D + d] == top.min()
    assert ties >= 10                                                  # the lattice does produce equal support values


def test_atlas_rule():
    uv, tex = RR.atlas(4, 3, [[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.7, 0.8, 0.9], [1.0, 0.0, 0.5]])
    assert uv.shape == (12, 2) and tex.shape == (3, 1, 4)
    assert np.array_equal(uv[:, 0], uv[:, 1]) and np.array_equal(uv[3:6, 0], np.full(3, np.float32(1 / 4 + 0.01)))
    assert np.array_equal(tex[:, 0, 1], np.array([0.4, 0.5, 0.6], np.float32))
    from vpn_amd.modules import augmentation as A
    got_uv = A._atlas_uv(2, 4, 3, 'cpu')
    assert np.array_equal(got_uv[1].numpy(), uv)
    colors = torch.rand(2, 4, 3)
    got_tex = A._atlas_texture(2, 4, colors, 'cpu')
    assert got_tex.shape == (2, 3, 1, 4) and np.array_equal(got_tex[1].numpy(), RR.atlas(4, 3, colors[1].numpy())[1])
    torch.manual_seed(5)
    drawn = A._atlas_texture(2, 4, None, 'cpu')
    torch.manual_seed(5)
    want = torch.stack([torch.rand(3) for _ in range(8)]).reshape(2, 4, 3)            # merge_meshes' draws, mesh after mesh
    assert torch.equal(drawn, want.permute(0, 2, 1)[:, :, None, :])
    f = RR.hull_faces([[0, 1, 2]], 3, 3)
    assert f.dtype == np.int32 and f.tolist() == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]


def test_hull_template_is_the_uv_sphere_repeated():
    from vpn_amd import ops
    from vpn_amd.modules.meshing import uv_sphere
    v, f = uv_sphere()
    dirs, faces = ops.hull_template(3, 'cpu')
    assert dirs.shape == (128, 3) and faces.shape == (3 * f.shape[0], 3) and faces.dtype == torch.int32
    assert torch.equal(dirs, v / v.norm(dim=1, keepdim=True))
    assert np.array_equal(faces.numpy(), RR.hull_faces(f.numpy(), 3, 128))
    assert ops.hull_template(3, 'cpu')[1] is faces                     # uploaded once, found again


def test_entries_are_bound_and_exported():
    import vpn_amd._lib as lib
    L = lib.lib()
    for name in ('vpn_cluster_points', 'vpn_support_hulls'):
        assert name in lib.SIGNATURES and hasattr(ctypes.CDLL(lib.LIB_PATH), name)
    assert L.vpn_abi_version() == 9                                    # entries added, none changed
    assert L.vpn_cluster_points(None, 1, 8, 2, 1, None, None, None, None) == -1
    assert L.vpn_support_hulls(None, None, None, None, 1, 8, 2, 4, None, None, None) == -1
    one = ctypes.c_void_p(16)                                          # never dereferenced: the size checks come first
    assert L.vpn_cluster_points(one, 1, 8193, 2, 1, one, one, one, None) == -2
    assert L.vpn_cluster_points(one, 1, 8, 33, 1, one, one, one, None) == -2
    assert L.vpn_support_hulls(one, one, one, one, 1, 8193, 2, 4, one, one, None) == -2
    assert L.vpn_support_hulls(one, one, one, one, 1, 8, 33, 4, one, one, None) == -2


def test_reference_names_and_positional_parameters():
    import vpn_amd
    from vpn_amd.modules import augmentation as A
    sig = inspect.signature

    def positional(fn):
        return [p.name for p in sig(fn).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]

    assert positional(A.point_mixup_data) == ['view_center_points']                    # point_mixup.py:12
    assert positional(A.generate_point_mixup_data) == ['view_center_points']           # :78
    assert positional(A.points_to_meshes_and_colors) == ['points']                     # :43
    assert positional(A.points_to_mesh_batch) == ['points']
    assert positional(A.meshes_to_imgs) == ['meshes', 'uvs', 'textures']               # :58
    assert positional(A.check_parameters) == ['view_center_points']                    # :73
    for kw in ('ratio', 'indices', 'colors', 'seed', 'sample_base'):
        assert sig(A.point_mixup_data).parameters[kw].kind == inspect.Parameter.KEYWORD_ONLY
    assert sig(A.points_to_meshes_and_colors).parameters['iters'].default == 8
    assert vpn_amd.config.DECOMPOSE_CONVEX_NUM == 16
    for name in ('point_mixup_data', 'generate_point_mixup_data', 'points_to_meshes_and_colors', 'meshes_to_imgs',
                 'cluster_points', 'support_hulls', 'hull_meshes'):
        assert callable(getattr(vpn_amd, name))
    with pytest.raises(AssertionError):
        A.check_parameters(torch.rand(4, 3))
    with pytest.raises(RuntimeError, match='GPU only'):                # no CPU path
        vpn_amd.hull_meshes(torch.rand(1, 16, 3), 2)
    with pytest.raises(RuntimeError, match='gradients'):               # data only
        vpn_amd.hull_meshes(torch.rand(1, 16, 3, requires_grad=True), 2)
    with pytest.raises(ValueError, match='support_hulls'):             # shapes are checked before anything is unpacked
        vpn_amd.support_hulls(torch.rand(16, 3), torch.zeros(16, dtype=torch.int32), torch.rand(1, 2, 3), torch.rand(4, 3))
    uv = A._atlas_uv(3, 2, 4, 'cpu')
    assert uv.shape == (3, 8, 2) and uv.stride(0) == 0                 # one constant, visibly shared over the batch
