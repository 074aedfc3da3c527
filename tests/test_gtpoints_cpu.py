"""The ground-truth stage without a GPU: the host half of MeshBatch, the numpy restatement
(tests/gtpoints_ref.py) against the oracle's mesh_sample and against what a surface sampler must do, the transforms of
dataset.py:168-184 and genre.py:69-73, and the argument validation of vpn_ragged_sample.  kaolin is absent, so parity with
TriangleMesh.sample stays unpinned, as tests/test_mesh_path.py notes."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gtpoints_ref as R
from conftest import ROOT
from oracle import vpn_oracle as O


def _dataset():
    from vpn_amd.modules import dataset
    return dataset


def _face_counts(chunk):
    return [1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 5]


def test_pack_offsets_and_chunks_tile_every_mesh_in_order():
    D = _dataset()
    counts = _face_counts(D.CHUNK)
    vcounts = [3, 700, 5, 129, 64, 2000, 17, 333]                      # unrelated to the face counts
    g = torch.Generator().manual_seed(0)
    meshes = [(torch.rand(p, 3, generator=g), torch.randint(0, p, (f, 3), generator=g)) for p, f in zip(vcounts, counts)]
    b = D.MeshBatch.pack(meshes)                                       # no device: the host half alone
    assert b.verts is None and b.device is None and len(b) == 8
    h = b.host
    assert h['vert_offset'].tolist() == np.concatenate([[0], np.cumsum(vcounts)]).tolist()
    assert h['face_offset'].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert h['verts'].dtype == torch.float32 and h['faces'].dtype == torch.int32
    assert all(h[k].dtype == torch.int32 for k in ('vert_offset', 'face_offset', 'chunk_offset', 'chunks'))
    for s, (v, f) in enumerate(meshes):                                # packed as they came, indices mesh-local
        assert torch.equal(h['verts'][h['vert_offset'][s]:h['vert_offset'][s + 1]], v)
        assert torch.equal(h['faces'][h['face_offset'][s]:h['face_offset'][s + 1]].long(), f)
    chunks, coff = h['chunks'].tolist(), h['chunk_offset'].tolist()
    assert coff[0] == 0 and coff[-1] == len(chunks) and len(coff) == 9
    nxt = 0
    for s in range(8):
        rows = chunks[coff[s]:coff[s + 1]]
        assert len(rows) == -(-counts[s] // D.CHUNK)
        for mesh, first, count in rows:
            assert mesh == s and first == nxt and 1 <= count <= D.CHUNK
            assert h['face_offset'][s] <= first and first + count <= h['face_offset'][s + 1]          # never straddles
            nxt += count
        assert nxt == h['face_offset'][s + 1]                          # tiled exactly once, in order
    assert D.CHUNK == int(__import__('re').search(r'#define\s+VPN_RAGGED_CHUNK\s+(\d+)',
                                                  open(os.path.join(ROOT, 'include', 'vpn_hip.h')).read()).group(1))


def test_pack_accepts_triangle_meshes_and_obj_files(tmp_path):
    import vpn_amd
    v, f = R.icosphere(0)
    obj = tmp_path / 'm.obj'
    vpn_amd.TriangleMesh(v, f).save_mesh(str(obj))
    a = vpn_amd.MeshBatch.pack([vpn_amd.TriangleMesh(v, f), (v.numpy(), f.tolist())])
    b = vpn_amd.MeshBatch.from_objs([str(obj), str(obj)])
    for k in vpn_amd.MeshBatch.FIELDS:
        assert torch.equal(a.host[k], b.host[k]), k
    assert a.face_counts == [20, 20] and a.vert_counts == [12, 12]


def test_pack_rejects_empty_meshes_by_index():
    D = _dataset()
    v, f = R.icosphere(0)
    with pytest.raises(ValueError, match='mesh 1 has no faces'):
        D.MeshBatch.pack([(v, f), (v, torch.zeros(0, 3, dtype=torch.int64)), (v, f)])
    with pytest.raises(ValueError, match='mesh 2 has no vertices'):
        D.MeshBatch.pack([(v, f), (v, f), (torch.zeros(0, 3), f)])
    with pytest.raises(ValueError):
        D.MeshBatch.pack([])


def test_sampling_needs_a_device_batch():
    D = _dataset()
    b = D.MeshBatch.pack([R.icosphere(0)])
    with pytest.raises(RuntimeError, match='GPU only'):
        D.sample_gt_points(b, 8)


STRETCH = (1.0, 0.3, 2.0)


def test_restatement_equals_the_oracle_sampler():
    v, f = R.icosphere(1, 1.0, STRETCH)
    n = 4000
    u = O.philox_uniforms_mesh(11, 5, n)
    assert np.array_equal(R.uniforms(11, 5, 0, n), u.numpy())          # set 0 draws the existing sampler's stream
    pts, idx = O.mesh_sample(v, f, u)
    # precondition: on these draws the oracle's fp32 running sum chooses what a float64 running sum of ITS areas chooses
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * torch.cross(b - a, c - a, dim=1).norm(dim=1).float()
    cdf64 = torch.cumsum(area.double(), 0).float()
    idx64 = torch.searchsorted(cdf64, u[:, 0] * cdf64[-1], right=True).clamp_max(f.shape[0] - 1)
    assert torch.equal(idx, idx64)
    face, bary, p = R.sample(v.numpy(), f.numpy(), u.numpy())
    assert np.array_equal(face, idx.numpy())
    assert float(np.abs(p - pts.numpy()).max()) <= 1e-6
    assert float(np.abs(bary.sum(1) - 1).max()) <= 2e-7


def test_restatement_is_uniform_on_the_surface():
    v, f = R.icosphere(1, 1.0, STRETCH)
    n = 20000
    face, _, p = R.sample(v.numpy(), f.numpy(), R.uniforms(7, 3, 1, n))
    area = R.face_areas(v.numpy(), f.numpy()).astype(np.float64)
    share = area / area.sum()
    got = np.bincount(face, minlength=len(area)) / n
    sigma = np.sqrt(share * (1 - share) / n)
    assert float((np.abs(got - share) / sigma).max()) < 4.0            # the criterion of test_oracle_mesh_sample_is_uniform_on_the_surface
    a, b, c = R.corners(v.numpy(), f.numpy())
    nrm = np.cross(b - a, c - a)[face]
    assert float(np.abs(((p - a[face]) * nrm).sum(1)).max()) < 1e-5    # every point lies in the plane of its face


def test_zero_area_faces_are_never_chosen():
    v, f = R.icosphere(0, 1.0, STRETCH)
    flat = torch.tensor([[0, 0, 1], [2, 2, 2], [3, 4, 3]])             # repeated corners: no area
    rows, zero = [], []
    for i, tri in enumerate(f.tolist()):                               # a flat face before every real one, two at the end
        zero.append(len(rows))
        rows += [flat[i % 3].tolist(), tri]
    zero += [len(rows), len(rows) + 1]
    rows += [flat[0].tolist(), flat[1].tolist()]
    faces = np.array(rows, np.int64)
    areas = R.face_areas(v.numpy(), faces)
    assert zero[0] == 0 and zero[-1] == len(faces) - 1 and not areas[zero].any() and (np.delete(areas, zero) > 0).all()
    u0 = np.arange(1024, dtype=np.float32) / np.float32(1024)
    chosen = R.choose_faces(R.cumulative_areas(areas), u0)
    assert not np.isin(chosen, zero).any()
    assert chosen[0] == 1 and chosen[-1] == len(faces) - 3             # the first and the last face with area


def _apply(m, p):
    return torch.einsum('sij,snj->sni', m[:, :, :3], p) + m[:, None, :, 3]


def test_view_center_xforms_equal_obj_to_view_points():
    D = _dataset()
    g = torch.Generator().manual_seed(3)
    S = 6
    dists = 0.7 + torch.rand(S, generator=g)
    elevs, azims = 60 * torch.rand(S, generator=g) - 30, 360 * torch.rand(S, generator=g)
    p = torch.rand(S, 100, 3, generator=g) - 0.5
    m = D.view_center_xforms(dists, elevs, azims)
    assert m.shape == (S, 3, 4) and m.dtype == torch.float32 and not m[:, :, 3].any()
    assert float((_apply(m, p) - O.obj_to_view_points(p, dists, elevs, azims)).abs().max()) <= 1e-6
    same = D.view_center_xforms(dists.tolist(), elevs.tolist(), azims.tolist())       # host numbers
    assert float((same - m).abs().max()) <= 1e-6
    inv = D.view_center_xforms(dists, elevs, azims, dist_invariant=True)             # dataset.py:45-46: scale 1
    gram = torch.bmm(inv[:, :, :3], inv[:, :, :3].transpose(1, 2))
    assert float((gram - torch.eye(3)).abs().max()) <= 1e-6
    assert float((inv[:, :, :3] - m[:, :, :3] * dists[:, None, None]).abs().max()) <= 1e-6


def test_genre_xforms_equal_the_normalisation_written_out():
    D = _dataset()
    g = torch.Generator().manual_seed(4)
    meshes = [(128 * torch.rand(p, 3, generator=g), torch.randint(0, p, (7, 3), generator=g)) for p in (50, 3, 211)]
    m = D.genre_xforms(D.MeshBatch.pack(meshes))
    assert m.shape == (3, 3, 4) and m.dtype == torch.float32
    for s, (v, _) in enumerate(meshes):
        w = v.clone()                                                  # genre.py:69-73
        w -= torch.mean(w, 0)
        w /= 128
        w = w[:, [0, 2, 1]]
        w[:, 0] *= -1
        w /= 1.7
        assert float((_apply(m[s:s + 1], v[None])[0] - w).abs().max()) <= 1e-6


def test_ragged_sample_rejects_bad_arguments_before_any_launch():
    """Every call below carries exactly one bad argument and must return before anything is launched: the pointers are
    made-up addresses that no kernel may ever see."""
    lib_path = os.path.join(ROOT, 'volumetric-primitives-net_amd', 'libvpn_hip.so')
    try:
        import vpn_amd._lib as lib
        L = lib.lib()
    except (OSError, RuntimeError) as e:                               # pragma: no cover
        pytest.skip('libvpn_hip.so does not load here (%s): %s' % (lib_path, e))
    S, T, n, sumP, sumF, C = 2, 2, 16, 10, 2000, 3
    need = L.vpn_ragged_sample_workspace(sumF, C, S)
    assert need % 16 == 0 and need >= 8 * sumF + 8 * C + 4 * S
    assert L.vpn_ragged_sample_workspace(0, C, S) == 0 and L.vpn_ragged_sample_workspace(sumF, 0, S) == 0
    assert L.vpn_ragged_sample_workspace(sumF, C, 0) == 0
    P = ctypes.c_void_p(0x1000)
    good = dict(verts=P, faces=P, vert_offset=P, face_offset=P, chunk_offset=P, chunks=P, xforms=None, xform_mask=0, u=None,
                seed=1, seed_dev=None, mesh_base=0, S=S, T=T, n=n, sumP=sumP, sumF=sumF, C=C, workspace=P,
                workspace_bytes=need, points=P, face_idx=None, bary=None, stream=None)

    def rc(**bad):
        assert len(bad) == 1
        return L.vpn_ragged_sample(*{**good, **bad}.values())
    for name in ('verts', 'faces', 'vert_offset', 'face_offset', 'chunk_offset', 'chunks', 'workspace', 'points'):
        assert rc(**{name: None}) == -1, name
    for name in ('S', 'T', 'n', 'sumP', 'sumF', 'C'):
        assert rc(**{name: 0}) == -1 and rc(**{name: -3}) == -1, name
    assert rc(T=17) == -2                                              # VPN_RAGGED_MAX_SETS
    assert rc(S=40000) == -2                                           # S * T beyond the grid's second dimension
    assert rc(sumP=0x7fffffff // 3 + 1) == -2 and rc(sumF=0x7fffffff // 3 + 1) == -2        # int32 index range
    assert rc(C=sumF + 1) == -1                                        # more chunks than faces
    assert rc(workspace=ctypes.c_void_p(0x1008)) == -1                 # not 16-byte aligned
    assert rc(workspace_bytes=need - 1) == -1


def test_kernels_use_no_scratch_and_little_lds():
    """The budget DESIGN.md 4.15 quotes: compiled the way build.py compiles gtpoints.hip."""
    import importlib.util
    import re
    import subprocess
    spec = importlib.util.spec_from_file_location('vpn_build', os.path.join(ROOT, 'volumetric-primitives-net_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert 'gtpoints.hip' in b.SOURCES and '-ffp-contract=off' in b.PER_FILE['gtpoints.hip']
    cmd = [b.hipcc()] + b.COMMON + b.PER_FILE['gtpoints.hip'] + ['-c', os.path.join(b.CSRC, 'gtpoints.hip'), '-o', os.devnull,
                                                                 '-Rpass-analysis=kernel-resource-usage']
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'warning' not in out.stderr, out.stderr
    rows, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r'remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\S+)', line)
        if m and m.group(1) == 'Function Name':
            cur = rows.setdefault(m.group(2), {})
        elif m and cur is not None:
            cur[m.group(1).split(' ')[0]] = int(m.group(2))
    kernels = {k: v for k, v in rows.items() if 'ragged_' in k}
    assert len(kernels) == 3, list(rows)
    for name, r in kernels.items():
        assert r['ScratchSize'] == 0 and r['LDS'] <= 64 and r['VGPRs'] <= 128, (name, r)
