"""GPU checks of the ground-truth stage (modules/dataset.py::MeshBatch / sample_gt_points / gt_points, csrc/gtpoints.hip;
DESIGN.md 4.15).  Every comparison with tests/gtpoints_ref.py is exact (torch.equal), with no share of excused draws: the
meshes are built so that float64 sums of their fp32 areas are exact in any order (asserted on the CPU before the GPU is
touched), so the chunked scan of the kernels and the sequential sum of the restatement hold the same table.  The optional
seed_dev counter form is implemented and tested here."""
import numpy as np
import pytest
import torch

import gtpoints_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N_MAX, T_MAX, SEED, BASE = 257, 2, 2024, 5


def _counts():
    from vpn_amd.modules.dataset import CHUNK
    return [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]


def _mesh(F, extra, stretch, flat_every=97):
    """F faces cut from a stretched icosphere's face list (repeated as often as needed), every flat_every-th one collapsed
    to no area (also the first and the last one when F allows), `extra` unused vertices in front so that P is unrelated to F."""
    v, f = R.icosphere(3, 0.4, stretch)
    f = f.repeat(-(-F // f.shape[0]), 1)[:F].clone()
    if F > 2:
        f[flat_every::flat_every, 2] = f[flat_every::flat_every, 1]
        f[-1, 1] = f[-1, 0]
    if F > 3:
        f[0, 2] = f[0, 1]
    v = torch.cat([torch.full((extra, 3), 9.0), v])
    return v.contiguous(), (f + extra).contiguous()


@pytest.fixture(scope='module')
def case():
    """The eight meshes, their draws and the restatement's results at the largest (n, T): smaller ones are prefixes."""
    stretches = [(1.0, 0.3, 2.0), (1.0, 1.0, 1.0), (0.5, 1.5, 1.0), (2.0, 0.25, 1.0), (1.0, 0.3, 2.0), (1.0, 2.0, 0.5),
                 (0.7, 0.7, 1.9), (1.3, 0.4, 1.0)]
    meshes = [_mesh(F, 3 * i + (i % 2) * 40, st) for i, (F, st) in enumerate(zip(_counts(), stretches))]
    for v, f in meshes:                                                # the premise of exactness, before any GPU work
        assert R.exact_sum_margin(R.face_areas(v.numpy(), f.numpy())) < 2 ** 29
    g = torch.Generator().manual_seed(17)
    S = len(meshes)
    u = torch.rand(S, T_MAX, N_MAX, 3, generator=g)
    u[:, :, 0, 0], u[:, :, 1, 0] = 0.0, 1.0 - 2.0 ** -24               # both ends of the table
    xf = torch.randn(S, T_MAX, 3, 4, generator=g)
    want = {('philox', False): R.sample_batch(meshes, N_MAX, T_MAX, seed=SEED, mesh_base=BASE),
            ('philox', True): R.sample_batch(meshes, N_MAX, T_MAX, seed=SEED, mesh_base=BASE, xforms=xf.numpy()),
            ('explicit', False): R.sample_batch(meshes, N_MAX, T_MAX, u=u.numpy()),
            ('explicit', True): R.sample_batch(meshes, N_MAX, T_MAX, u=u.numpy(), xforms=xf.numpy())}
    import vpn_amd
    return dict(meshes=meshes, u=u, xf=xf, want=want, batch=vpn_amd.MeshBatch.pack(meshes, DEV))


def _equal(got, want, n, T):
    pts, face, bary = (x.cpu() for x in got)
    wf, wb, wp = want
    assert torch.equal(face.long(), wf[:, :T, :n])
    assert torch.equal(bary, wb[:, :T, :n])
    assert torch.equal(pts, wp[:, :T, :n])


@pytest.mark.parametrize('T', [1, 2])
@pytest.mark.parametrize('n', [1, 255, 257])
def test_bit_exact_against_the_restatement(case, n, T):
    import vpn_amd
    b, u, xf = case['batch'], case['u'][:, :T, :n].contiguous(), case['xf'][:, :T].contiguous()
    for draws in ('philox', 'explicit'):
        for with_xf in (False, True):
            kw = dict(seed=SEED, mesh_base=BASE) if draws == 'philox' else dict(u=u.to(DEV))
            got = vpn_amd.sample_gt_points(b, n, sets=T, xforms=xf.to(DEV) if with_xf else None, return_faces=True, **kw)
            _equal(got, case['want'][(draws, with_xf)], n, T)
    only = vpn_amd.sample_gt_points(b, n, sets=T, seed=SEED, mesh_base=BASE)              # without return_faces: the points alone
    assert torch.equal(only.cpu(), case['want'][('philox', False)][2][:, :T, :n])


def test_set_0_is_the_existing_sampler(case):
    """Four meshes of one topology on a 2^-4 grid (cross products and squared norms are then exact in fp32, so mesh.hip,
    compiled with contraction, computes the same areas): equal faces, points within 1e-6."""
    import vpn_amd
    from vpn_amd import ops
    v, f = R.icosphere(2, 1.0)
    assert f.shape[0] == 320
    scales = torch.tensor([[1.0, 0.5, 2.0], [1.0, 1.0, 1.0], [2.0, 1.0, 0.5], [0.75, 1.5, 1.0]])
    verts = torch.round(v[None] * scales[:, None] * 16) / 16
    for s in range(4):
        areas = R.face_areas(verts[s].numpy(), f.numpy())
        assert areas.min() > 0 and R.exact_sum_margin(areas) < 2 ** 29
        a, b, c = (x.astype(np.float64) for x in R.corners(verts[s].numpy(), f.numpy()))
        q = (np.cross(b - a, c - a) ** 2).sum(1)
        assert np.array_equal(q, q.astype(np.float32).astype(np.float64))      # exact in fp32: contraction cannot change an area
    n, seed, base = 64, 99, 7
    p0, f0, _ = ops.sample_meshes(verts.to(DEV), ops.faces_i32(f, torch.device(DEV)), n, seed, base)
    batch = vpn_amd.MeshBatch.pack([(verts[s], f) for s in range(4)], DEV)
    p1, f1, _ = vpn_amd.sample_gt_points(batch, n, seed=seed, mesh_base=base, return_faces=True)
    assert torch.equal(f1[:, 0], f0)
    assert float((p1[:, 0] - p0).abs().max()) <= 1e-6


def test_shards_and_repacking_change_nothing(case):
    import vpn_amd
    meshes, n = case['meshes'], 255
    whole = vpn_amd.sample_gt_points(case['batch'], n, sets=2, seed=SEED, mesh_base=0, return_faces=True)
    shard = vpn_amd.sample_gt_points(vpn_amd.MeshBatch.pack(meshes[2:6], DEV), n, sets=2, seed=SEED, mesh_base=2, return_faces=True)
    for w, s in zip(whole, shard):
        assert torch.equal(w[2:6], s)
    perm = [5, 0, 7, 2, 3, 6, 1, 4]
    u = case['u'][:, :, :n].contiguous()
    a = vpn_amd.sample_gt_points(case['batch'], n, sets=2, u=u.to(DEV), return_faces=True)
    b = vpn_amd.sample_gt_points(vpn_amd.MeshBatch.pack([meshes[i] for i in perm], DEV), n, sets=2, u=u[perm].to(DEV),
                                 return_faces=True)
    for x, y in zip(a, b):
        assert torch.equal(x[perm], y)


def test_out_of_range_face_indices_are_clamped():
    """Clamped by construction (load_tri of gtpoints.hip): an index of P reads vertex P - 1, -1 reads vertex 0, and the
    result is the restatement's under the same clamp."""
    import vpn_amd
    v, f = R.icosphere(1, 0.5, (1.0, 0.6, 1.4))
    hi, lo = f.clone(), f.clone()
    hi[3, 1], hi[40, 2] = v.shape[0], v.shape[0]
    lo[0, 0], lo[79, 1] = -1, -1
    meshes = [(v, hi), (v, lo)]
    for vv, ff in meshes:
        assert R.exact_sum_margin(R.face_areas(vv.numpy(), ff.numpy())) < 2 ** 29
    got = vpn_amd.sample_gt_points(vpn_amd.MeshBatch.pack(meshes, DEV), 257, seed=3, return_faces=True)
    _equal(got, R.sample_batch(meshes, 257, 1, seed=3), 257, 1)


def _cameras(S):
    g = torch.Generator().manual_seed(5)
    return (0.8 + torch.rand(S, generator=g)).to(DEV), (40 * torch.rand(S, generator=g) - 20).to(DEV), (360 * torch.rand(S, generator=g)).to(DEV)


def test_gt_points_are_two_sets_over_one_table(case):
    import vpn_amd
    b, n = case['batch'], 255
    dists, elevs, azims = _cameras(len(b))
    canon, view = vpn_amd.gt_points(b, dists, elevs, azims, n=n, seed=SEED, mesh_base=BASE)
    assert canon.shape == (8, n, 3) and view.shape == (8, n, 3)
    wf, wb, wp = case['want'][('philox', False)]
    assert torch.equal(canon.cpu(), wp[:, 0, :n])                      # set 0: no transform, bit for bit
    m = vpn_amd.view_center_xforms(dists, elevs, azims).cpu()
    want = R.sample_batch(case['meshes'], n, 2, seed=SEED, mesh_base=BASE, xforms=torch.stack([m, m], 1).numpy(), xform_mask=2)
    assert torch.equal(view.cpu(), want[2][:, 1])
    # ... which is the reference's order of operations, sample then obj_to_view_points, to rounding
    moved = vpn_amd.obj_to_view_points(wp[:, 1, :n].to(DEV), dists.float(), elevs.float(), azims.float())
    assert float((view - moved).abs().max()) <= 1e-5
    inv = vpn_amd.gt_points(b, dists, elevs, azims, n=n, seed=SEED, mesh_base=BASE, dist_invariant=True)[1]
    assert float((inv - view * dists[:, None, None]).abs().max()) <= 1e-5


def test_launch_count_does_not_depend_on_the_number_of_meshes(case):
    import vpn_amd
    from vpn_amd import _lib, ops
    seen = []
    for meshes in (case['meshes'][:1], case['meshes']):
        b = vpn_amd.MeshBatch.pack(meshes, DEV)
        torch.cuda.synchronize()
        with _lib.KernelProfile() as kp:
            vpn_amd.sample_gt_points(b, 64, sets=2, seed=1)
        seen.append({k: c for k, (c, _ms) in kp.summary().items()})
    assert seen[0] == seen[1] and sum(seen[0].values()) == ops.RAGGED_LAUNCHES == 3, seen


def test_no_host_synchronisation(case):
    import vpn_amd
    b = case['batch']
    cams = _cameras(len(b))
    want = vpn_amd.gt_points(b, *cams, n=255, seed=8)                  # warm-up: code objects, cached constants
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = vpn_amd.gt_points(b, *cams, n=255, seed=8)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_graph_capture_and_replay(case):
    import vpn_amd
    b = case['batch']
    cams = _cameras(len(b))
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    eager = vpn_amd.gt_points(b, *cams, n=255, seed=8)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vpn_amd.gt_points(b, *cams, n=255, seed=8, seed_dev=step)
    torch.cuda.current_stream().wait_stream(s)
    fixed, counted = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(fixed):
        out_fixed = vpn_amd.gt_points(b, *cams, n=255, seed=8)
    with torch.cuda.graph(counted):
        out_counted = vpn_amd.gt_points(b, *cams, n=255, seed=8, seed_dev=step)
    for _ in range(2):                                                 # a fixed seed: every replay gives the eager bytes
        fixed.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_fixed[0], eager[0]) and torch.equal(out_fixed[1], eager[1])
    counted.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_counted[0], eager[0]) and torch.equal(out_counted[1], eager[1])
    step += 1                                                          # the replay reads the counter: new draws, seed 9's
    counted.replay()
    torch.cuda.synchronize()
    fresh = vpn_amd.gt_points(b, *cams, n=255, seed=9)
    assert not torch.equal(out_counted[0], eager[0])
    assert torch.equal(out_counted[0], fresh[0]) and torch.equal(out_counted[1], fresh[1])
