"""GPU tests of the surface evaluation (SurfaceEvaluationMeter, ops.surfeval_step, ops.face_normals_at,
ops.ragged_face_normals on csrc/surfeval.hip) against the float64 restatement of tests/surfeval_ref.py.

Bars.  Columns 0-5 of a row, and P, R and F: 2 fp32 ulps, a relative 2.4e-7 -- one rounding to fp32 of an fp64 sum, and one
ulp of margin for the fp64 summation order, whose error of about N 2^-53 can move that rounding.  Threshold counts, recovered
as round(P N) and round(R M): exact.  Normals: 1e-5 absolute per component on meshes whose faces have sin >= 0.1 of every
angle (tests/test_surfeval_cpu.py checks the inputs).  Bookkeeping, determinism, graph replay: bit-equal."""
import os
import subprocess
import sys

import pytest
import torch

import meshreg_ref as MR
import surfeval_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAMES5 = ['airplane', 'rifle', 'display', 'table', 'telephone']
ULP2 = 2.4e-7


def _close(got, want):
    """Within 2 fp32 ulps of the float64 value, relative (an exact 0 must be 0)."""
    got, want = got.double().cpu(), want.double()
    err = ((got - want).abs() / want.abs().clamp_min(1e-300)).where(want != 0, (got != 0).double())
    return float(err.max())


def _unit_normals(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g), dim=-1).contiguous()


def _step(p, q, cls, C, thr2, n_pred=None, n_gt=None):
    """ops.surfeval_step on a fresh state -> (rows, state) on the host, and the scan's outputs it was computed from."""
    from vpn_amd import ops
    state = ops.surfeval_state(C, thr2.numel(), DEV)
    dev = lambda t: None if t is None else t.to(DEV)
    rows = ops.surfeval_step(dev(p), dev(q), torch.tensor(cls, dtype=torch.int32, device=DEV), state, C, dev(thr2), dev(n_pred),
                             dev(n_gt))
    nn = [t.cpu() for t in ops.chamfer_nn(dev(p), dev(q))]
    return rows.cpu(), state.cpu(), nn


def _check_rows(rows, nn, thr2, n_pred, n_gt, N, M):
    d1, i1, d2, i2 = nn
    want, counts = R.sample_rows(d1, i1, d2, i2, thr2, n_pred, n_gt)                # float64 on the SAME fp32 scan outputs (distances, not squared)
    T = thr2.numel()
    err = _close(rows, want)
    print('rows against float64: worst relative %.2e (bar %.1e)' % (err, ULP2))
    assert err <= ULP2
    assert torch.equal((rows[:, 6:6 + T].double() * N).round().long(), counts[:, 0])         # exact, no case left out
    assert torch.equal((rows[:, 6 + T:6 + 2 * T].double() * M).round().long(), counts[:, 1])
    return want, counts


@pytest.mark.parametrize('kind', ['uniform', 'clustered'])
def test_sample_kernel_against_float64_and_counts_from_points(kind):
    p, q = R.clouds(kind)                                                            # (B, N, M, T) = (3, 257, 300, 3)
    taus = R.gap_thresholds(kind)
    thr2 = R.thr2_of(taus)
    n_pred, n_gt = _unit_normals(3, 257, 1), _unit_normals(3, 300, 2)
    n_pred[1, 5] = 0                                                                 # a zero normal adds 0
    rows, _, nn = _step(p, q, [0, 1, 2], 5, thr2, n_pred, n_gt)
    want, counts = _check_rows(rows, nn, thr2, n_pred, n_gt, 257, 300)
    assert float(rows[:, 4:6].min()) > 0.3 and float(rows[:, 4:6].max()) < 0.7       # E|cos| of random directions is 1/2
    # from the points: a float64 brute force over the clouds at thresholds that sit in gaps of its distances
    b1, _, b2, _ = R.brute_nn(p, q)
    for t, tau in enumerate(taus):
        assert torch.equal(counts[:, 0, t], (b1 < tau * tau).sum(1)) and torch.equal(counts[:, 1, t], (b2 < tau * tau).sum(1))
        assert 0 < int(counts[:, :, t].min()) and int(counts[:, 0, t].max()) < 257 and int(counts[:, 1, t].max()) < 300
    # without normals: columns 4 and 5 are 0, the rest the same bits
    bare, _, _ = _step(p, q, [0, 1, 2], 5, thr2)
    assert not bare[:, 4:6].any() and torch.equal(bare[:, :4], rows[:, :4]) and torch.equal(bare[:, 6:], rows[:, 6:])


def test_sample_kernel_one_point_and_eight_thresholds():
    # (1, 1, 1, 1): one pair
    p, q = torch.tensor([[[0.25, -0.125, 0.5]]]), torch.tensor([[[0.25, 0.125, 0.5]]])
    n = torch.tensor([[[0.0, 0.0, 1.0]]])
    for tau2, hit in ((0.0625, 0.0), (0.07, 1.0)):                                    # d = 1/16 exactly: ON the threshold is a miss
        rows, _, nn = _step(p, q, [0], 1, torch.tensor([tau2]), n, -n)
        assert rows[0].tolist() == [0.0625, 0.0625, 0.25, 0.25, 1.0, 1.0, hit, hit, hit]     # F = 0, not NaN, when P + R = 0
    # (2, 256, 64, 8): exactly one element per lane, M below a wave; thresholds at squared distances that occur, below and beyond all
    g = torch.Generator().manual_seed(21)
    p, q = torch.rand(2, 256, 3, generator=g) - 0.5, torch.rand(2, 64, 3, generator=g) - 0.5
    from vpn_amd import ops
    d1, _, d2, _ = [t.cpu() for t in ops.chamfer_nn(p.to(DEV), q.to(DEV))]
    sq = lambda x: float(x) ** 2                                                      # the scan's distances are not squared
    thr2 = torch.tensor([0.0, sq(d1.min()), sq(d1[0, 17]), sq(d2[1, 3]), sq(d1.median()), sq(d2.median()), sq(d1.max() * 1.001), 10.0])
    n_pred, n_gt = _unit_normals(2, 256, 3), _unit_normals(2, 64, 4)
    rows, _, nn = _step(p, q, [0, 0], 1, thr2, n_pred, n_gt)
    want, counts = _check_rows(rows, nn, thr2, n_pred, n_gt, 256, 64)
    assert counts[:, :, 0].tolist() == [[0, 0], [0, 0]] and counts[:, :, 7].tolist() == [[256, 64], [256, 64]]
    assert counts[:, 0, 6].tolist() == [256, 256] and int(counts[:, 0, 1].sum()) <= 1
    assert rows[:, 6 + 16].tolist() == [0.0, 0.0] and rows[:, 6 + 23].tolist() == [1.0, 1.0]


def _meshes():
    """[(verts [B,P,3] fp32, faces [F,3] int64)]: two icospheres of different sizes and the strip of 65 vertices."""
    return [(R.mesh_vertices(1, 3), R.icosphere(1)[1]), (R.mesh_vertices(2, 3), R.icosphere(2)[1]),
            (MR.vertices('strip_65', 3), MR.mesh('strip_65')[0])]


def _xforms(B):
    """A view_center_xforms row, a genre_xforms-style row (x negated, y and z swapped, scaled, moved) and a true reflection."""
    from vpn_amd.modules.dataset import view_center_xforms
    k = 1.0 / (128.0 * 1.7)
    rows = [view_center_xforms([1.3], [25.0], [140.0])[0],
            torch.tensor([[-k * 100, 0, 0, 0.1], [0, 0, k * 100, -0.2], [0, k * 100, 0, 0.05]]),
            torch.tensor([[0.5, 0, 0, 0.1], [0, 0, 0.5, -0.2], [0, 0.5, 0, 0.3]])]
    return torch.stack([rows[b % 3] for b in range(B)]).float().contiguous()


def test_normals_batched_layout():
    from vpn_amd import ops
    for verts, faces in _meshes():
        B, F = verts.shape[0], faces.shape[0]
        g = torch.Generator().manual_seed(F)
        fidx = torch.cat([torch.arange(F)[None].expand(B, -1), torch.randint(0, F, (B, 257 - F % 257), generator=g)], 1).int().contiguous()
        fidx[0, -1], fidx[1, -1], fidx[2, -2] = -1, F, 2 ** 31 - 1                    # outside [0,F): (0,0,0), nothing read
        for xf in (None, _xforms(B)):
            got = ops.face_normals_at(verts.to(DEV), faces.to(DEV), fidx.to(DEV), None if xf is None else xf.to(DEV)).cpu()
            want = R.face_normals(verts, faces, fidx, xf)
            err = float((got.double() - want).abs().max())
            print('F %d n %d xforms %s: worst component %.2e' % (F, fidx.shape[1], xf is not None, err))
            assert got.shape == (B, fidx.shape[1], 3) and err <= 1e-5
            assert not got[0, -1].any() and not got[1, -1].any() and not got[2, -2].any()
            assert float((got.norm(dim=-1) - 1).abs()[:, :F].max()) <= 1e-6
        # int32 faces on the device and int64 faces on the host are the same call
        again = ops.face_normals_at(verts.to(DEV), faces.int(), fidx.to(DEV), _xforms(B))
        assert torch.equal(again.cpu(), got)
    # a vertex index outside [0,P): (0,0,0)
    v, f = R.mesh_vertices(1, 3), R.icosphere(1)[1].clone()
    f[3, 1], f[5, 0] = 42, -1
    got = ops.face_normals_at(v.to(DEV), f.to(DEV), torch.arange(80, dtype=torch.int32, device=DEV)[None].repeat(3, 1)).cpu()
    assert not got[:, 3].any() and not got[:, 5].any() and bool(got[:, 4].any())


def test_normals_exact_cases():
    from vpn_amd import ops
    v = torch.tensor([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [5, 5, 5]]])
    f = torch.tensor([[0, 1, 2], [0, 1, 3], [4, 4, 4], [1, 0, 2]])
    got = ops.face_normals_at(v.to(DEV), f, torch.tensor([[0, 1, 2, 3]], dtype=torch.int32, device=DEV)).cpu()
    assert got[0].tolist() == [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, -1.0]]       # bit-exact
    swap = torch.tensor([[[2.0, 0, 0, 1], [0, 0, 2, 0], [0, 2, 0, -1]]])                                   # exact in fp32; det < 0
    got = ops.face_normals_at(v.to(DEV), f, torch.tensor([[0, 1, 2, 3]], dtype=torch.int32, device=DEV), swap.to(DEV)).cpu()
    assert got[0].tolist() == [[0.0, -1.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]]       # the reflection flips the sign


def test_normals_ragged_layout_and_gt_normals():
    """Two meshes of different sizes, sets = 2, mesh-local indices, through sample_gt_points and gt_normals."""
    import vpn_amd
    from vpn_amd import ops
    (v1, f1), (v2, f2) = _meshes()[:2]
    batch = vpn_amd.MeshBatch.pack([(v1[0], f1), (v2[1], f2)], DEV)
    S, sets, n = 2, 2, 300
    view = vpn_amd.view_center_xforms([1.3, 0.9], [25.0, -10.0], [140.0, 33.0])
    xf = torch.stack([view, _xforms(3)[[2, 1]]], 1).contiguous()                      # [S,sets,3,4]
    pts, face, bary = vpn_amd.sample_gt_points(batch, n, sets=sets, xforms=xf, seed=5, return_faces=True)
    face_h = face.cpu()
    assert int(face_h[0].max()) < 80 <= int(face_h[1].max()) < 320                   # mesh-local, different sizes
    for x in (None, xf):
        got = vpn_amd.gt_normals(batch, face, sets=sets, xforms=None if x is None else x.to(DEV)).cpu()
        want = R.ragged_normals(batch.host['verts'], batch.host['faces'], batch.host['vert_offset'], batch.host['face_offset'],
                                face_h, sets, x)
        err = float((got.double() - want).abs().max())
        print('ragged, xforms %s: worst component %.2e' % (x is not None, err))
        assert got.shape == (S, sets, n, 3) and err <= 1e-5
        flat = ops.ragged_face_normals(batch.verts, batch.faces, batch.vert_offset, batch.face_offset, face.reshape(S * sets, n), sets,
                                       None if x is None else x.reshape(S * sets, 3, 4))
        assert torch.equal(flat.cpu().reshape(S, sets, n, 3), got)
    # the mapped normal is perpendicular to the mapped face the point was sampled on: the sampled points lie in its plane
    corners = R._map(batch.host['verts'].double()[batch.host['faces'].long()[:80]][face_h[0, 1].long()], xf[0, 1].double())
    assert float(((pts[0, 1].cpu().double() - corners[:, 0]) * got[0, 1].double()).sum(-1).abs().max()) <= 1e-6
    # a face index outside its mesh gives (0,0,0): index 80 exists in the packed list but not in mesh 0
    bad = face.clone()
    bad[0, 0, 0], bad[1, 1, 7] = 80, -1
    got = vpn_amd.gt_normals(batch, bad, sets=sets).cpu()
    assert not got[0, 0, 0].any() and not got[1, 1, 7].any() and bool(got[0, 0, 1].any())


def test_bookkeeping_is_the_host_loop_bit_for_bit():
    from vpn_amd import SurfaceEvaluationMeter, ops
    C, T = 5, 3
    taus = R.gap_thresholds('clustered')
    meter = SurfaceEvaluationMeter(NAMES5, DEV, thresholds=taus)
    assert torch.equal(meter.thr2.cpu(), R.thr2_of(taus))
    batches, normals = [], []
    for k, (sl, idx) in enumerate((([0, 1, 2], [0, -1, 2]), ([2, 0, 1], [2, 2, C]), ([1, 2], [4, 0]))):     # sizes (3, 3, 2); one class index -1, one equal to C
        p, q = R.clouds('clustered')
        n_pred, n_gt = _unit_normals(3, 257, 10 + k), _unit_normals(3, 300, 20 + k)
        b = len(sl)
        rows = meter.update(p[sl].to(DEV), q[sl].to(DEV), idx, n_pred[sl].to(DEV), n_gt[sl].to(DEV))
        assert rows.shape == (b, 6 + 3 * T) and rows.dtype == torch.float32
        batches.append((rows.cpu(), idx))
    sums, counts = R.bookkeeping(batches, C, T)
    assert counts == [8, 3, 2, 2, 0, 3, 0, 1]
    assert torch.equal(meter.state.cpu(), R.state_tensor(sums, counts))               # float64 and int64 bit patterns
    res = meter.result()
    W = 6 + 3 * T
    assert (res['n_samples'], res['n_batches'], res['n_invalid'], res['class_n']) == (8, 3, 2, [2, 0, 3, 0, 1])
    tot = [s / 8 for s in sums[:W]]
    assert res['cd'] == tot[0] + tot[1] and res['cd_l1'] == 0.5 * (tot[2] + tot[3]) and res['normal_consistency'] == 0.5 * (tot[4] + tot[5])
    assert res['accuracy'] == tot[0] and res['completeness'] == tot[1]
    assert res['precision'] == tot[6:6 + T] and res['recall'] == tot[6 + T:6 + 2 * T] and res['fscore'] == tot[6 + 2 * T:]
    c2 = [s / 3 for s in sums[3 * W:4 * W]]
    assert res['class_cd'][2] == c2[0] + c2[1] and res['class_fscore'][2] == c2[6 + 2 * T:] and res['class_cd'][1] is None
    assert res['thresholds'] == list(taus)
    # an epoch without normals reports None; reset starts a new epoch
    meter.reset()
    p, q = R.clouds('uniform')
    meter.update(p.to(DEV), q.to(DEV), torch.tensor([1, 1, 3]))
    res = meter.result()
    assert res['normal_consistency'] is None and res['class_normal_consistency'] == [None] * C and res['class_n'] == [0, 2, 0, 1, 0]
    assert 0 <= res['fscore'][0] <= res['fscore'][2] <= 1 and res['fscore'][2] > 0
    # more samples than one staging chunk and more (class, column) items than lanes
    Cb, B = 40, 300
    big = SurfaceEvaluationMeter(['c%d' % i for i in range(Cb)], DEV, thresholds=(0.2,))
    g = torch.Generator().manual_seed(33)
    p, q, idx = torch.rand(B, 5, 3, generator=g) - 0.5, torch.rand(B, 3, 3, generator=g) - 0.5, torch.randint(-1, Cb + 1, (B,), generator=g)
    rows = big.update(p.to(DEV), q.to(DEV), idx)
    sums, counts = R.bookkeeping([(rows.cpu(), idx.tolist())], Cb, 1)
    assert torch.equal(big.state.cpu(), R.state_tensor(sums, counts)) and counts[2] > 0


def _gcn_case():
    """A small GCNModel over two composed spheres per sample: (model, meshes' vertices [B,256,3], faces, maps, glob, rgbs)."""
    from vpn_amd.modules.meshing import uv_sphere
    from vpn_amd.modules.network import GCNModel
    gen = torch.Generator().manual_seed(9)
    sv, sf = uv_sphere()
    B, K = 2, 2
    verts = torch.stack([torch.cat([sv * (torch.rand(3, generator=gen) * 0.2 + 0.1) + (torch.rand(3, generator=gen) - 0.5) * 0.6
                                    for _ in range(K)]) for _ in range(B)])
    faces = torch.cat([sf + sv.shape[0] * k for k in range(K)])
    maps = [torch.randn(B, c, s, s, generator=gen) for c, s in [(4, 32), (8, 16), (16, 8), (32, 4)]]
    glob = torch.randn(B, 16, generator=gen)
    rgbs = torch.zeros(B, 3, 64, 64)
    rgbs[:, :, 8:56, 12:50] = 0.5
    torch.manual_seed(11)
    return GCNModel(img_feature_dim=60 + 16, v_num=verts.shape[1]), verts, faces, maps, glob, rgbs


def test_update_mesh_is_its_three_steps_and_takes_a_refined_mesh():
    from vpn_amd import SurfaceEvaluationMeter, ops
    from vpn_amd.modules.meshing import TriangleMesh
    verts, faces = _meshes()[1]
    _, q = R.clouds('uniform')
    gt_n = _unit_normals(3, 300, 5).to(DEV)
    v, q = verts.to(DEV), q.to(DEV)
    a, b = SurfaceEvaluationMeter(NAMES5, DEV), SurfaceEvaluationMeter(NAMES5, DEV)
    rows_a = a.update_mesh(v, faces, q, [0, 1, 1], n=257, seed=77, mesh_base=3, gt_normals=gt_n)
    f32 = ops.faces_i32(faces, v.device)
    pts, fidx, _ = ops.sample_meshes(v, f32, 257, 77, 3)
    rows_b = b.update(pts, q, [0, 1, 1], ops.face_normals_at(v, f32, fidx), gt_n)
    assert torch.equal(rows_a, rows_b) and torch.equal(a.state, b.state) and a.result() == b.result()
    assert a.result()['normal_consistency'] is not None
    # without ground-truth normals the normals step is skipped
    rows_c = a.update_mesh(v, faces, q, [0, 1, 1], n=257, seed=77, mesh_base=3)
    assert not rows_c[:, 4:6].any() and torch.equal(rows_c[:, :4], rows_a[:, :4]) and torch.equal(rows_c[:, 6:], rows_a[:, 6:])
    # the refined mesh of a small GCNModel
    model, gv, gf, maps, glob, rgbs = _gcn_case()
    model = model.to(DEV).eval()
    with torch.no_grad():
        refined = model([TriangleMesh(gv[i].to(DEV), gf.to(DEV)) for i in range(2)], rgbs.to(DEV), [m.to(DEV) for m in maps], glob.to(DEV))
    assert refined.shape == gv.shape
    m = SurfaceEvaluationMeter(NAMES5, DEV, thresholds=(0.05, 0.1))
    rows = m.update_mesh(refined, gf, q[:2], [4, 4], n=512, seed=1, gt_normals=gt_n[:2])
    res = m.result()
    assert bool(torch.isfinite(rows).all()) and res['class_n'] == [0, 0, 0, 0, 2] and 0 < res['cd'] < 3 and 0 <= res['fscore'][0] <= res['fscore'][1] <= 1
    assert 0 < res['normal_consistency'] < 1


def test_determinism_no_host_sync_and_graph_replay():
    from vpn_amd import SurfaceEvaluationMeter
    verts, faces = _meshes()[0]
    faces_d = faces.int().to(DEV)
    gt_n = _unit_normals(3, 300, 6).to(DEV)
    batches = []
    for k in range(3):
        _, q = R.clouds('uniform' if k % 2 else 'clustered')
        batches.append((R.mesh_vertices(1, 3, seed=k).to(DEV), q.to(DEV), torch.tensor([(2 * k + b) % 5 for b in range(3)], dtype=torch.int32, device=DEV)))

    def run(meter):
        return [meter.update_mesh(v, faces_d, q, idx, n=257, seed=4, gt_normals=gt_n).clone() for v, q, idx in batches]

    one, two = SurfaceEvaluationMeter(NAMES5, DEV), SurfaceEvaluationMeter(NAMES5, DEV)
    rows_1 = run(one)                                                                # also the warm-up of every code object
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        rows_2 = run(two)                                                            # class indices already on the device
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(rows_1, rows_2)) and torch.equal(one.state, two.state)       # two runs: the same bits
    want = one.result()
    # one capture, three replays
    meter = SurfaceEvaluationMeter(NAMES5, DEV)
    sv, sq, sidx = batches[0][0].clone(), batches[0][1].clone(), batches[0][2].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        meter.update_mesh(sv, faces_d, sq, sidx, n=257, seed=4, gt_normals=gt_n)     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    meter.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rows = meter.update_mesh(sv, faces_d, sq, sidx, n=257, seed=4, gt_normals=gt_n)
    assert meter.result()['n_batches'] == 0                                          # capturing ran nothing
    for k, (v, q, idx) in enumerate(batches):
        sv.copy_(v)
        sq.copy_(q)
        sidx.copy_(idx)
        graph.replay()
        assert torch.equal(rows, rows_1[k])
    torch.cuda.synchronize()
    assert torch.equal(meter.state, one.state) and meter.result() == want
    assert want['n_batches'] == 3 and want['n_samples'] == 9


def test_the_old_meter_is_untouched_by_a_surface_update():
    from vpn_amd import EvaluationMeter, SurfaceEvaluationMeter
    p, q = [t.to(DEV) for t in R.clouds('clustered')]
    old = EvaluationMeter(NAMES5, DEV, emd=False)
    before, _ = old.update(p, q, [0, 1, 2])
    state = old.state.clone()
    SurfaceEvaluationMeter(NAMES5, DEV).update(p, q, [0, 1, 2])
    assert torch.equal(old.state, state)
    after, _ = old.update(p, q, [0, 1, 2])
    assert torch.equal(before, after) and old.result()['n_batches'] == 2


@pytest.mark.parametrize('flags', [[], ['--gcn']])
def test_eval_step_example_prints_the_surface_table(flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'eval_step.py'), '--batches', '2', '--epoch', '3', '--surface',
                        '--thresholds', '0.02,0.05,0.1'] + flags, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if 'surface cd = ' in l]
    assert len(lines) == 13 + 1 and lines[-1].startswith('total'), r.stdout          # 8 + 5 samples over 13 classes
    for l in lines:
        assert all('F@%s = ' % t in l for t in ('0.02', '0.05', '0.1')), l
        assert ('nc = n/a' not in l) == bool(flags), l                               # normals with the refined mesh only
        v = float(l.split('surface cd = ')[1].split(',')[0])
        assert v == v and 0.0 < v < float('inf'), l
    assert ('avg cd loss = ' in r.stdout) != bool(flags)                             # the existing table is still printed
