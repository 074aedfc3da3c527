"""GPU tests of the volumetric evaluation (VolumeEvaluationMeter, ops.primitive_occupancy, ops.winding_number,
ops.ragged_winding_number, ops.mesh_occupancy, ops.voliou_step on csrc/occupancy.hip) against the float64
restatement of tests/occupancy_ref.py.

Bars.  Winding number: max(1e-4, 4 x own) absolute, own the error of the restatement run in fp32 against float64 on the same
inputs (the rule of tests/test_pointmesh.py); the decision w > 0.5 equals float64's for every query, which the inputs allow:
every query lies >= 1e-3 from every triangle and has |w64 - 0.5| >= 0.05 (tests/test_occupancy_cpu.py checks it).  Primitive
occupancy and owner: exact, every |m64 - 1| >= 1e-4.  IoU counts: exact; rows: 1 fp32 ulp, one rounding of an fp64 quotient.
Bookkeeping, determinism, graph replay: bit-equal.

Worst measured on an MI355X: winding number 1.2e-7 on the icospheres and the ragged batch (own 1.8e-7 to
2.4e-7), 6.5e-9 on the cube; everything else exact."""
import os
import subprocess
import sys

import pytest
import torch

import occupancy_ref as R
import surfeval_ref as SR
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAMES5 = ['airplane', 'rifle', 'display', 'table', 'telephone']
REFLECT = [[1.0, 0, 0, 0], [0, 0, 1.0, 0], [0, 1.0, 0, 0]]                    # y and z swapped: det < 0


def _bar(verts, faces, queries, xforms, w64):
    own = float((R.winding(verts, faces, queries, xforms, dtype=torch.float32).double() - w64).abs().max())
    return max(1e-4, 4 * own), own


def _check(name, got, w64, bar, own):
    err = float((got.double().cpu() - w64).abs().max())
    print('%s: winding number against float64: worst %.2e (own %.2e, bar %.1e)' % (name, err, own, bar))
    assert bool(torch.isfinite(got).all()) and err <= bar
    assert torch.equal(got.cpu() > 0.5, w64 > 0.5)                             # every decision, no case left out


def _batched(name):
    from vpn_amd import ops
    c = R.mesh_case(name)
    verts, faces, q = c['verts'], c['faces'], c['queries']
    w64 = R.winding(verts, faces, q)
    bar, own = _bar(verts, faces, q, None, w64)
    got = ops.winding_number(verts.to(DEV), faces, q.to(DEV))
    _check(name, got, w64, bar, own)
    occ = ops.mesh_occupancy(verts.to(DEV), faces, q.to(DEV))
    assert occ.dtype == torch.uint8 and torch.equal(occ, (got > 0.5).to(torch.uint8))
    return c, got


def test_winding_cube_one_query():
    c, got = _batched('cube')
    assert got.shape == (1, 1) and c['faces'].shape[0] == 12


def test_winding_shared_queries_equal_repeated_ones_and_three_slices():
    from vpn_amd import ops
    assert ops.winding_plan(3, 257, 320) == (3, 107) and 320 - 2 * 107 < 107        # at least three slices, the last one short
    c, got = _batched('ico2')
    assert got.shape == (3, 257)
    rep = c['queries'][None].expand(3, -1, -1).contiguous().to(DEV)
    assert torch.equal(ops.winding_number(c['verts'].to(DEV), c['faces'], rep), got)  # [Q,3] and [B,Q,3]: the same bits
    assert torch.equal(ops.winding_number(c['verts'].to(DEV), c['faces'].int().to(DEV), rep), got)


def test_winding_ten_slices():
    from vpn_amd import ops
    assert ops.winding_plan(1, 257, 1280)[0] >= 3
    _batched('ico3')


def test_winding_ragged_layout_with_view_maps():
    from vpn_amd import MeshBatch, ops
    c = R.ragged_case()
    batch = MeshBatch.pack(c['meshes'], DEV)
    assert batch.face_counts == [12, 80, 1280] and torch.equal(batch.host['verts'], c['verts'])
    w64 = R.ragged_winding(c['verts'], c['faces'], c['vert_offset'], c['face_offset'], c['queries'], c['xforms'])
    w32 = R.ragged_winding(c['verts'], c['faces'], c['vert_offset'], c['face_offset'], c['queries'], c['xforms'], dtype=torch.float32)
    own = float((w32.double() - w64).abs().max())
    q, xf = c['queries'].to(DEV), c['xforms'].to(DEV)
    got = ops.ragged_winding_number(batch, q, xf)
    _check('ragged', got, w64, max(1e-4, 4 * own), own)
    arrays = (batch.verts, batch.faces, batch.vert_offset, batch.face_offset, 1280)
    assert torch.equal(ops.ragged_winding_number(arrays, q, xf), got)
    assert torch.equal(ops.mesh_occupancy(batch, None, q, xf), (got > 0.5).to(torch.uint8))
    # a plan made for fewer faces than a mesh has still sums every face (its last slice runs to the end)
    low = ops.ragged_winding_number((batch.verts, batch.faces, batch.vert_offset, batch.face_offset, 200), q, xf)
    _check('ragged, max_faces 200', low, w64, max(1e-4, 4 * own), own)
    # every mesh alone in the batched layout gives what it gives in the packed one, within the bar
    for s, (v, f) in enumerate(c['meshes']):
        alone = ops.winding_number(v.float()[None].to(DEV), f, q[s:s + 1], xf[s:s + 1])
        assert float((alone - got[s:s + 1]).abs().max()) <= 1e-4


def test_winding_known_answers():
    from vpn_amd import ops
    v, f = R.box()
    v32 = v.float()[None].to(DEV)
    inside = torch.tensor([[0.0, 0.0, 0.0], [0.2, -0.1, 0.24], [-0.2, 0.2, 0.0]])
    outside = torch.tensor([[0.3, 0.0, 0.0], [0.0, 0.0, -0.26], [2.0, 1.0, -3.0], [0.26, 0.26, 0.26]])
    x = torch.cat([inside, outside]).to(DEV)
    want = torch.tensor([[1.0] * 3 + [0.0] * 4])
    bar = 1e-4
    w = ops.winding_number(v32, f, x).cpu()
    assert float((w - want).abs().max()) <= bar
    assert abs(float(ops.winding_number(v32, f[:10], x[:1])) - 5 / 6) <= bar                # the cube without its top
    v2, f2 = R.two_boxes()
    x2 = torch.tensor([[0.1, 0.0, 0.0], [-0.1, 0.0, 0.0], [0.4, 0.1, 0.1], [0.6, 0.0, 0.0]])
    w2 = ops.winding_number(v2.float()[None].to(DEV), f2, x2.to(DEV)).cpu()
    assert float((w2 - torch.tensor([[2.0, 1.0, 1.0, 0.0]])).abs().max()) <= bar            # 2 in the overlap
    assert ops.mesh_occupancy(v2.float()[None].to(DEV), f2, x2.to(DEV)).tolist() == [[1, 1, 1, 0]]
    assert float((ops.winding_number(v32, f.flip(1), x).cpu() + want).abs().max()) <= bar   # reversed faces: -1
    assert not ops.mesh_occupancy(v32, f.flip(1), x).any()
    xf = torch.tensor([REFLECT]).to(DEV)
    assert float((ops.winding_number(v32, f, x, xf).cpu() + want).abs().max()) <= bar       # a reflection negates w
    for name in ('cube', 'ico2'):                                                           # and exactly so on the drawn queries
        c = R.mesh_case(name)
        B = c['verts'].shape[0]
        plain = ops.winding_number(c['verts'].to(DEV), c['faces'], c['queries'].to(DEV))
        mirrored = ops.winding_number(c['verts'].to(DEV), c['faces'], c['queries'][..., [0, 2, 1]].contiguous().to(DEV),
                                      torch.tensor([REFLECT] * B).to(DEV))
        w64 = R.winding(c['verts'], c['faces'], c['queries'])
        assert float((mirrored.double().cpu() + w64).abs().max()) <= bar and float((mirrored + plain).abs().max()) <= bar


def test_winding_exact_zero_cases_and_indices_outside_the_mesh():
    from vpn_amd import ops
    v, f = R.box()
    v32 = v.float()[None].to(DEV)
    on_vertex, on_plane_in, on_plane_out = v[0].tolist(), [0.1, -0.05, -0.25], [3.0, 7.0, -0.25]
    x = torch.tensor([on_vertex, on_plane_in, on_plane_out, [0.0, 0.1, 0.2], [0.4, 0.0, 0.0]])
    # one face alone: exactly 0 from a vertex and from its plane
    assert ops.winding_number(v32, f[:1], x[:3].to(DEV)).tolist() == [[0.0, 0.0, 0.0]]
    flat = torch.tensor([[0, 0, 0], [0, 1, 1], [2, 2, 0]])
    assert ops.winding_number(v32, flat, x.to(DEV)).tolist() == [[0.0] * 5]                  # faces of no area
    outside_mesh = torch.tensor([[0, 1, 8], [-1, 2, 3], [0, 1 << 30, 2]])
    assert ops.winding_number(v32, outside_mesh, x.to(DEV)).tolist() == [[0.0] * 5]          # nothing read out of range
    # beside the closed cube such faces change nothing; the float64 statement skips them too
    extra = torch.cat([f[:5], flat, outside_mesh, f[5:]])
    got, base = ops.winding_number(v32, extra, x.to(DEV)), ops.winding_number(v32, f, x.to(DEV))
    w64 = R.winding(v.float()[None], extra, x)
    assert bool(torch.isfinite(got).all()) and float((got.double().cpu() - w64).abs().max()) <= 1e-4
    assert float((got - base).abs().max()) <= 1e-6 and got[0, 3:].tolist() == base[0, 3:].tolist()
    assert float((R.winding(v.float()[None], f, x) - w64).abs().max()) <= 1e-14
    # the same in the ragged layout, and an offset table that does not describe the arrays names no face
    vo, fo = torch.tensor([0, 8, 16], dtype=torch.int32, device=DEV), torch.tensor([0, 12, 23], dtype=torch.int32, device=DEV)
    packed_v, packed_f = torch.cat([v, v]).float().to(DEV), torch.cat([f, extra[:11]]).int().to(DEV)
    rag = ops.ragged_winding_number((packed_v, packed_f, vo, fo, 12), x.to(DEV))
    assert torch.equal(rag[0], base[0]) and float((rag[1].double().cpu() - R.winding(v.float()[None], extra[:11], x)[0]).abs().max()) <= 1e-4
    bad_fo = torch.tensor([0, 12, 24], dtype=torch.int32, device=DEV)                         # 24 > 23 faces: mesh 1 names nothing
    rag = ops.ragged_winding_number((packed_v, packed_f, vo, bad_fo, 12), x.to(DEV))
    assert torch.equal(rag[0], base[0]) and rag[1].tolist() == [0.0] * 5
    # a coordinate that is not finite makes w NaN, and NaN is outside
    xn = x.clone()
    xn[0, 0], xn[1, 2] = float('nan'), float('inf')
    w = ops.winding_number(v32, f, xn.to(DEV))
    assert torch.isnan(w[0, :2]).all() and torch.equal(w[0, 2:], base[0, 2:])
    assert ops.mesh_occupancy(v32, f, xn.to(DEV))[0].tolist() == [0, 0, 0, 1, 0]
    vn = v.float()[None].clone()
    vn[0, 7, 1] = float('inf')
    assert torch.isnan(ops.winding_number(vn.to(DEV), f, x.to(DEV))).all()
    assert bool(torch.isfinite(ops.winding_number(vn.to(DEV), f[:1], x.to(DEV))).all())      # vertex 7 is not in face 0


# ---- primitives

def test_primitives_against_float64():
    from vpn_amd import ops
    c = R.prim_case()
    params, kinds, q = c['params'].to(DEV), c['kinds'], c['queries'].to(DEV)
    occ64, owner64 = R.prim_occupancy(c['params'], kinds, c['queries'])
    occ, owner = ops.primitive_occupancy(params, list(kinds), q, owner=True)
    assert occ.dtype == torch.uint8 and owner.dtype == torch.int32 and occ.shape == (3, 769)
    assert torch.equal(occ.cpu(), occ64) and torch.equal(owner.cpu(), owner64)               # exactly
    assert torch.equal(ops.primitive_occupancy(params, list(kinds), q), occ)
    rep = c['queries'][None].expand(3, -1, -1).contiguous().to(DEV)
    occ_r, owner_r = ops.primitive_occupancy(params, list(kinds), rep, owner=True)
    assert torch.equal(occ_r, occ) and torch.equal(owner_r, owner)                           # [Q,3] and [B,Q,3]: the same bits
    # the union is the OR of three K = 1 calls, bit for bit; the owner the lowest of them
    single = [ops.primitive_occupancy(params[:, k:k + 1].contiguous(), [kinds[k]], q) for k in range(3)]
    assert torch.equal(single[0] | single[1] | single[2], occ)
    lowest = torch.where(single[0] > 0, 0, torch.where(single[1] > 0, 1, torch.where(single[2] > 0, 2, -1))).int()
    assert torch.equal(lowest, owner)
    # K = 1 and Q = 1
    one, own = ops.primitive_occupancy(params[:1, 1:2].contiguous(), [kinds[1]], params[0, 1, 7:10][None].contiguous(), owner=True)
    assert one.tolist() == [[1]] and own.tolist() == [[0]]                                   # the centre of a sphere
    far, own = ops.primitive_occupancy(params[:1, 1:2].contiguous(), [kinds[1]], torch.full((1, 3), 5.0, device=DEV), owner=True)
    assert far.tolist() == [[0]] and own.tolist() == [[-1]]
    # a non-finite m is outside: a zero extent gives 0 / 0 at the centre and inf elsewhere
    bad = c['params'].clone()
    bad[0, :, 0] = 0.0
    qb = torch.cat([bad[0, 0, 7:10][None], c['queries'][:5]]).contiguous().to(DEV)
    occ_b, own_b = ops.primitive_occupancy(bad.to(DEV), list(kinds), qb, owner=True)
    assert not occ_b[0].any() and bool((own_b[0] == -1).all())
    more = ops.primitive_occupancy(torch.cat([params] * 100, 1).contiguous(), list(kinds) * 100, q, owner=True)       # K = 300: two stagings
    assert torch.equal(more[0], occ) and torch.equal(more[1], owner)


@pytest.mark.parametrize('kind', [0, 1])
def test_pose_convention_is_the_samplers(kind):
    """Points of vpn_sample_fwd for K = 1 lie on the primitive's surface: pulled towards t by 0.99 all are inside, pushed
    out by 1.01 all are outside."""
    from vpn_amd import ops
    c = R.prim_case()
    params = c['params'][:, kind:kind + 1].contiguous().to(DEV)
    pts = ops.SampleFunction.apply(params, [kind], None, 11, 0, 257)                          # [3,257,3]
    t = params[:, :, 7:10]
    inner, outer = (t + 0.99 * (pts - t)).contiguous(), (t + 1.01 * (pts - t)).contiguous()
    assert bool(ops.primitive_occupancy(params, [kind], inner).all())
    assert not ops.primitive_occupancy(params, [kind], outer).any()


# ---- IoU and the meter

def _occupancies(B, Q, seed):
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(B, Q, generator=g) < 0.4).to(torch.uint8)
    b = (torch.rand(B, Q, generator=g) < 0.5).to(torch.uint8) * (torch.rand(B, 1, generator=g) < 0.8).to(torch.uint8)
    return a, b


def _ulp1(got, want):
    got, want = got.cpu(), want
    return bool(((got - want).abs() <= torch.finfo(torch.float32).eps * want.abs()).all())


def test_iou_counts_rows_two_boxes_and_the_empty_union():
    from vpn_amd import ops
    for B, Q, seed in ((3, 769, 1), (1, 1, 2), (2, 256, 3), (5, 4097, 4)):
        a, b = _occupancies(B, Q, seed)
        a[0, 0] = 7                                                                          # any non-zero value is inside
        state = ops.voliou_state(3, DEV)
        rows, counts = ops.voliou_step(a.to(DEV), b.to(DEV), torch.zeros(B, dtype=torch.int32, device=DEV), state, 3)
        want_rows, want_counts = R.iou_rows(a, b)
        assert torch.equal(counts.cpu().long(), want_counts) and _ulp1(rows, want_rows)
        assert torch.equal(rows.cpu(), want_rows)                                            # one rounding of the same fp64 quotient
    # two half-extent-0.25 boxes at x = 0 and x = 0.25 on the 16^3 grid: as cuboids and as meshes
    q = ops.grid_queries(16, device=DEV)
    assert torch.equal(q.cpu(), R.grid_queries(16))
    p = R.two_box_params().to(DEV)
    occ_a, occ_b = (ops.primitive_occupancy(p[:, k:k + 1].contiguous(), [1], q) for k in range(2))
    v, f = R.box()
    vb, _ = R.box((0.25, 0.0, 0.0))
    mesh_a, mesh_b = (ops.mesh_occupancy(x.float()[None].to(DEV), f, q) for x in (v, vb))
    assert torch.equal(mesh_a, occ_a) and torch.equal(mesh_b, occ_b)
    state = ops.voliou_state(1, DEV)
    rows, counts = ops.voliou_step(occ_a, mesh_b, torch.zeros(1, dtype=torch.int32, device=DEV), state, 1)
    assert counts.tolist() == [[256, 768, 512, 512]]
    assert rows[0].tolist() == [float(torch.tensor(1 / 3, dtype=torch.float64).float()), 0.5, 0.5, 0.125, 0.125]
    # an empty union: a row of 0 and n_empty
    zero = torch.zeros(2, 100, dtype=torch.uint8, device=DEV)
    rows, counts = ops.voliou_step(zero, zero, torch.zeros(2, dtype=torch.int32, device=DEV), state, 1)
    assert not rows.any() and not counts.any()
    sums, cnt = ops.voliou_state_fields(state.cpu(), 1)
    assert cnt.tolist() == [3, 2, 2, 0, 3]


def test_meter_state_is_the_host_loop():
    from vpn_amd import VolumeEvaluationMeter
    C = 5
    meter = VolumeEvaluationMeter(NAMES5, DEV, resolution=4)
    batches = []
    for k, (B, idx) in enumerate(((3, [0, 2, -1]), (3, [2, C, 4]), (2, [2, 0]))):
        a, b = _occupancies(B, 513, 10 + k)
        if k == 1:
            a[1], b[1] = 0, 0                                                                # an empty union
        rows, counts = meter.update(a.to(DEV), b.to(DEV), idx if k else torch.tensor(idx))
        batches.append((rows.cpu(), counts.cpu(), idx))
    sums, counts = R.bookkeeping(batches, C)
    assert (counts[0], counts[1], counts[3]) == (8, 3, 2) and counts[2] >= 1 and counts[4:] == [2, 0, 3, 0, 1]
    assert torch.equal(meter.state.cpu(), R.state_tensor(sums, counts))                      # float64 and int64 bit patterns
    res = meter.result()
    assert (res['n_samples'], res['n_batches'], res['n_empty'], res['n_invalid'], res['class_n']) == (8, 3, counts[2], 2, [2, 0, 3, 0, 1])
    assert [res[k] for k in ('iou', 'precision', 'recall', 'vol_pred', 'vol_gt')] == [s / 8 for s in sums[:5]]
    assert res['class_iou'][2] == sums[15] / 3 and res['class_iou'][1] is None
    # more samples than one staging chunk and more (class, column) items than lanes
    Cb, B = 60, 300
    big = VolumeEvaluationMeter(['c%d' % i for i in range(Cb)], DEV, resolution=2)
    a, b = _occupancies(B, 70, 20)
    a[[5, 290]], b[[5, 290]] = 0, 0                                                          # empty unions in both staging chunks
    idx = torch.randint(-1, Cb + 1, (B,), generator=torch.Generator().manual_seed(33))
    rows, cnt = big.update(a.to(DEV), b.to(DEV), idx)
    sums, counts = R.bookkeeping([(rows.cpu(), cnt.cpu(), idx.tolist())], Cb)
    assert torch.equal(big.state.cpu(), R.state_tensor(sums, counts)) and counts[3] > 0 and counts[2] == 2


def _meter_inputs():
    """Three batches of (params, verts, MeshBatch, xforms, class indices) on the device: K = 3 primitives, the level-1
    icosphere as the predicted mesh, ragged ground truth of a box and two icospheres."""
    from vpn_amd import MeshBatch
    from vpn_amd.modules.dataset import view_center_xforms
    c = R.prim_case()
    faces = SR.icosphere(1)[1].int().to(DEV)
    out = []
    for k in range(3):
        params = c['params'].roll(k, 0).contiguous().to(DEV)
        verts = R.ellipsoids(1, 3, seed=k).to(DEV)
        meshes = [R.box((0.05 * k, 0.0, 0.0)), (SR.icosphere(1)[0] * (0.3 + 0.02 * k), SR.icosphere(1)[1]),
                  (SR.icosphere(2)[0] * 0.25, SR.icosphere(2)[1])]
        xf = view_center_xforms([1.0, 1.1, 0.9], [20.0 + k, 5.0, 30.0], [100.0, 200.0 + k, 10.0]).to(DEV)
        idx = torch.tensor([(2 * k + b) % 5 for b in range(3)], dtype=torch.int32, device=DEV)
        out.append((params, verts, MeshBatch.pack(meshes, DEV), xf, idx))
    return c['kinds'], faces, out


def test_update_primitives_and_update_mesh_are_their_steps():
    from vpn_amd import VolumeEvaluationMeter, ops
    kinds, faces, batches = _meter_inputs()
    params, verts, gt, xf, idx = batches[0]
    a, b = VolumeEvaluationMeter(NAMES5, DEV, resolution=8), VolumeEvaluationMeter(NAMES5, DEV, resolution=8)
    q = ops.grid_queries(8, device=DEV)
    assert torch.equal(a.queries, q)
    occ_gt = ops.mesh_occupancy(gt, None, q, xf)
    rows_a, counts_a = a.update_primitives(params, list(kinds), gt, idx, gt_xforms=xf)
    rows_b, counts_b = b.update(ops.primitive_occupancy(params, list(kinds), q), occ_gt, idx)
    assert torch.equal(rows_a, rows_b) and torch.equal(counts_a, counts_b) and torch.equal(a.state, b.state)
    rows_a, counts_a = a.update_mesh(verts, faces, gt, idx, gt_xforms=xf)
    rows_b, counts_b = b.update(ops.mesh_occupancy(verts, faces, q), occ_gt, idx)
    assert torch.equal(rows_a, rows_b) and torch.equal(counts_a, counts_b) and torch.equal(a.state, b.state)
    assert a.result() == b.result() and 0 < a.result()['iou'] < 1 and a.result()['n_empty'] == 0
    assert int(counts_a[:, 0].min()) > 0                                                     # prediction and ground truth overlap
    own = VolumeEvaluationMeter(NAMES5, DEV, queries=q.cpu())                                # explicit queries: the same bits
    assert torch.equal(own.update_mesh(verts, faces, gt, idx, gt_xforms=xf)[0], rows_a)


def test_determinism_no_host_sync_and_graph_replay():
    from vpn_amd import VolumeEvaluationMeter
    kinds, faces, batches = _meter_inputs()
    from vpn_amd import ops
    kt = ops.kinds_tensor(list(kinds), DEV)

    def run(meter, items):
        out = []
        for params, verts, gt, xf, idx in items:
            out.append(meter.update_primitives(params, kt, gt, idx, gt_xforms=xf)[0].clone())
            out.append(meter.update_mesh(verts, faces, gt, idx, gt_xforms=xf)[0].clone())
        return out

    one, two = VolumeEvaluationMeter(NAMES5, DEV, resolution=8), VolumeEvaluationMeter(NAMES5, DEV, resolution=8)
    rows_1 = run(one, batches)                                                               # also the warm-up of every code object
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        rows_2 = run(two, batches)                                                           # class indices already on the device
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(rows_1, rows_2)) and torch.equal(one.state, two.state)       # two runs: the same bits
    want = one.result()
    # one capture, three replays: the ground truth keeps its topology (one MeshBatch), its vertices, maps and the prediction change
    meter = VolumeEvaluationMeter(NAMES5, DEV, resolution=8)
    same_gt = [(p, v, batches[0][2], xf, idx) for p, v, _, xf, idx in batches]
    ref = VolumeEvaluationMeter(NAMES5, DEV, resolution=8)
    rows_ref = run(ref, same_gt)
    sp, sv, gt, sxf, sidx = (batches[0][0].clone(), batches[0][1].clone(), batches[0][2], batches[0][3].clone(), batches[0][4].clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(meter, [(sp, sv, gt, sxf, sidx)])                                                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    meter.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rows = run(meter, [(sp, sv, gt, sxf, sidx)])
    assert meter.result()['n_batches'] == 0                                                  # capturing ran nothing
    for k, (p, v, _, xf, idx) in enumerate(same_gt):
        sp.copy_(p)
        sv.copy_(v)
        sxf.copy_(xf)
        sidx.copy_(idx)
        graph.replay()
        assert torch.equal(rows[0], rows_ref[2 * k]) and torch.equal(rows[1], rows_ref[2 * k + 1])
    torch.cuda.synchronize()
    assert torch.equal(meter.state, ref.state) and meter.result() == ref.result()
    assert want['n_batches'] == 6 and want['n_samples'] == 18


def test_the_other_meters_are_untouched_by_a_volume_update():
    from vpn_amd import EvaluationMeter, SurfaceEvaluationMeter, VolumeEvaluationMeter
    p, q = [t.to(DEV) for t in SR.clouds('clustered')]
    old, surf = EvaluationMeter(NAMES5, DEV, emd=False), SurfaceEvaluationMeter(NAMES5, DEV)
    before, _ = old.update(p, q, [0, 1, 2])
    rows_before = surf.update(p, q, [0, 1, 2])
    state, sstate = old.state.clone(), surf.state.clone()
    kinds, faces, batches = _meter_inputs()
    params, verts, gt, xf, idx = batches[0]
    vol = VolumeEvaluationMeter(NAMES5, DEV, resolution=4)
    vol.update_primitives(params, list(kinds), gt, idx, gt_xforms=xf)
    vol.update_mesh(verts, faces, gt, idx, gt_xforms=xf)
    assert torch.equal(old.state, state) and torch.equal(surf.state, sstate)
    after, _ = old.update(p, q, [0, 1, 2])
    assert torch.equal(before, after) and old.result()['n_batches'] == 2
    assert torch.equal(surf.update(p, q, [0, 1, 2]), rows_before)


@pytest.mark.parametrize('flags', [[], ['--gcn']])
def test_eval_step_example_prints_the_volume_table(flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'eval_step.py'), '--batches', '2', '--epoch', '3', '--volume',
                        '--resolution', '8'] + flags, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if 'volume iou = ' in l]
    assert len(lines) == 13 + 1 and lines[-1].startswith('total'), r.stdout                  # 8 + 5 samples over 13 classes
    for l in lines:
        v = float(l.split('volume iou = ')[1].split(' ')[0])
        assert 0.0 <= v <= 1.0, l
    assert float(lines[-1].split('vol_gt = ')[1]) > 0.0                                      # the stand-in ground truth holds grid points
    assert ('avg cd loss = ' in r.stdout) != bool(flags)                                     # the existing table is still printed
    assert 'surface cd = ' not in r.stdout
