"""CPU checks of the volumetric evaluation (VolumeEvaluationMeter, ops.primitive_occupancy, ops.winding_number,
ops.ragged_winding_number, ops.mesh_occupancy, ops.voliou_step, csrc/occupancy.hip): the restatement of
tests/occupancy_ref.py against plain Python loops, known answers, the host side of the meter on CPU states, the all-reduce on a
one-rank gloo group, the argument contract of ops and of the C entries, the kernels' resources and the conditioning of the
inputs the GPU test uses."""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import occupancy_ref as R
import surfeval_ref as SR
from conftest import ROOT
from kernel_resources import kernel_resources

NAMES = ['airplane', 'rifle', 'display', 'table', 'telephone']
REFLECT = [[1.0, 0, 0, 0], [0, 0, 1.0, 0], [0, 1.0, 0, 0]]                    # y and z swapped: det < 0


# ---- the restatement against plain loops

def test_winding_equals_plain_loops_in_both_layouts():
    g = torch.Generator().manual_seed(3)
    verts = torch.rand(2, 6, 3, generator=g, dtype=torch.float64)
    faces = torch.tensor([[0, 1, 2], [2, 3, 4], [5, 0, 3], [1, 1, 4], [0, 7, 2], [-1, 2, 3]])
    x = torch.rand(2, 5, 3, generator=g, dtype=torch.float64) * 2 - 0.5
    xf = torch.randn(2, 3, 4, generator=g, dtype=torch.float64)
    for m in (None, xf):
        got = R.winding(verts, faces, x, m)
        for b in range(2):
            for i in range(5):
                want = R.winding_plain(verts[b].tolist(), faces.tolist(), x[b, i].tolist(), None if m is None else m[b].tolist())
                assert abs(float(got[b, i]) - want) <= 1e-14
    shared = R.winding(verts, faces, x[0], xf)
    assert torch.equal(shared, R.winding(verts, faces, x[0][None].expand(2, -1, -1), xf))
    v2, f2 = torch.rand(4, 3, generator=g, dtype=torch.float64), torch.tensor([[0, 1, 2], [1, 3, 2]])
    packed_v, packed_f = torch.cat([verts[0], v2]), torch.cat([faces[:3], f2])
    got = R.ragged_winding(packed_v, packed_f, torch.tensor([0, 6, 10]), torch.tensor([0, 3, 5]), x, xf)
    for s, (v, f) in enumerate(((verts[0], faces[:3]), (v2, f2))):
        for i in range(5):
            assert abs(float(got[s, i]) - R.winding_plain(v.tolist(), f.tolist(), x[s, i].tolist(), xf[s].tolist())) <= 1e-14


def test_primitives_equal_plain_loops():
    c = R.prim_case()
    m = R.prim_m(c['params'], c['kinds'], c['queries'])
    for b in range(3):
        for i in (0, 100, 511, 512, 768):
            for k in range(3):
                want = R.prim_plain(c['params'][b, k].double().tolist(), c['kinds'][k], c['queries'][i].double().tolist())
                assert abs(float(m[b, i, k]) - want) <= 1e-12 * max(1.0, want)
    occ, owner = R.prim_occupancy(c['params'], c['kinds'], c['queries'])
    inside = m <= 1
    assert torch.equal(occ.bool(), inside.any(-1))
    for b, i in ((0, 0), (1, 300), (2, 700)):
        want = next((k for k in range(3) if bool(inside[b, i, k])), -1)
        assert int(owner[b, i]) == want
    # a non-finite m is outside
    bad = c['params'].clone()
    bad[0, :, 0] = 0.0                                                           # 0 / 0 at x = t, inf elsewhere
    q = torch.cat([bad[0, 0, 7:10][None], c['queries'][:3]])
    occ, owner = R.prim_occupancy(bad, c['kinds'], q)
    assert not occ[0].any() and bool((owner[0] == -1).all())


def test_grid_queries_ordering():
    from vpn_amd import ops
    q = R.grid_queries(4)
    assert q.shape == (64, 3) and q.dtype == torch.float32
    assert q[0].tolist() == [-0.375, -0.375, -0.375] and q[1].tolist() == [-0.125, -0.375, -0.375]         # ix runs fastest
    assert q[4].tolist() == [-0.375, -0.125, -0.375] and q[16].tolist() == [-0.375, -0.375, -0.125]
    assert q[(3 * 4 + 2) * 4 + 1].tolist() == [-0.125, 0.125, 0.375]
    for R_, lo, hi in ((4, -0.5, 0.5), (5, -0.3, 0.7), (16, -0.5, 0.5), (3, 0.0, 1.0)):
        assert torch.equal(ops.grid_queries(R_, lo, hi), R.grid_queries(R_, lo, hi))
    for bad in ((0, -0.5, 0.5), (300, -0.5, 0.5), (4, 0.5, 0.5), (4, 0.0, float('inf'))):
        with pytest.raises(ValueError):
            ops.grid_queries(*bad)


# ---- known answers in float64

def test_closed_cube_open_cube_doubled_boxes_reversed_and_reflected():
    v, f = R.box()
    inside = torch.tensor([[0.0, 0.0, 0.0], [0.2, -0.1, 0.24], [-0.249, 0.249, 0.0]], dtype=torch.float64)
    outside = torch.tensor([[0.3, 0.0, 0.0], [0.0, 0.0, -0.2501], [2.0, 1.0, -3.0], [0.26, 0.26, 0.26]], dtype=torch.float64)
    w_in, w_out = R.winding(v[None], f, inside), R.winding(v[None], f, outside)
    assert float((w_in - 1).abs().max()) <= 1e-12 and float(w_out.abs().max()) <= 1e-12
    centre = torch.zeros(1, 3, dtype=torch.float64)
    assert abs(float(R.winding(v[None], f[:10], centre)) - 5 / 6) <= 1e-12           # the cube without its top
    v2, f2 = R.two_boxes()
    x = torch.tensor([[0.1, 0.0, 0.0], [-0.1, 0.0, 0.0], [0.4, 0.1, 0.1], [0.6, 0.0, 0.0]], dtype=torch.float64)
    assert float((R.winding(v2[None], f2, x)[0] - torch.tensor([2.0, 1.0, 1.0, 0.0], dtype=torch.float64)).abs().max()) <= 1e-12
    assert float((R.winding(v[None], f.flip(1), inside) + 1).abs().max()) <= 1e-12   # reversed faces
    xf = torch.tensor([REFLECT], dtype=torch.float64)
    assert float((R.winding(v[None], f, inside, xf) + 1).abs().max()) <= 1e-12       # a reflection negates w
    assert float((R.winding(v[None], f, inside, xf) + R.winding(v[None], f, inside[:, [0, 2, 1]])).abs().max()) <= 1e-12


def test_cases_that_contribute_exactly_zero():
    v, f = R.box()
    one = lambda faces, x, verts=v: float(R.winding(verts[None], faces, torch.tensor([x], dtype=torch.float64)))
    assert one(f[:1], v[0].tolist()) == 0.0 and one(f[:1], v[3].tolist()) == 0.0             # a query on a vertex
    assert one(f[:1], [0.1, -0.05, -0.25]) == 0.0 and one(f[:1], [3.0, 7.0, -0.25]) == 0.0   # on the face's plane, in and out of it
    flat = torch.tensor([[0, 0, 0], [0, 1, 1], [2, 2, 0]])                                   # no area: repeated and collinear corners
    collinear = torch.tensor([[0.0, 0, 0], [0.25, 0.25, 0.25], [0.5, 0.5, 0.5]], dtype=torch.float64)
    assert all(one(flat[k:k + 1], [0.3, -0.2, 0.1]) == 0.0 for k in range(3))
    assert one(torch.tensor([[0, 1, 2]]), [0.3, -0.2, 0.1], collinear) == 0.0
    assert one(torch.tensor([[0, 1, 8], [-1, 2, 3], [0, 1 << 30, 2]]), [0.0, 0.0, 0.0]) == 0.0   # an index outside the mesh
    # such faces beside a closed cube change nothing, bit for bit
    x = torch.tensor([[0.0, 0.1, 0.2], [0.4, 0.0, 0.0]], dtype=torch.float64)
    extra = torch.cat([f, flat, torch.tensor([[0, 1, 8], [-1, 2, 3]])])
    assert torch.equal(R.winding(v[None], extra, x), R.winding(v[None], f, x))
    # a coordinate that is not finite makes w NaN
    assert math.isnan(one(f, [float('nan'), 0.0, 0.0])) and math.isnan(one(f, [float('inf'), 0.0, 0.0]))
    bad = v.clone()
    bad[7, 1] = float('inf')
    assert math.isnan(one(f, [0.0, 0.0, 0.0], bad)) and one(f[:1], [0.0, 0.0, 0.0], bad) != 0.0   # vertex 7 is not in face 0
    assert not bool((torch.tensor([float('nan')]) > 0.5).any())                               # NaN is outside


def test_two_boxes_on_the_16_grid_give_a_third():
    q = R.grid_queries(16)
    v, f = R.box()
    vb, _ = R.box((0.25, 0.0, 0.0))
    occ_a = (R.winding(v[None], f, q) > 0.5).to(torch.uint8)
    occ_b = (R.winding(vb[None], f, q) > 0.5).to(torch.uint8)
    rows, counts = R.iou_rows(occ_a, occ_b)
    assert counts.tolist() == [[256, 768, 512, 512]]
    assert rows[0].tolist() == [float(torch.tensor(1 / 3, dtype=torch.float64).float()), 0.5, 0.5, 0.125, 0.125]
    # the same from the primitives, and no centre is nearer than 1/32 to a boundary
    p = R.two_box_params()
    m = R.prim_m(p, (R.CUBOID, R.CUBOID), q)
    assert torch.equal((m[0, :, 0] <= 1).to(torch.uint8), occ_a[0]) and torch.equal((m[0, :, 1] <= 1).to(torch.uint8), occ_b[0])
    assert float((m * 0.25 - 0.25).abs().min()) >= 1 / 32 - 1e-12
    union, owner = R.prim_occupancy(p, (R.CUBOID, R.CUBOID), q)
    assert int(union.sum()) == 768 and int((owner == 0).sum()) == 512 and int((owner == 1).sum()) == 256
    # an empty union: every quotient over 0 is 0
    rows, counts = R.iou_rows(torch.zeros(1, 8, dtype=torch.uint8), torch.zeros(1, 8, dtype=torch.uint8))
    assert rows.tolist() == [[0.0] * 5] and counts.tolist() == [[0, 0, 0, 0]]


def test_bookkeeping_is_a_plain_loop():
    C = 3
    rows = [torch.arange(10, dtype=torch.float32).reshape(2, 5), torch.ones(1, 5)]
    cnt = [torch.tensor([[1, 2, 1, 2], [0, 0, 0, 0]]), torch.tensor([[1, 1, 1, 1]])]
    sums, counts = R.bookkeeping([(rows[0], cnt[0], [1, -1]), (rows[1], cnt[1], [1])], C)
    assert counts == [3, 2, 1, 1, 0, 2, 0]
    assert sums[:5] == [float(k + 5 + k + 1) for k in range(5)] and sums[10:15] == [float(k + 1) for k in range(5)]
    assert not any(sums[5:10]) and not any(sums[15:])
    assert R.state_tensor(sums, counts).numel() == (1 + C) * 5 + 4 + C


# ---- the host side of the meter

def _filled(C, k):
    from vpn_amd import ops
    state = ops.voliou_state(C, 'cpu')
    sums, counts = ops.voliou_state_fields(state, C)
    sums.copy_(torch.arange(sums.numel(), dtype=torch.float64) * 0.125 * k + k)
    counts.copy_(torch.tensor([3 * k + 1, k, 2, 1] + [k] * 3 + [0] * (C - 3)))
    return state


def test_state_merge_load_and_result_on_cpu():
    from vpn_amd import VolumeEvaluationMeter, ops
    import vpn_amd
    assert vpn_amd.modules.evaluation.VolumeEvaluationMeter is VolumeEvaluationMeter
    C, W = len(NAMES), 5
    meter = VolumeEvaluationMeter(NAMES, 'cpu', resolution=4)
    assert meter.state.numel() == (1 + C) * W + 4 + C and torch.equal(meter.queries, R.grid_queries(4))
    assert VolumeEvaluationMeter(NAMES, 'cpu', resolution=3, bounds=(0.0, 1.0)).queries.shape == (27, 3)
    own = VolumeEvaluationMeter(NAMES, 'cpu', queries=torch.zeros(7, 3))
    assert own.queries.shape == (7, 3) and own.resolution is None
    res = meter.result()
    assert res['iou'] is None and res['class_iou'] == [None] * C and res['n_samples'] == 0 and res['n_empty'] == 0
    a, b = _filled(C, 1), _filled(C, 2)
    merged = VolumeEvaluationMeter.merge(a, b)
    (sa, na), (sb, nb), (sm, nm) = (ops.voliou_state_fields(t, C) for t in (a, b, merged))
    assert torch.equal(sm, sa + sb) and torch.equal(nm, na + nb)
    meter.load_state(merged)
    assert torch.equal(meter.state, merged) and meter.state is not merged
    res = meter.result()
    n = 4 + 7
    tot = [float(v) / n for v in sm[:W]]
    assert (res['n_samples'], res['n_batches'], res['n_empty'], res['n_invalid'], res['class_n']) == (n, 3, 4, 2, [3, 3, 3, 0, 0])
    assert [res[k] for k in ('iou', 'precision', 'recall', 'vol_pred', 'vol_gt')] == tot
    c1 = [float(v) / 3 for v in sm[2 * W:3 * W]]
    assert [res['class_' + k][1] for k in ('iou', 'precision', 'recall', 'vol_pred', 'vol_gt')] == c1
    assert res['class_iou'][3] is None and res['class_vol_gt'][4] is None
    meter.reset()
    assert not meter.state.any() and meter.result()['n_batches'] == 0
    with pytest.raises(ValueError, match='not a volumetric evaluation state'):
        meter.load_state(a[:-1])
    with pytest.raises(ValueError, match='not a volumetric evaluation state'):
        ops.voliou_state_fields(a, C + 1)
    with pytest.raises(ValueError, match='merge needs'):
        VolumeEvaluationMeter.merge(a, b[:-1])
    with pytest.raises(ValueError):
        VolumeEvaluationMeter([], 'cpu')
    with pytest.raises(ValueError):
        VolumeEvaluationMeter(NAMES, 'cpu', queries=torch.zeros(7, 2))
    with pytest.raises(ValueError):
        VolumeEvaluationMeter(NAMES, 'cpu', resolution=0)
    with pytest.raises(ValueError):
        ops.voliou_state(0, 'cpu')


def test_report_prints_the_classes_that_occurred_then_the_total(capsys):
    from vpn_amd import VolumeEvaluationMeter
    meter = VolumeEvaluationMeter(NAMES, 'cpu', resolution=2)
    meter.load_state(_filled(len(NAMES), 1))
    res = meter.report(epoch=4)
    out = capsys.readouterr().out.splitlines()
    assert 'Epoch 4' in out and res == meter.result()
    rows = [l for l in out if 'volume iou = ' in l]
    assert [l.split()[0] for l in rows] == NAMES[:3] + ['total'] and all('vol_pred = ' in l and 'vol_gt = ' in l for l in rows)
    assert any(l.startswith('n_invalid = 1') for l in out) and any(l.startswith('n_empty = 2') for l in out)


def _one_rank(rank, port, out):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=0, world_size=1)
    from vpn_amd import VolumeEvaluationMeter
    meter = VolumeEvaluationMeter(NAMES, 'cpu', resolution=2)
    mine = _filled(len(NAMES), 2)
    meter.load_state(mine)
    res = meter.result(group=dist.group.WORLD)
    assert torch.equal(meter.state, mine)
    torch.save((res, meter.result()), out)
    dist.destroy_process_group()


def test_result_over_a_one_rank_group_equals_the_local_result(tmp_path):
    import vpn_amd
    out = str(tmp_path / 'r.pt')
    mp.spawn(_one_rank, args=(29500 + ((os.getpid() + 977) % 2000), out), nprocs=1, join=True)
    grouped, local = torch.load(out, weights_only=True)
    assert grouped == local and grouped['n_samples'] == 7 and grouped['n_empty'] == 2
    with pytest.raises(RuntimeError, match='initialised process group'):
        vpn_amd.dist.all_reduce_voliou_state(_filled(5, 1), 5)
    with pytest.raises(ValueError, match='not a volumetric evaluation state'):
        vpn_amd.dist.all_reduce_voliou_state(_filled(5, 1), 4)


# ---- the argument contract

def test_ops_contract_is_checked_before_any_launch():
    """On CPU tensors: one ValueError per rule, from shapes and dtypes alone; a valid call has no CPU path."""
    import vpn_amd
    from vpn_amd import VolumeEvaluationMeter, ops
    prm, kinds, q = torch.zeros(2, 3, 10), [1, 0, 0], torch.zeros(5, 3)
    with pytest.raises(ValueError, match=r'params must be float32 \[B,K,10\]'):
        ops.primitive_occupancy(prm[0], kinds, q)
    with pytest.raises(ValueError, match=r'params must be float32 \[B,K,10\]'):
        ops.primitive_occupancy(prm.double(), kinds, q)
    with pytest.raises(ValueError, match='2 kinds for 3 primitives'):
        ops.primitive_occupancy(prm, kinds[:2], q)
    with pytest.raises(ValueError, match='at most 1024 primitives'):
        ops.primitive_occupancy(torch.zeros(1, 1025, 10), [0] * 1025, q)
    with pytest.raises(ValueError, match=r'queries must be float32 \[Q,3\] or \[B,Q,3\]'):
        ops.primitive_occupancy(prm, kinds, q.double())
    with pytest.raises(ValueError, match=r'queries must be float32 \[Q,3\] or \[B,Q,3\]'):
        ops.primitive_occupancy(prm, kinds, q[:, :2])
    with pytest.raises(ValueError, match='must have B = 2'):
        ops.primitive_occupancy(prm, kinds, torch.zeros(3, 5, 3))
    with pytest.raises(ValueError, match='unknown primitive kind'):
        ops.primitive_occupancy(prm, [0, 1, 2], q)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.primitive_occupancy(prm, kinds, q)
    v, f = torch.zeros(2, 4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]])
    for fn in (ops.winding_number, ops.mesh_occupancy):
        with pytest.raises(ValueError, match=r'verts must be float32 \[B,P,3\]'):
            fn(v[0], f, q)
        with pytest.raises(ValueError, match=r'verts must be float32 \[B,P,3\]'):
            fn(v.double(), f, q)
        with pytest.raises(ValueError, match=r'faces must be \[F,3\]'):
            fn(v, f[:0], q)
        with pytest.raises(ValueError, match='faces must be int32 or int64'):
            fn(v, f.float(), q)
        with pytest.raises(ValueError, match='queries must be float32'):
            fn(v, f, q.half())
        with pytest.raises(ValueError, match='must have B = 2'):
            fn(v, f, torch.zeros(1, 5, 3))
        with pytest.raises(ValueError, match='xforms must be'):
            fn(v, f, q, torch.zeros(3, 3, 4))
        with pytest.raises(RuntimeError, match='GPU only'):
            fn(v, f, q)
    pv, vo, fo = torch.zeros(8, 3), torch.tensor([0, 4, 8], dtype=torch.int32), torch.tensor([0, 1, 2], dtype=torch.int32)
    rw = ops.ragged_winding_number
    with pytest.raises(ValueError, match='a MeshBatch or'):
        rw(pv, q)
    with pytest.raises(ValueError, match=r'verts must be float32 \[sumP,3\]'):
        rw((v, f, vo, fo, 1), q)
    with pytest.raises(ValueError, match='vert_offset must be an int32'):
        rw((pv, f, vo.long(), fo, 1), q)
    with pytest.raises(ValueError, match='S \\+ 1 entries each'):
        rw((pv, f, vo, fo[:2], 1), q)
    with pytest.raises(ValueError, match='max_faces must be 1 .. 2'):
        rw((pv, f, vo, fo, 3), q)
    with pytest.raises(ValueError, match='max_faces must be 1 .. 2'):
        rw((pv, f, vo, fo, 0), q)
    with pytest.raises(RuntimeError, match='GPU only'):
        rw((pv, f, vo, fo, 1), q)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.mesh_occupancy(vpn_amd.MeshBatch.pack([(pv[:4], f)]), None, q)
    C = 3
    state, cls = ops.voliou_state(C, 'cpu'), torch.zeros(2, dtype=torch.int32)
    a, b = torch.zeros(2, 9, dtype=torch.uint8), torch.ones(2, 9, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r'occ_pred must be uint8 \[B,Q\]'):
        ops.voliou_step(a.bool(), b, cls, state, C)
    with pytest.raises(ValueError, match=r'occ_gt must be uint8 \[B,Q\]'):
        ops.voliou_step(a, b[0], cls, state, C)
    with pytest.raises(ValueError, match='one shape'):
        ops.voliou_step(a, b[:, :8], cls, state, C)
    with pytest.raises(ValueError, match='agree on the batch size'):
        ops.voliou_step(a, b, cls[:1], state, C)
    with pytest.raises(ValueError, match='class_index must be an int32'):
        ops.voliou_step(a, b, cls.long(), state, C)
    with pytest.raises(ValueError, match='not a volumetric evaluation state'):
        ops.voliou_step(a, b, cls, state, C + 1)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.voliou_step(a, b, cls, state, C)
    assert not state.any()
    meter = VolumeEvaluationMeter(NAMES, 'cpu', resolution=2)
    with pytest.raises(RuntimeError, match='GPU only'):
        meter.update(a, b, [0, 1])
    with pytest.raises(TypeError, match='MeshBatch'):
        meter.update_primitives(prm, kinds, None, [0, 1])
    with pytest.raises(ValueError, match='1 ground-truth meshes for a batch of 2'):
        meter.update_mesh(v, f, vpn_amd.MeshBatch.pack([(pv[:4], f)]), [0, 1])
    for name in ('primitive_occupancy', 'winding_number', 'ragged_winding_number', 'mesh_occupancy', 'grid_queries', 'voliou_state',
                 'voliou_step'):
        assert getattr(vpn_amd, name) is getattr(ops, name), name
    assert vpn_amd.dist.all_reduce_voliou_state is not None


def test_plan_is_a_function_of_the_shape():
    from vpn_amd import ops
    assert ops.winding_plan(3, 257, 320) == (3, 107)                          # three slices, the last one short: 107 107 106
    assert ops.winding_plan(1, 257, 1280) == (10, 128)
    assert ops.winding_plan(1, 1, 12) == (1, 12) and ops.winding_plan(8, 32768, 4032) == (1, 4032)
    assert ops.winding_plan(64, 32768, 4032) == (1, 4032) and ops.winding_plan(1, 256, 100000) == (64, 1563)
    with pytest.raises(ValueError):
        ops.winding_plan(0, 1, 1)


def test_entries_were_added_without_an_abi_change():
    import vpn_amd._lib as lib
    L = lib.lib()
    assert L.vpn_abi_version() == lib.ABI_VERSION == 9
    for name in ('vpn_occupancy_prims', 'vpn_winding_workspace', 'vpn_winding_plan', 'vpn_winding_number', 'vpn_voliou_state_size',
                 'vpn_voliou_accumulate'):
        assert name in lib.SIGNATURES and hasattr(L, name), name
    H = lib.CONSTANTS
    assert H['VPN_OCCUPANCY_MAX_ITEMS'] == 1 << 24 and H['VPN_VOLIOU_WIDTH'] == 5 and H['VPN_OCCUPANCY_TILE'] == 256
    big = H['VPN_OCCUPANCY_MAX_ITEMS'] + 1
    size = L.vpn_voliou_state_size
    assert size(13) == ((1 + 13) * 5 + 4 + 13) * 8 and size(1) == (2 * 5 + 5) * 8
    assert size(0) == 0 and size(-1) == 0 and size(big) == 0
    ws = L.vpn_winding_workspace
    assert ws(3, 257, 320, 0, 0) == 3 * 3 * 257 * 8 + 8 + 3 * 320 * 48        # partial sums rounded up to 16 bytes, then the records
    assert ws(3, 300, 1412, 1, 1280) == 3 * 10 * 300 * 8 + 1412 * 48
    assert ws(0, 1, 1, 0, 0) == 0 and ws(1, 0, 1, 0, 0) == 0 and ws(1, 1, 0, 0, 0) == 0 and ws(1, 1, 4, 1, 0) == 0 and ws(1, 1, 4, 1, 5) == 0
    assert ws(65536, 1, 1, 0, 0) == 0 and ws(1, big, 1, 0, 0) == 0 and ws(1, 1, big, 0, 0) == 0
    assert L.vpn_winding_plan(0, 1, 1, None) == -1 and L.vpn_winding_plan(1, big, 1, None) == -2 and L.vpn_winding_plan(1, 1, 1, None) == 1
    # sizes and limits are looked at before any pointer is followed: host buffers stand in for device memory
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd8, odd16 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 8)
    assert p.value % 16 == 0

    def prims(params=p, kinds=p, queries=p, occ=p, owner=p, B=1, K=2, Q=4):
        return L.vpn_occupancy_prims(params, kinds, queries, 1, B, K, Q, occ, owner, None)

    for bad in (dict(params=None), dict(kinds=None), dict(queries=None), dict(occ=None, owner=None), dict(B=0), dict(K=0), dict(Q=0),
                dict(Q=-2)):
        assert prims(**bad) == -1, bad
    for too in (dict(B=65536), dict(Q=big), dict(K=H['VPN_MAX_PRIMS'] + 1)):
        assert prims(**too) == -2, too

    def wind(verts=p, faces=p, vo=None, fo=None, queries=p, B=1, Q=4, P=4, F=4, mf=4, work=p, nbytes=32768, w=p, occ=p):
        return L.vpn_winding_number(verts, faces, vo, fo, None, queries, 1, B, Q, P, F, mf, work, nbytes, w, occ, None)

    need = ws(1, 4, 4, 0, 0)
    for bad in (dict(verts=None), dict(faces=None), dict(queries=None), dict(work=None), dict(w=None, occ=None), dict(vo=p), dict(fo=p),
                dict(B=0), dict(Q=0), dict(P=0), dict(F=0), dict(vo=p, fo=p, mf=0), dict(vo=p, fo=p, mf=5), dict(nbytes=need - 1),
                dict(work=odd16), dict(F=-1)):
        assert wind(**bad) == -1, bad
    for too in (dict(B=65536), dict(Q=big), dict(P=big), dict(F=big), dict(vo=p, fo=p, F=big, mf=7)):
        assert wind(**too) == -2, too

    def acc(pred=p, gt=p, cls=p, B=1, Q=4, C=3, state=p, rows=p, counts=p):
        return L.vpn_voliou_accumulate(pred, gt, cls, B, Q, C, state, rows, counts, None)

    for bad in (dict(pred=None), dict(gt=None), dict(cls=None), dict(state=None), dict(rows=None), dict(counts=None), dict(state=odd8),
                dict(B=0), dict(Q=0), dict(C=0), dict(Q=-3)):
        assert acc(**bad) == -1, bad
    for too in (dict(B=65536), dict(Q=big), dict(C=big)):
        assert acc(**too) == -2, too
    assert not any(buf)                                                       # nothing was written


def test_kernels_use_no_scratch():
    from kernel_resources import load_build
    b = load_build()
    assert 'occupancy.hip' in b.SOURCES and b.PER_FILE['occupancy.hip'] == ['-ffp-contract=off']
    rows = kernel_resources('occupancy.hip')
    kernels = ('occ_prims_kernel', 'winding_prep_kernel', 'winding_kernel', 'winding_merge_kernel', 'voliou_sample_kernel',
               'voliou_book_kernel')
    for k in kernels:
        hits = [v for name, v in rows.items() if k in name]
        assert len(hits) == 1, (k, list(rows))
        assert hits[0]['ScratchSize'] == 0, (k, hits[0])
    assert len(rows) == len(kernels), list(rows)
    src = open(os.path.join(b.CSRC, 'occupancy.hip')).read()
    assert 'atomic' not in src.split('#include', 1)[1]                        # no atomics, no hand-off between workgroups


# ---- the conditioning of the GPU test's inputs

def _own(verts, faces, queries, xforms=None):
    w64 = R.winding(verts, faces, queries, xforms)
    w32 = R.winding(verts, faces, queries, xforms, dtype=torch.float32)
    return float((w32.double() - w64).abs().max()), w64


@pytest.mark.parametrize('name', ['cube', 'ico2', 'ico3'])
def test_queries_of_the_gpu_test_keep_their_distance(name):
    """(a) float64 distance >= 1e-3 from every triangle, (b) |w64 - 0.5| >= 0.05; volumes >= 0.05, coordinates within +-1."""
    c = R.mesh_case(name)
    verts, faces, q = c['verts'], c['faces'], c['queries']
    B = verts.shape[0]
    assert q.shape == {'cube': (1, 1, 3), 'ico2': (257, 3), 'ico3': (1, 257, 3)}[name]
    x = q[None].expand(B, -1, -1) if q.dim() == 2 else q
    d, m = R.mesh_margins(x, verts, faces)
    own, w64 = _own(verts, faces, q)
    print('%s: nearest triangle %.2e, |w - 0.5| >= %.3f, own %.2e, w off an integer by %.1e, inside %d of %d'
          % (name, float(d.min()), float(m.min()), own, float((w64 - w64.round()).abs().max()), int((w64 > 0.5).sum()), w64.numel()))
    assert float(d.min()) >= R.MIN_DISTANCE and float(m.min()) >= R.MIN_W_MARGIN
    assert float(verts.abs().max()) <= 1 and float(q.abs().max()) <= 1
    corners = verts.double()[:, faces]                                                        # [B,F,3,3]
    volume = (corners[:, :, 0] * torch.cross(corners[:, :, 1], corners[:, :, 2], dim=-1)).sum(-1).sum(-1) / 6
    assert float(volume.min()) >= 0.05
    assert own <= 2.5e-5                                                                       # a quarter of the 1e-4 bar
    if name != 'cube':
        inside = (w64 > 0.5).sum(-1)
        assert int(inside.min()) > 20 and int((w64.shape[-1] - inside).min()) > 20             # both decisions occur


def test_ragged_queries_of_the_gpu_test_keep_their_distance():
    c = R.ragged_case()
    assert c['queries'].shape == (3, 300, 3) and c['face_offset'].tolist() == [0, 12, 92, 1372]
    w64 = R.ragged_winding(c['verts'], c['faces'], c['vert_offset'], c['face_offset'], c['queries'], c['xforms'])
    w32 = R.ragged_winding(c['verts'], c['faces'], c['vert_offset'], c['face_offset'], c['queries'], c['xforms'], dtype=torch.float32)
    for s, (v, f) in enumerate(c['meshes']):
        d, m = R.mesh_margins(c['queries'][s:s + 1], v.float()[None], f, c['xforms'][s:s + 1])
        assert float(d.min()) >= R.MIN_DISTANCE and float(m.min()) >= R.MIN_W_MARGIN
        mapped = R._map(v[None], c['xforms'][s:s + 1].double())
        assert float(mapped.abs().max()) <= 1
        corners = mapped[:, f]
        volume = (corners[:, :, 0] * torch.cross(corners[:, :, 1], corners[:, :, 2], dim=-1)).sum(-1).sum(-1) / 6
        assert float(volume) >= 0.05
    own = float((w32.double() - w64).abs().max())
    print('ragged: own %.2e, inside %s of 300' % (own, (w64 > 0.5).sum(-1).tolist()))
    assert own <= 2.5e-5 and int((w64 > 0.5).sum(-1).min()) > 10


def test_primitive_queries_of_the_gpu_test_keep_their_margin():
    """(c) |m64 - 1| >= 1e-4 for every primitive; the fp32 restatement decides every one of them like float64."""
    c = R.prim_case()
    assert c['queries'].shape == (512 + 257, 3) and c['params'].shape == (3, 3, 10)
    m64, m32 = R.prim_m(c['params'], c['kinds'], c['queries']), R.prim_m(c['params'], c['kinds'], c['queries'], dtype=torch.float32)
    near = (m64 - 1).abs() < 0.1
    print('primitives: |m - 1| >= %.2e, fp32 error of m near the boundary %.2e, inside %s'
          % (float((m64 - 1).abs().min()), float((m32.double() - m64).abs()[near].max()), (m64 <= 1).any(-1).sum(-1).tolist()))
    assert float((m64 - 1).abs().min()) >= R.MIN_M_MARGIN
    assert float((m32.double() - m64).abs()[near].max()) <= R.MIN_M_MARGIN / 10                # more than tenfold headroom
    assert torch.equal(m32 <= 1, m64 <= 1)
    occ, owner = R.prim_occupancy(c['params'], c['kinds'], c['queries'])
    assert int(occ.sum(-1).min()) > 20 and all(int((owner == k).sum()) > 0 for k in (-1, 0, 1, 2))
    assert float(c['params'][:, :, 0:3].min()) >= 0.15 and float(c['queries'].abs().max()) <= 1
