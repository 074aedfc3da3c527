"""CPU checks of the surface evaluation (SurfaceEvaluationMeter, ops.surfeval_step, ops.face_normals_at,
ops.ragged_face_normals, csrc/surfeval.hip): the restatement of tests/surfeval_ref.py against plain Python
loops, known answers, the host side of the meter on CPU states, the all-reduce on a one-rank gloo group, the argument contract
of ops and of the C entries, the kernels' resources and the conditioning of the inputs the GPU test uses."""
import ctypes
import math
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import meshreg_ref as M
import surfeval_ref as R
from conftest import ROOT
from kernel_resources import kernel_resources

NAMES = ['airplane', 'rifle', 'display', 'table', 'telephone']


# ---- the restatement against plain loops

def test_rows_equal_plain_loops():
    g = torch.Generator().manual_seed(3)
    B, N, M_, T = 2, 7, 5, 3
    d1, d2 = torch.rand(B, N, generator=g, dtype=torch.float64) * 0.1, torch.rand(B, M_, generator=g, dtype=torch.float64) * 0.1
    i1, i2 = torch.randint(-1, M_ + 1, (B, N), generator=g), torch.randint(-1, N + 1, (B, M_), generator=g)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g, dtype=torch.float64), dim=-1)
    n_pred, n_gt = unit(N), unit(M_)
    n_pred[0, 0] = 0                                                          # a zero normal adds 0, the denominator stays N
    thr2 = torch.tensor([0.002, 0.005, float(d1[0, 3]) ** 2], dtype=torch.float64)   # one threshold ON a squared distance: strictly below
    rows, counts = R.sample_rows(d1, i1, d2, i2, thr2, n_pred, n_gt)
    bare, _ = R.sample_rows(d1, i1, d2, i2, thr2)
    for b in range(B):
        want = R.rows_plain(d1[b].tolist(), i1[b].tolist(), d2[b].tolist(), i2[b].tolist(), thr2.tolist(), n_pred[b].tolist(),
                            n_gt[b].tolist())
        assert max(abs(x - y) for x, y in zip(rows[b].tolist(), want)) <= 1e-15
        assert [round(want[6 + t] * N) for t in range(T)] == counts[b, 0].tolist()
        assert [round(want[6 + T + t] * M_) for t in range(T)] == counts[b, 1].tolist()
        assert bare[b, 4:6].tolist() == [0.0, 0.0] and torch.equal(bare[b, 6:], rows[b, 6:])
    assert int(counts[0, 0, 2]) == int((d1[0] < d1[0, 3]).sum())            # the point on the threshold is a miss (x -> x * x is monotone)


def test_normals_equal_plain_loops_in_both_layouts():
    g = torch.Generator().manual_seed(4)
    verts = torch.rand(2, 6, 3, generator=g, dtype=torch.float64)
    faces = torch.tensor([[0, 1, 2], [2, 3, 4], [5, 0, 3], [1, 1, 4], [0, 7, 2], [-1, 2, 3]])
    fidx = torch.tensor([[0, 1, 2, 3, 4, 5, 6, -1], [2, 2, 1, 0, 5, 4, 3, 1]])
    xf = torch.randn(2, 3, 4, generator=g, dtype=torch.float64)
    for x in (None, xf):
        got = R.face_normals(verts, faces, fidx, x)
        for b in range(2):
            want = R.normals_plain(verts[b].tolist(), faces.tolist(), fidx[b].tolist(), None if x is None else x[b].tolist())
            assert (got[b] - torch.tensor(want, dtype=torch.float64)).abs().max() <= 1e-14
        assert not got[0, 3].any() and not got[0, 4].any() and not got[0, 5].any() and not got[0, 6].any() and not got[0, 7].any()
    # ragged: two meshes of different sizes, two sets, mesh-local indices
    v2, f2 = torch.rand(4, 3, generator=g, dtype=torch.float64), torch.tensor([[0, 1, 2], [1, 3, 2]])
    packed_v, packed_f = torch.cat([verts[0], v2]), torch.cat([faces[:3], f2])
    vo, fo = torch.tensor([0, 6, 10]), torch.tensor([0, 3, 5])
    fi = torch.tensor([[[0, 1, 2, 3], [2, 2, 0, -1]], [[0, 1, 1, 2], [1, 0, 0, 1]]])
    xr = torch.randn(2, 2, 3, 4, generator=g, dtype=torch.float64)
    got = R.ragged_normals(packed_v, packed_f, vo, fo, fi, 2, xr)
    for s, (v, f) in enumerate(((verts[0], faces[:3]), (v2, f2))):
        for t in range(2):
            want = R.normals_plain(v.tolist(), f.tolist(), fi[s, t].tolist(), xr[s, t].tolist())
            assert (got[s, t] - torch.tensor(want, dtype=torch.float64)).abs().max() <= 1e-14
    assert not got[0, 0, 3].any() and not got[1, 0, 3].any()                  # face 3 of a 3-face mesh, face 2 of a 2-face mesh


def test_bookkeeping_is_a_plain_loop():
    T, C = 1, 3
    rows = [torch.arange(18, dtype=torch.float32).reshape(2, 9), torch.ones(1, 9)]
    sums, counts = R.bookkeeping([(rows[0], [1, -1]), (rows[1], [1])], C, T)
    assert counts == [3, 2, 1, 0, 2, 0]
    assert sums[:9] == [float(k + 9 + k + 1) for k in range(9)] and sums[18:27] == [float(k + 1) for k in range(9)]
    assert not any(sums[9:18]) and not any(sums[27:])
    assert R.state_tensor(sums, counts).numel() == (1 + C) * 9 + 3 + C


# ---- known answers

def test_identical_clouds():
    p, _ = R.clouds('uniform')
    d1, i1, d2, i2 = R.brute_nn(p, p)
    n = torch.nn.functional.normalize(p.double(), dim=-1)
    rows, _ = R.sample_rows(d1.sqrt(), i1, d2.sqrt(), i2, R.thr2_of((0.01, 0.02)).double(), n, n)
    assert torch.equal(rows[:, :4], torch.zeros(3, 4, dtype=torch.float64))                # cd = 0
    assert (rows[:, 4:6] - 1).abs().max() <= 1e-15                                          # nc = 1
    assert torch.equal(rows[:, 6:], torch.ones(3, 6, dtype=torch.float64))                 # P = R = F = 1


def test_shifted_lattice():
    """A 4 x 4 x 4 lattice of spacing 0.1 shifted by delta = 0.03 < spacing / 2: every nearest distance is delta."""
    delta = 0.03
    k = torch.arange(4, dtype=torch.float64) * 0.1
    p = torch.stack(torch.meshgrid(k, k, k, indexing='ij'), -1).reshape(1, 64, 3)
    q = p + torch.tensor([delta, 0.0, 0.0], dtype=torch.float64)
    d1, i1, d2, i2 = R.brute_nn(p, q)
    assert (d1.sqrt() - delta).abs().max() <= 1e-15 and torch.equal(i1[0], torch.arange(64))
    rows, _ = R.sample_rows(d1.sqrt(), i1, d2.sqrt(), i2, torch.tensor([0.02 ** 2, 0.04 ** 2], dtype=torch.float64))
    T = 2
    assert rows[0, 6:6 + T].tolist() == [0.0, 1.0] and rows[0, 6 + T:6 + 2 * T].tolist() == [0.0, 1.0]
    assert rows[0, 6 + 2 * T:].tolist() == [0.0, 1.0]                         # F is 0, not NaN, when P + R = 0
    assert abs(float(rows[0, 2]) - delta) <= 1e-15 and abs(float(rows[0, 0]) - delta * delta) <= 1e-15   # cd_l1 and accuracy


def test_exact_normals():
    v = torch.tensor([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [5, 5, 5]]])
    f = torch.tensor([[0, 1, 2], [0, 1, 3], [4, 4, 4], [1, 0, 2]])
    for dtype in (torch.float32, torch.float64):
        n = R.face_normals(v, f, torch.tensor([[0, 1, 2, 3]]), dtype=dtype)
        assert n[0].tolist() == [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, -1.0]]


def test_mapped_mesh_has_the_normals_of_the_mapped_vertices():
    from vpn_amd.modules.dataset import view_center_xforms
    verts = R.mesh_vertices(1, 2)
    _, faces = R.icosphere(1)
    fidx = torch.arange(80)[None].repeat(2, 1)
    reflect = torch.tensor([[0.5, 0, 0, 0.1], [0, 0, 0.5, -0.2], [0, 0.5, 0, 0.3]], dtype=torch.float64)    # y and z swapped: det < 0
    xf = torch.stack([view_center_xforms([1.3], [25.0], [140.0])[0].double(), reflect])
    mapped = (xf[:, None, :, :3] * verts.double()[:, :, None, :]).sum(-1) + xf[:, None, :, 3]
    got, want = R.face_normals(verts, faces, fidx, xf), R.face_normals(mapped, faces, fidx)
    assert (got - want).abs().max() <= 1e-13
    plain = R.face_normals(verts, faces, fidx)
    # a rotation with a uniform scale turns the normal; the reflection flips its sign against the turned one
    rot = xf[0, :, :3] * 1.3
    assert ((rot @ plain[0].T).T - got[0]).abs().max() <= 1e-6
    lin = reflect[:, :3]
    turned = torch.nn.functional.normalize((torch.linalg.inv(lin).T @ plain[1].T).T, dim=-1)
    assert (turned + got[1]).abs().max() <= 1e-12                            # sign flipped: det < 0; |dot| does not see it


# ---- the host side of the meter

def _filled(C, T, k):
    from vpn_amd import ops
    state = ops.surfeval_state(C, T, 'cpu')
    sums, counts = ops.surfeval_state_fields(state, C, T)
    sums.copy_(torch.arange(sums.numel(), dtype=torch.float64) * 0.125 * k + k)
    counts.copy_(torch.tensor([3 * k + 1, k, 1] + [k] * 3 + [0] * (C - 3)))
    return state


def test_state_merge_load_and_result_on_cpu():
    from vpn_amd import SurfaceEvaluationMeter, ops
    import vpn_amd
    assert vpn_amd.modules.evaluation.SurfaceEvaluationMeter is SurfaceEvaluationMeter
    C, T = len(NAMES), 2
    W = 6 + 3 * T
    meter = SurfaceEvaluationMeter(NAMES, 'cpu')
    assert meter.thresholds == [0.01, 0.02] and meter.T == T and meter.state.numel() == (1 + C) * W + 3 + C
    assert torch.equal(meter.thr2, torch.tensor([0.01 * 0.01, 0.02 * 0.02], dtype=torch.float64).float())
    res = meter.result()
    assert res['cd'] is None and res['fscore'] is None and res['class_cd'] == [None] * C and res['n_samples'] == 0
    a, b = _filled(C, T, 1), _filled(C, T, 2)
    merged = SurfaceEvaluationMeter.merge(a, b)
    sa, na = ops.surfeval_state_fields(a, C, T)
    sb, nb = ops.surfeval_state_fields(b, C, T)
    sm, nm = ops.surfeval_state_fields(merged, C, T)
    assert torch.equal(sm, sa + sb) and torch.equal(nm, na + nb)
    meter.load_state(merged)
    assert torch.equal(meter.state, merged) and meter.state is not merged
    res = meter.result()
    n = 4 + 7
    tot = [float(v) / n for v in sm[:W]]
    assert res['n_samples'] == n and res['n_batches'] == 3 and res['n_invalid'] == 2 and res['class_n'] == [3, 3, 3, 0, 0]
    assert res['accuracy'] == tot[0] and res['completeness'] == tot[1] and res['cd'] == tot[0] + tot[1]
    assert res['cd_l1'] == 0.5 * (tot[2] + tot[3]) and res['normal_consistency'] == 0.5 * (tot[4] + tot[5])
    assert res['precision'] == tot[6:8] and res['recall'] == tot[8:10] and res['fscore'] == tot[10:12]
    c1 = [float(v) / 3 for v in sm[2 * W:3 * W]]
    assert res['class_cd'][1] == c1[0] + c1[1] and res['class_fscore'][1] == c1[10:12] and res['class_recall'][1] == c1[8:10]
    assert res['class_cd'][3] is None and res['class_fscore'][4] is None and res['thresholds'] == [0.01, 0.02]
    meter.load_state(merged, has_normals=False)
    assert meter.result()['normal_consistency'] is None and meter.result()['class_normal_consistency'] == [None] * C
    meter.reset()
    assert not meter.state.any() and meter.result()['n_batches'] == 0
    with pytest.raises(ValueError, match='not a surface evaluation state'):
        meter.load_state(a[:-1])
    with pytest.raises(ValueError, match='not a surface evaluation state'):
        ops.surfeval_state_fields(a, C, 3)
    with pytest.raises(ValueError, match='merge needs'):
        SurfaceEvaluationMeter.merge(a, b[:-1])
    with pytest.raises(ValueError, match='merge needs'):
        SurfaceEvaluationMeter.merge(a, b, T=3)
    for bad in ((), tuple([0.01] * 9), (0.0,), (float('nan'),), (-0.01,)):
        with pytest.raises(ValueError):
            SurfaceEvaluationMeter(NAMES, 'cpu', thresholds=bad)
    with pytest.raises(ValueError):
        SurfaceEvaluationMeter([], 'cpu')


def test_report_prints_the_classes_that_occurred_then_the_total(capsys):
    from vpn_amd import SurfaceEvaluationMeter
    meter = SurfaceEvaluationMeter(NAMES, 'cpu')
    meter.load_state(_filled(len(NAMES), 2, 1))
    res = meter.report(epoch=4)
    out = capsys.readouterr().out.splitlines()
    assert 'Epoch 4' in out and res == meter.result()
    rows = [l for l in out if 'surface cd = ' in l]
    assert [l.split()[0] for l in rows] == NAMES[:3] + ['total'] and all('F@0.01 = ' in l and 'F@0.02 = ' in l for l in rows)
    assert any(l.startswith('n_invalid = 1') for l in out)


def _one_rank(rank, port, out):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=0, world_size=1)
    from vpn_amd import SurfaceEvaluationMeter
    meter = SurfaceEvaluationMeter(NAMES, 'cpu')
    mine = _filled(len(NAMES), 2, 2)
    meter.load_state(mine)
    res = meter.result(group=dist.group.WORLD)
    assert torch.equal(meter.state, mine)
    torch.save((res, meter.result()), out)
    dist.destroy_process_group()


def test_result_over_a_one_rank_group_equals_the_local_result(tmp_path):
    import vpn_amd
    out = str(tmp_path / 'r.pt')
    mp.spawn(_one_rank, args=(29500 + ((os.getpid() + 1431) % 2000), out), nprocs=1, join=True)
    grouped, local = torch.load(out, weights_only=True)
    assert grouped == local and grouped['n_samples'] == 7
    with pytest.raises(RuntimeError, match='initialised process group'):
        vpn_amd.dist.all_reduce_surfeval_state(_filled(5, 2, 1), 5, 2)
    with pytest.raises(ValueError, match='not a surface evaluation state'):
        vpn_amd.dist.all_reduce_surfeval_state(_filled(5, 2, 1), 4, 2)


# ---- the argument contract

def test_ops_contract_is_checked_before_any_launch():
    """On CPU tensors: one ValueError per rule, from shapes and dtypes alone; a valid call has no CPU path."""
    import vpn_amd
    from vpn_amd import SurfaceEvaluationMeter, ops
    v, f, fi = torch.zeros(2, 4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]]), torch.zeros(2, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match=r'verts must be \[B,P,3\]'):
        ops.face_normals_at(v[0], f, fi)
    with pytest.raises(ValueError, match='verts must be float32'):
        ops.face_normals_at(v.double(), f, fi)
    with pytest.raises(ValueError, match=r'faces must be \[F,3\]'):
        ops.face_normals_at(v, f[:0], fi)
    with pytest.raises(ValueError, match='faces must be int32 or int64'):
        ops.face_normals_at(v, f.float(), fi)
    with pytest.raises(ValueError, match='fidx must be int32'):
        ops.face_normals_at(v, f, fi.long())
    with pytest.raises(ValueError, match=r'fidx must be \[B,n\] with B = 2'):
        ops.face_normals_at(v, f, fi[:1])
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.face_normals_at(v, f, fi)
    pv, vo, fo, rfi = torch.zeros(8, 3), torch.tensor([0, 4, 8], dtype=torch.int32), torch.tensor([0, 1, 2], dtype=torch.int32), \
        torch.zeros(2, 2, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match=r'verts must be \[sumP,3\]'):
        ops.ragged_face_normals(v, f, vo, fo, rfi, 2)
    with pytest.raises(ValueError, match='vert_offset must be an int32'):
        ops.ragged_face_normals(pv, f, vo.long(), fo, rfi, 2)
    with pytest.raises(ValueError, match='S \\+ 1 entries each'):
        ops.ragged_face_normals(pv, f, vo, fo[:2], rfi, 2)
    with pytest.raises(ValueError, match=r'fidx must be \[S,sets,n\]'):
        ops.ragged_face_normals(pv, f, vo, fo, rfi, 1)
    with pytest.raises(ValueError, match='sets must be positive'):
        ops.ragged_face_normals(pv, f, vo, fo, rfi, 0)
    with pytest.raises(ValueError, match='xforms must be'):
        ops.ragged_face_normals(pv, f, vo, fo, rfi, 2, torch.zeros(2, 1, 3, 4))
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.ragged_face_normals(pv, f, vo, fo, rfi, 2)
    C, T = 3, 2
    state, thr2 = ops.surfeval_state(C, T, 'cpu'), torch.tensor([1e-4, 4e-4])
    p, q, cls = torch.zeros(2, 5, 3), torch.zeros(2, 6, 3), torch.zeros(2, dtype=torch.int32)
    step = lambda *a, **k: ops.surfeval_step(*a, **k)
    with pytest.raises(ValueError, match=r'predict_points must be \[B,n,3\]'):
        step(p[0], q, cls, state, C, thr2)
    with pytest.raises(ValueError, match='agree on the batch size'):
        step(p, q[:1], cls, state, C, thr2)
    with pytest.raises(ValueError, match='agree on the batch size'):
        step(p, q, cls[:1], state, C, thr2)
    with pytest.raises(ValueError, match='thr2 must be a float32'):
        step(p, q, cls, state, C, thr2.double())
    with pytest.raises(ValueError, match='1 .. 8 thresholds'):
        step(p, q, cls, state, C, torch.zeros(9))
    with pytest.raises(ValueError, match='not a surface evaluation state'):
        step(p, q, cls, state, C + 1, thr2)
    with pytest.raises(ValueError, match='come together'):
        step(p, q, cls, state, C, thr2, predict_normals=p)
    with pytest.raises(ValueError, match='gt_normals must be float32'):
        step(p, q, cls, state, C, thr2, predict_normals=p, gt_normals=p)
    with pytest.raises(ValueError, match='class_index must be an int32'):
        step(p, q, cls.long(), state, C, thr2)
    with pytest.raises(RuntimeError, match='GPU only'):
        step(p, q, cls, state, C, thr2)
    assert not state.any()
    meter = SurfaceEvaluationMeter(NAMES, 'cpu')
    with pytest.raises(ValueError, match='come together'):
        meter.update(p, q, [0, 1], gt_normals=q)
    with pytest.raises(RuntimeError, match='GPU only'):
        meter.update(p, q, [0, 1])
    with pytest.raises(RuntimeError, match='GPU only'):
        meter.update_mesh(v, f, q, [0, 1], seed=1)
    with pytest.raises(TypeError, match='MeshBatch'):
        vpn_amd.gt_normals(None, rfi)
    assert vpn_amd.surfeval_step is ops.surfeval_step and vpn_amd.face_normals_at is ops.face_normals_at
    assert vpn_amd.ragged_face_normals is ops.ragged_face_normals and vpn_amd.modules.gt_normals is vpn_amd.gt_normals


def test_entries_were_added_without_an_abi_change():
    import vpn_amd._lib as lib
    L = lib.lib()
    assert L.vpn_abi_version() == lib.ABI_VERSION == 9
    for name in ('vpn_surfeval_state_size', 'vpn_face_normals_at', 'vpn_surfeval_accumulate'):
        assert name in lib.SIGNATURES and hasattr(L, name), name
    H = lib.CONSTANTS
    assert H['VPN_SURFEVAL_MAX_THRESHOLDS'] == 8 and H['VPN_SURFEVAL_MAX_ITEMS'] == 1 << 24
    big = H['VPN_SURFEVAL_MAX_ITEMS'] + 1
    size = L.vpn_surfeval_state_size
    assert size(13, 2) == ((1 + 13) * 12 + 3 + 13) * 8 and size(1, 1) == (2 * 9 + 4) * 8 and size(5, 8) == (6 * 30 + 8) * 8
    assert size(0, 2) == 0 and size(-1, 2) == 0 and size(3, 0) == 0 and size(3, 9) == 0 and size(big, 1) == 0
    # sizes and limits are looked at before any pointer is followed: host buffers stand in for device memory
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)

    def normals(verts=p, faces=p, vo=None, fo=None, fidx=p, out=p, B=1, n=4, P=4, F=4, sets=1):
        return L.vpn_face_normals_at(verts, faces, vo, fo, fidx, None, B, n, P, F, sets, out, None)

    for bad in (dict(verts=None), dict(faces=None), dict(fidx=None), dict(out=None), dict(vo=p), dict(fo=p), dict(B=0), dict(n=0),
                dict(P=0), dict(F=0), dict(sets=0), dict(B=-1), dict(vo=p, fo=p, B=3, sets=2)):
        assert normals(**bad) == -1, bad
    for too in (dict(B=65536), dict(n=big), dict(P=big), dict(F=big), dict(vo=p, fo=p, P=big), dict(vo=p, fo=p, F=big)):
        assert normals(**too) == -2, too

    def accumulate(d1=p, i1=p, d2=p, i2=p, n_pred=None, n_gt=None, thr2=p, cls=p, B=1, N=4, M=4, T=2, C=3, state=p, rows=p):
        return L.vpn_surfeval_accumulate(d1, i1, d2, i2, n_pred, n_gt, thr2, cls, B, N, M, T, C, state, rows, None)

    for bad in (dict(d1=None), dict(i1=None), dict(d2=None), dict(i2=None), dict(thr2=None), dict(cls=None), dict(state=None),
                dict(rows=None), dict(n_pred=p), dict(n_gt=p), dict(state=odd), dict(B=0), dict(N=0), dict(M=0), dict(T=0), dict(C=0),
                dict(N=-3)):
        assert accumulate(**bad) == -1, bad
    for too in (dict(T=9), dict(B=65536), dict(N=big), dict(M=big), dict(C=big)):
        assert accumulate(**too) == -2, too
    assert not any(buf)                                                       # nothing was written


def test_kernels_use_no_scratch():
    from kernel_resources import load_build
    b = load_build()
    assert 'surfeval.hip' in b.SOURCES and b.PER_FILE['surfeval.hip'] == ['-ffp-contract=off'] == b.PER_FILE['evaluate.hip']
    rows = kernel_resources('surfeval.hip')
    kernels = ('surfeval_normals_kernel', 'surfeval_sample_kernel', 'surfeval_book_kernel')
    for k in kernels:
        hits = [v for name, v in rows.items() if k in name]
        assert len(hits) == 1, (k, list(rows))
        assert hits[0]['ScratchSize'] == 0, (k, hits[0])
    assert len(rows) == len(kernels), list(rows)
    src = open(os.path.join(b.CSRC, 'surfeval.hip')).read()
    assert 'atomic' not in src.split('#include', 1)[1]                        # no atomics, no hand-off between workgroups


# ---- the conditioning of the GPU test's inputs

def test_meshes_of_the_gpu_test_are_well_conditioned():
    """Every face has sin of its smallest angle >= 0.1 and edges >= 0.01: the fp32 cross product is then within a few
    2^-24 / sin of the float64 one, inside the 1e-5 bar of tests/test_surfeval.py.  strip_65 and the icospheres satisfy it;
    the uv_sphere and fan_70 generators (pole and hub slivers: sin 0.02) do not and are not used."""
    cases = [(R.mesh_vertices(1, 3), R.icosphere(1)[1]), (R.mesh_vertices(2, 3), R.icosphere(2)[1]),
             (R.mesh_vertices(1, 2), R.icosphere(1)[1]), (M.vertices('strip_65', 3), M.mesh('strip_65')[0])]
    for v, f in cases:
        s, e = R.face_shape(v, f)
        print('faces %d: smallest sin %.3f, shortest edge %.4f' % (f.shape[0], s, e))
        assert s >= 0.1 and e >= 0.01
        n32, n64 = R.face_normals(v, f, torch.arange(f.shape[0])[None].expand(v.shape[0], -1), dtype=torch.float32), \
            R.face_normals(v, f, torch.arange(f.shape[0])[None].expand(v.shape[0], -1))
        assert (n32.double() - n64).abs().max() <= 0.25e-5                    # the restatement in fp32: a quarter of the bar
    for name in ('uv_sphere', 'fan_70'):
        assert R.face_shape(M.vertices(name, 3), M.mesh(name)[0])[0] < 0.1


@pytest.mark.parametrize('kind', ['uniform', 'clustered'])
def test_thresholds_of_the_gpu_test_sit_in_gaps(kind):
    """No float64 nearest-neighbour distance of the test clouds lies within a relative 1e-5 of tau^2 (an fp32 scan is within
    a few 1e-7 of it, and float32(tau^2) within 6e-8), and every count lies strictly between 0 and the number of points."""
    p, q = R.clouds(kind)
    assert p.shape == (3, 257, 3) and q.shape == (3, 300, 3) and float(p.abs().max()) <= 0.5 and float(q.abs().max()) <= 0.5
    d1, _, d2, _ = R.brute_nn(p, q)
    taus = R.gap_thresholds(kind)
    assert len(taus) == 3 and taus[0] < taus[1] < taus[2]
    for tau, t2 in zip(taus, R.thr2_of(taus).tolist()):
        for d, n in ((d1, 257), (d2, 300)):
            gap = float(((d - tau * tau).abs() / (tau * tau)).min())
            counts = (d < tau * tau).sum(1)
            print('%s tau %.5f: nearest distance at a relative %.1e, counts %s of %d' % (kind, tau, gap, counts.tolist(), n))
            assert gap > 1e-5 and abs(t2 - tau * tau) <= 1e-7 * tau * tau
            assert int(counts.min()) > 0 and int(counts.max()) < n
            assert torch.equal(counts, (d < t2).sum(1))
