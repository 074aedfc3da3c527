"""GPU tests of conv1 in factored form (ops.GcnFactoredInputFunction, GCNModel(factored_input=True), the gcn_factored_
kernels of csrc/gcn.hip) against the float64 restatement of tests/gcn_ref.py and against the plain path."""
import os
import subprocess
import sys

import pytest
import torch

import gcn_factored_ref as F
from conftest import ROOT, rel_err
from test_gcn import _model_case, _run_gpu, _run_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def vpn():
    import vpn_amd
    return vpn_amd


def _run_op(vpn, c, grads=('verts', 'glob', 'weight', 'maps')):
    """(h, dverts, dweight, dglob, [dmap]) of one forward + backward on the GPU; an input outside `grads` requires none."""
    v = c['verts'].to(DEV).requires_grad_('verts' in grads)
    w = c['weight'].to(DEV).requires_grad_('weight' in grads)
    g = c['glob'].to(DEV).requires_grad_('glob' in grads) if c['glob'] is not None else None
    mp = [m.to(DEV).requires_grad_('maps' in grads) for m in c['maps']]
    h = vpn.gcn_factored_input(v, c['bounds'].to(DEV), g, w, c['venc'], mp)
    (h * c['R'].to(DEV)).sum().backward()
    return h.detach(), v.grad, w.grad, g.grad if g is not None else None, [m.grad for m in mp]


@pytest.mark.parametrize('name', sorted(F.OP_CASES))
def test_op_against_float64(vpn, name):
    c = F.op_case(name)
    if name == 'corners_outside':
        out, inside = F.outside_fractions(c['verts'], c['bounds'], 32)
        assert out >= 0.2 and inside >= 0.2, (out, inside)
    h, dv, dw, dg, dm = _run_op(vpn, c)
    h64, dv64, dw64, dg64, dm64 = F.float64_reference(c)
    errs = dict(h=rel_err(h.cpu(), h64), dverts=rel_err(dv.cpu(), dv64), dweight=rel_err(dw.cpu(), dw64))
    if dg64 is not None:
        errs['dglobal'] = rel_err(dg.cpu(), dg64)
    for i, (a, b) in enumerate(zip(dm, dm64)):
        errs['dmap%d' % i] = rel_err(a.cpu(), b)
    print(name, errs)
    assert h.shape == h64.shape and dw.shape == c['weight'].shape and len(dm) == len(c['maps'])
    assert errs.pop('h') <= 1e-5
    for k, e in errs.items():
        assert e <= 1e-4, (k, e)
    # dverts again, split into the rows that hold an extent and the others (tests/gcn_input_ref.py): each element-wise, no
    # worse than 1e-3 nor than 4 x the error of the plain form evaluated in fp32 on the CPU
    import gcn_input_ref as G
    v32, w32 = c['verts'].clone().requires_grad_(True), c['weight'].clone()
    (F.plain(v32, c['bounds'], c['glob'], w32, c['venc'], c['maps']) * c['R']).sum().backward()
    masked = G.undecidable_rows(c['verts'], c['bounds'], c['maps']) if c['maps'] else torch.zeros(dv.shape[:2], dtype=torch.bool)
    rows = dict(masked=masked, extent=G.extent_rows(c['verts']))
    mine, own = G.split_errors(dv.cpu(), dv64, rows), G.split_errors(v32.grad, dv64, rows)
    print(name, 'dverts split (O, E): kernel %.2e %.2e, fp32 restatement %.2e %.2e' % (mine + own))
    assert mine[0] <= G.split_bar(own[0]) and mine[1] <= G.split_bar(own[1]), (mine, own)


def test_gradients_nobody_needs_are_skipped(vpn):
    c = F.op_case('small')
    full = _run_op(vpn, c)
    part = _run_op(vpn, c, grads=('verts', 'weight'))
    assert part[3] is None and all(m is None for m in part[4])
    assert torch.equal(part[0], full[0]) and torch.equal(part[1], full[1]) and torch.equal(part[2], full[2])
    only_w = _run_op(vpn, c, grads=('weight',))
    assert only_w[1] is None and torch.equal(only_w[2], full[2])
    only_v = _run_op(vpn, c, grads=('verts',))
    assert only_v[2] is None and torch.equal(only_v[1], full[1])


MODEL_CASES = {
    'small': dict(B=2, K=2, map_shapes=F.SMALL_MAPS, G=16, img=64, seed=3),
    'small_no_pe': dict(B=2, K=2, map_shapes=F.SMALL_MAPS, G=16, img=64, seed=3),
    'real_channels': dict(B=2, K=2, map_shapes=F.REAL_MAPS, G=512, img=128, seed=5),
}


def _factored_twin(model, args, use_pe):
    from vpn_amd.modules.gcn import GCNModel
    twin = GCNModel(img_feature_dim=sum(c for c, _ in args['map_shapes']) + args['G'], v_num=model.fc[0].in_features // 3,
                    use_position_encoding=use_pe, factored_input=True)
    twin.load_state_dict(model.state_dict())
    return twin


@pytest.mark.parametrize('case', sorted(MODEL_CASES))
def test_model_against_float64(vpn, case):
    args, use_pe = MODEL_CASES[case], case != 'small_no_pe'
    model, verts, faces, maps, glob, rgbs, Wout = _model_case(vpn, use_pe=use_pe, **args)
    twin = _factored_twin(model, args, use_pe)
    out = _run_gpu(vpn, twin, verts, faces, maps, glob, rgbs, Wout)
    ref = _run_ref(twin, verts, faces, maps, glob, rgbs, Wout, use_pe, masks=twin.relu_masks)
    assert rel_err(out[0] - verts, ref[0] - verts.double()) <= 1e-4            # the deformation, not the vertices
    assert abs(float(out[1]) - float(ref[1])) <= 1e-4 * abs(float(ref[1]))
    for k, gr in ref[2].items():
        assert rel_err(out[2][k], gr) <= 1e-4, k
    assert rel_err(out[3], ref[3]) <= 1e-4
    for a, b in zip(out[4], ref[4]):
        assert rel_err(a, b) <= 1e-4
    assert rel_err(out[5], ref[5]) <= 1e-4


def test_plain_and_factored_models_agree(vpn):
    """Each is within 1e-4 of the same float64 result, so they are within 2e-4 of each other."""
    args = MODEL_CASES['small']
    model, verts, faces, maps, glob, rgbs, Wout = _model_case(vpn, use_pe=True, **args)
    twin = _factored_twin(model, args, True)
    a = _run_gpu(vpn, model, verts, faces, maps, glob, rgbs, Wout)
    b = _run_gpu(vpn, twin, verts, faces, maps, glob, rgbs, Wout)
    assert rel_err(b[0] - verts, a[0] - verts) <= 2e-4
    assert abs(float(a[1]) - float(b[1])) <= 2e-4 * abs(float(a[1]))
    assert sorted(a[2]) == sorted(b[2])
    for k in a[2]:
        assert rel_err(b[2][k], a[2][k]) <= 2e-4, k
    assert rel_err(b[3], a[3]) <= 2e-4
    for p, q in zip(a[4], b[4]):
        assert rel_err(q, p) <= 2e-4
    assert rel_err(b[5], a[5]) <= 2e-4


def test_forward_and_backward_are_deterministic(vpn):
    c = F.op_case('real_channels')
    a, b = _run_op(vpn, c), _run_op(vpn, c)
    for p, q in zip(a[:4], b[:4]):
        assert torch.equal(p, q)
    for p, q in zip(a[4], b[4]):
        assert torch.equal(p, q)


def test_no_host_sync_and_graph_replay(vpn):
    c = F.op_case('small')
    dev = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    dev['maps'] = [m.to(DEV) for m in c['maps']]
    sv = dev['verts'].clone().requires_grad_(True)                # static inputs of the capture
    sw = dev['weight'].clone().requires_grad_(True)
    sg = dev['glob'].clone().requires_grad_(True)
    sm = [m.clone().requires_grad_(True) for m in dev['maps']]
    leaves = [sv, sw, sg] + sm

    def step():
        # only detached results leave: a kept autograd graph would keep the leaves' gradient accumulators, and with them
        # the stream they were made on; a backward captured later would then hand its gradients to that stream, a fork
        # out of the capture that nothing joins
        h = vpn.gcn_factored_input(sv, dev['bounds'], sg, sw, c['venc'], sm)
        return [h.detach()] + list(torch.autograd.grad((h * dev['R']).sum(), leaves))

    eager = [t.clone() for t in step()]                           # warm-up: library handles and workspaces
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        strict = step()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for p, q in zip(strict, eager):
        assert torch.equal(p, q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for p, q in zip(captured, eager):
        assert torch.equal(p, q)
    fresh = F.op_case('venc3')                                    # the same shapes except the weight's rows: take its other inputs
    with torch.no_grad():
        sv.copy_(fresh['verts'].to(DEV))
        sg.copy_(fresh['glob'].to(DEV))
        sw.mul_(-0.5)
        for m, f in zip(sm, fresh['maps']):
            m.copy_(f.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    again = step()
    for p, q in zip(replayed, again):
        assert torch.equal(p, q)
    assert not torch.equal(replayed[0], eager[0])


def test_train_gcn_step_example_runs_factored():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'train_gcn_step.py'), '--gcn-input', 'factored',
                        '--steps', '2'], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith('step ')]
    assert len(lines) == 2, r.stdout
    for l in lines:
        cd, emd = float(l.split('CD Loss = ')[1].split(',')[0]), float(l.split('EMD Loss = ')[1])
        assert cd == cd and emd == emd and abs(cd) < float('inf') and abs(emd) < float('inf'), l
