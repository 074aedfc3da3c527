"""Time the GCN refinement stage on one GPU: every new kernel (the library's own per-launch events), each stage against
the torch composition of the same maths (grid_sample, index_add_, cat), and the whole GCNModel step split into the new
kernels and the rest (hipBLASLt GEMMs, fc, optimizer-free).  B = 8, N = 16 x 128, the ResNet-18 feature shapes of a
128 x 128 image.  Medians of --reps hipEvent-timed repetitions, ours and torch's alternating.

    python tools/time_gcn.py [--reps 50] [--out time_gcn.json]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vpn_amd  # noqa: E402
from vpn_amd import ops, _lib  # noqa: E402
from vpn_amd.modules.gcn import GCNModel  # noqa: E402
from vpn_amd.modules.meshing import TriangleMesh, uv_sphere  # noqa: E402

DEV = 'cuda'
HBM = 8.0e12


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def alternate(pairs, reps):
    """{name: (ours, torch)} -> {name: [median us ours, median us torch]}, ours and torch interleaved per repetition."""
    out = {k: [[], []] for k in pairs}
    for k, (f, g) in pairs.items():
        f(); g()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fs in pairs.items():
            for i, f in enumerate(fs):
                out[k][i].append(timed(f, 1))
    return {k: [statistics.median(v[0]), statistics.median(v[1])] for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default='time_gcn.json')
    args = ap.parse_args()
    torch.manual_seed(0)
    B, K = 8, 16
    sv, sf = uv_sphere()
    verts = torch.cat([sv[None] * (torch.rand(B, 1, 3) * 0.2 + 0.1) + (torch.rand(B, 1, 3) - 0.5) * 0.6 for _ in range(K)], 1).to(DEV)
    faces = torch.cat([sf + 128 * k for k in range(K)]).to(DEV)
    N = verts.shape[1]
    maps = [torch.randn(B, c, s, s, device=DEV) for c, s in [(64, 32), (128, 16), (256, 8), (512, 4)]]
    glob = torch.randn(B, 512, device=DEV)
    rgbs = torch.zeros(B, 3, 128, 128, device=DEV)
    rgbs[:, :, 20:100, 12:116] = torch.rand(B, 3, 80, 104, device=DEV)
    graph = ops.gcn_graph(faces, N, DEV)
    src = torch.cat([graph.col.long()])
    dst = torch.repeat_interleave(torch.arange(N, device=DEV), (graph.row_ptr[1:] - graph.row_ptr[:-1]).long())
    wts = graph.w
    ctot = 39 + 960 + 512
    g_in = torch.randn(B, N, ctot, device=DEV)
    h = torch.randn(B, N, 512, device=DEV)
    bias = torch.zeros(512, device=DEV)
    g512 = torch.randn(B, N, 512, device=DEV)
    bounds = ops.gcn_bounds(rgbs)

    # ---- ours
    def k_bounds():
        ops.gcn_bounds(rgbs)

    def k_input_fwd():
        return ops.GcnInputFunction.apply(verts, bounds, glob, 39, *maps)

    vg = verts.clone().requires_grad_(True)
    mg = [m.clone().requires_grad_(True) for m in maps]
    gg = glob.clone().requires_grad_(True)

    def k_input_fb():
        x = ops.GcnInputFunction.apply(vg, bounds, gg, 39, *mg)
        x.backward(g_in)

    def k_agg_fwd():
        return ops.GcnAggregateFunction.apply(h, bias, graph.row_ptr, graph.col, graph.w, True)

    hg = h.clone().requires_grad_(True)
    bg = bias.clone().requires_grad_(True)

    def k_agg_fb():
        ops.GcnAggregateFunction.apply(hg, bg, graph.row_ptr, graph.col, graph.w, True).backward(g512)

    # ---- torch composition of the same maths
    def t_input(v, m, g):
        zmax, zmin = v[..., 2].max(1, keepdim=True)[0], v[..., 2].min(1, keepdim=True)[0]
        ymax, ymin = v[..., 1].max(1, keepdim=True)[0], v[..., 1].min(1, keepdim=True)[0]
        bd = bounds[:, None, :]
        gx = bd[..., 0] + (1 - (v[..., 2] - zmin) / (zmax - zmin)) * (bd[..., 1] - bd[..., 0])
        gy = bd[..., 2] + (1 - (v[..., 1] - ymin) / (ymax - ymin)) * (bd[..., 3] - bd[..., 2])
        grid = torch.stack([gx, gy], -1)[:, None]
        pooled = torch.cat([F.grid_sample(x, grid, align_corners=True) for x in m], 1)[:, :, 0].permute(0, 2, 1)
        enc = [v] + [f(v * float(2 ** k)) for k in range(6) for f in (torch.sin, torch.cos)]
        return torch.cat(enc + [pooled, g[:, None, :].repeat(1, N, 1)], 2)

    def t_input_fwd():
        return t_input(verts, maps, glob)

    def t_input_fb():
        t_input(vg, mg, gg).backward(g_in)

    def t_agg(x, b):
        out = torch.zeros_like(x).index_add_(1, dst, x[:, src] * wts[None, :, None])
        return (out + b).relu()

    def t_agg_fwd():
        return t_agg(h, bias)

    def t_agg_fb():
        t_agg(hg, bg).backward(g512)

    def t_bounds():
        imgs = rgbs
        m = imgs.sum(1) > 0.03
        xs, ys = m.any(1), m.any(2)
        i = torch.arange(128, device=DEV)
        big = torch.full_like(i, 1 << 20)
        out = []
        for occ in (xs, ys):
            lo = torch.where(occ & (i >= 1), i, big).min(1)[0]
            hi = torch.where(occ, i, -big).max(1)[0]
            out += [torch.where(lo == big[0], 0, lo), torch.where(hi < 0, 128, hi)]
        return torch.stack(out, 1).float() / 128 * 2 - 1

    res = alternate({'bounds': (k_bounds, t_bounds), 'input_fwd': (k_input_fwd, t_input_fwd),
                     'input_fwd_bwd': (k_input_fb, t_input_fb), 'aggregate512_fwd': (k_agg_fwd, t_agg_fwd),
                     'aggregate512_fwd_bwd': (k_agg_fb, t_agg_fb)}, args.reps)

    # ---- per-kernel device times (the library's launch profile) over the same calls
    with _lib.KernelProfile() as kp:
        for _ in range(args.reps):
            k_bounds(); k_input_fb(); k_agg_fb()
            ops.GcnAggregateFunction.apply(h[..., :64].contiguous(), None, graph.row_ptr, graph.col, graph.w, False)
        torch.cuda.synchronize()
    kernels = {k: {'calls': c, 'mean_us': ms * 1e3} for k, (c, ms) in kp.summary().items()}

    # ---- the whole GCNModel step (forward + backward), and its split
    model = GCNModel().to(DEV)
    meshes = [TriangleMesh(verts[b], faces) for b in range(B)]
    mg2 = [m.clone().requires_grad_(True) for m in maps]

    def step():
        model.zero_grad(set_to_none=True)
        out = model(meshes, rgbs, mg2, glob)
        out.square().mean().backward()

    step()
    torch.cuda.synchronize()
    t_step = timed(step, args.reps)
    with _lib.KernelProfile() as kp:
        for _ in range(args.reps):
            step()
        torch.cuda.synchronize()
    ours_in_step = sum(c * ms for c, ms in kp.summary().values()) / args.reps * 1e3

    nbytes = {
        'gcn_bounds_kernel': B * 3 * 128 * 128 * 4 + B * 16,
        'gcn_input_kernel': B * N * ctot * 4 + B * N * 24 + B * 122880 * 4,
        'gcn_aggregate_kernel(C=512)': 2 * B * N * 512 * 4,
    }
    report = {'shape': dict(B=B, N=N, maps='64@32,128@16,256@8,512@4', G=512, ctot=ctot),
              'stages_median_us_ours_vs_torch': res, 'kernels': kernels, 'bytes': nbytes,
              'step_median_us': t_step, 'step_new_kernels_us': ours_in_step, 'step_rest_us': t_step - ours_in_step}
    for k, (a, b) in res.items():
        print('%-22s ours %9.1f us   torch %9.1f us   x%.2f' % (k, a, b, b / a))
    for k, v in sorted(kernels.items()):
        print('%-28s %5d calls  %8.1f us' % (k, v['calls'], v['mean_us']))
    print('GCNModel step %.1f us: new kernels %.1f us, the rest (GEMMs, fc, elementwise) %.1f us'
          % (t_step, ours_in_step, t_step - ours_in_step))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(report, f, indent=1)


if __name__ == '__main__':
    main()
