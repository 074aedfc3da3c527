"""bench.py — render + Chamfer forward+backward images/s on MI355X (BASELINE.json metric).

A step = one pass of the hot path over one batch of synthetic input already resident in HBM:
  sampler fwd (Philox in-kernel, fresh draws every step) -> Chamfer(pred, gt) fwd -> raster fwd (silhouette+depth)
  -> L1(sil) + L1(depth) -> backward of all of it to d/d(v,q,t) [-> one RCCL collective on the gradients if N>1].
Workloads (config.workload):
  c3 (default, the headline): BASELINE configs[2]: B=64 per GPU, K=32 sphere primitives, 256x256, n=256 points per
     primitive (N=8192) vs M=2048 GT points.  With --global-batch G the batch is split G/N per rank (BASELINE
     configs[3] = C4: G=256, strong scaling) instead of 64 per rank (weak scaling).
  c2: BASELINE configs[1]: K=16, 128x128 silhouette+depth, B=32, raster fwd/bwd only.  A --full run
     of c3 also measures it and reports it under the key "c2" next to the C3 headline.

    python bench.py [--gpus N --steps K --warmup W] [--workload c2] [--global-batch 256] [--collective allreduce]
    python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR     # also writes the last timed step's outputs
    python bench.py --full ...                                           # the headline and everything measured next to it
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
Rank 0 prints ONE JSON line (contract in the task statement).  A plain run sets up, warms up, times the steps, writes
--dump-outputs and prints the headline (metric, value, unit, ms_per_step, dtype, config, ...).  Everything else -- hipEvent
windows, steady state, per-kernel times and rooflines, the multi-rank `dist` record, the CPU baseline and the parity
legs against the oracle, the C2 / C5 / EMD / primitive-kind side workloads -- runs only with --full.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP32_PEAK_TFLOPS = 157.3     # fp32 vector peak = fp32-input MFMA peak (MI355X_MICROARCH.md chip table)
F16_PEAK_TFLOPS = 2500.0     # dense fp16 / bf16 MFMA (MI355X_MICROARCH.md; not the 2:1-sparsity figure)
N_SIMD = 1024                # 256 CUs x 4 SIMD-32
PMC_FILE = os.path.join(ROOT, 'profiles', 'r04_pmc.json')     # written by tools/pmc_collect.py from rocprofv3 passes


def synth_inputs(B, K, M, seed, device):
    """SURVEY.md 8d synthetic inputs (seed 1234 = reference config.py:20)."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.rand(B, K, 3, generator=g) + 0.1) / torch.tensor([8.0, 10.0, 10.0])   # vpnet_one_resnet.py:71,84
    q = torch.rand(B, K, 4, generator=g)                                               # sigmoid range (:72)
    t = 0.35 * (torch.rand(B, K, 3, generator=g) * 2 - 1)                              # tanh range (:73), inside the frustum
    gt_points = torch.rand(B, M, 3, generator=g) - 0.5                                 # dataset.py:165
    return torch.cat([v, q, t], 2).to(device), gt_points.to(device)


def event_windows(run, steps, windows):
    """Median / min / max over `windows` windows of `steps` calls each, timed with a HIP event pair on the current
    stream (the stream the step is launched on).  Returns milliseconds per step."""
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(steps):
            run(i)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return {'median': statistics.median(out), 'min': min(out), 'max': max(out), 'windows': windows, 'steps': steps}


def load_pmc(workload_key):
    """Counter summaries of the same command collected with rocprofv3 (tools/pmc_collect.py -> profiles/r04_pmc.json):
    {kernel: {counter: mean per dispatch}} for this workload, or {}."""
    try:
        return json.load(open(PMC_FILE)).get(workload_key, {})
    except (OSError, ValueError):
        return {}


def load_isa_mix():
    """Static issue-class mix of the raster kernels (tools/isa_mix.py -> profiles/r04_isa_mix.json)."""
    try:
        return json.load(open(os.path.join(ROOT, 'profiles', 'r04_isa_mix.json')))
    except (OSError, ValueError):
        return {}


def valu_issue_roofline(name, pmc, launch_us):
    """Executed-work roofline of a VALU-bound kernel: wave-instructions actually issued (PMC SQ_INSTS_VALU) x their
    issue cost / (launch time x SIMDs x clock).  Two prices: (a) every instruction at the plain rate the guide gives
    (2 cycles per wave64 instruction per SIMD) -- a lower bound of the utilisation; (b) class-weighted with the
    kernel's static ISA mix and the issue costs MEASURED on this chip (tools/ubench/valu_rates2.hip: plain 2.5,
    v_min/max/cmp/cndmask/DPP/SGPR-operand 4.3, transcendental 8.3 cycles; gfx950 has no counter that splits
    SQ_INSTS_VALU by class)."""
    k = pmc.get(name)
    if not k or 'SQ_INSTS_VALU' not in k:
        return None
    valu = k['SQ_INSTS_VALU']
    clock = 2.4e9
    avail = launch_us * 1e-6 * clock * N_SIMD
    out = {'valu_wave_insts': valu, 'issue_cycles_plain_price': 2.0 * valu,
           'frac_of_valu_issue_peak_at_2.4GHz': round(2.0 * valu / avail, 4)}
    mix = load_isa_mix().get(name)
    if mix:
        out['isa_mix'] = {c: round(v, 3) for c, v in mix['mix'].items()}
        out['cycles_per_valu_measured_classes'] = round(mix['cycles_per_valu'], 2)
        out['frac_of_measured_valu_issue_capacity'] = round(valu * mix['cycles_per_valu'] / avail, 4)
    if 'GRBM_GUI_ACTIVE' in k:      # sum over the 8 XCDs of active cycles -> the clock the launch actually ran at
        eff = k['GRBM_GUI_ACTIVE'] / 8.0 / (launch_us * 1e-6)
        out['effective_clock_GHz'] = round(eff / 1e9, 3)
    for c in ('SQ_INSTS_SALU', 'SQ_WAVES', 'SQ_WAIT_INST_ANY', 'SQ_WAVE_CYCLES', 'SQ_BUSY_CYCLES'):
        if c in k:
            out[c] = k[c]
    return out


def traffic_of(name, pmc):
    """HBM bytes per launch from the FETCH_SIZE / WRITE_SIZE passes (KB), corrected as the guide prescribes: FETCH_SIZE
    doubled for kernels whose reads are 16-B-per-lane coalesced streams (flagged per kernel by tools/pmc_collect.py)."""
    k = pmc.get(name)
    if not k or 'FETCH_SIZE' not in k or 'WRITE_SIZE' not in k:
        return None
    mul = 2.0 if k.get('fetch_doubled') else 1.0
    return int((k['FETCH_SIZE'] * mul + k['WRITE_SIZE']) * 1024)


def raster_only(vpn_amd, _lib, dev, B, K, H, steps, warmup, windows, pmc_key, use_graph=True, full=True):
    """C2: vpn_raster_loss_fwd + vpn_raster_loss_bwd alone (render, L1 silhouette + L1 depth, gradient to (v,q,t)),
    HIP-graph replay, hipEvent timing; with `full`, per-kernel times from the library's launch profiler and rooflines."""
    W = H
    kinds = vpn_amd.kinds_tensor([vpn_amd.SPHERE] * K, dev)
    params, _ = synth_inputs(B, K, 8, 1234, dev)
    params.requires_grad_(True)
    cam = torch.tensor([[1.0, 0.0, 0.0]], device=dev).expand(B, 3).contiguous()
    p2, _ = synth_inputs(B, K, 8, 4321, dev)
    sigma, gamma, z_far = vpn_amd.config.RASTER_SIGMA, vpn_amd.config.RASTER_GAMMA, vpn_amd.config.RASTER_Z_FAR
    with torch.no_grad():
        a2, d2 = vpn_amd.RasterFunction.apply(p2, kinds, cam, H, W, sigma, gamma, z_far)
    gt_sil, gt_depth = (a2 > 0.5).float(), d2.clone()
    one = torch.ones((), device=dev)

    def compute(_i=0):
        # total_img = SilhouetteLoss(L1) + L1 depth loss and its gradient to (v,q,t): the raster part of the C3 step
        params.grad = None
        out = vpn_amd.RasterTotalFunction.apply(params, kinds, cam, gt_sil, gt_depth, H, W, sigma, gamma, z_far, False, 1.0, 1.0)
        out[2].backward(one)
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            compute()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    run = compute
    if use_graph:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            compute()
        run = lambda i=0: graph.replay()
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    ev = event_windows(run, steps, windows)
    ms = ev['median']
    res = {'workload': 'C2: B=%d, K=%d sphere primitives, %dx%d silhouette+depth, raster fwd+bwd only '
                       '(vpn_raster_total_fwd/bwd: render + L1(sil) + L1(depth) + gradient to (v,q,t))' % (B, K, H, W),
           'images_per_s': round(B / ms * 1e3, 1), 'ms_per_step': round(ms, 5), 'timing': ev}
    if not full:
        return res
    ksteps = 20
    with _lib.KernelProfile() as kp:
        for _ in range(ksteps):
            compute()
    kern = kp.summary()
    kernel_us = {k: {'calls_per_step': round(v[0] / ksteps, 2), 'avg_us': round(v[1] * 1e3, 2)} for k, v in kern.items()}
    fwd_b, bwd_b = B * (40 * K + 8 * H * W), B * (8 * H * W + 80 * K)
    pmc = load_pmc(pmc_key)
    roof = {}
    for name, alg in (('raster_total_kernel', fwd_b + bwd_b), ('raster_fwd_kernel<1>', fwd_b), ('raster_bwd_kernel<1>', bwd_b)):
        if name not in kern:
            continue
        us = kern[name][1] * 1e3
        gbs = alg / (us * 1e-6) / 1e9
        roof[name] = {'avg_launch_us': round(us, 2), 'algorithmic_bytes_per_launch': alg,
                      'hbm': {'bound': 'hbm', 'achieved': round(gbs, 2), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                              'frac': round(gbs / HBM_PEAK_GBS, 5), 'traffic': traffic_of(name, pmc)},
                      'executed_work': valu_issue_roofline(name, pmc, us)}
    res.update({'algorithmic_bytes_per_image': (fwd_b + bwd_b) // B, 'kernel_us': kernel_us, 'roofline': roof,
                'pmc_source': os.path.relpath(PMC_FILE, ROOT) if pmc else None})
    return res


def c5_inputs(vpn_amd, B, K, n, H, dev, gt_mode='uniform'):
    """Synthetic batch of the reference's training step (train.py:227-262) at a given shape: packed primitive parameters,
    view-centred GT points (M = K*n: the only shape emd_module.py:36-39 admits), their object-centred counterpart
    (dataset.py:165 stores both; here canonical = view_to_obj_points(view_center)), the dataset's camera values, and a GT
    silhouette rendered from a second primitive set.
    gt_mode 'uniform' (SURVEY.md 8d's inputs): GT cloud uniform in the cube, predicted primitives unrelated to it -- what the
    first iterations of a training run look like, and the hardest case for the auction (500-1500 bidders in every round).
    gt_mode 'surface': the GT cloud is sampled on the surfaces of a TARGET primitive set, the GT silhouette is its render, and
    the predicted primitives are the target's perturbed by 10 % -- a step of a run that has partly converged."""
    M = K * n
    params, gt_view = synth_inputs(B, K, M, 1234, dev)
    if gt_mode == 'surface':
        kinds_t = vpn_amd.kinds_tensor([vpn_amd.SPHERE] * K, dev)
        g2 = torch.Generator().manual_seed(99)
        target = params.clone()
        with torch.no_grad():
            gt_view = vpn_amd.Sampling.sample_primitives(target, kinds_t, n, seed=4321).contiguous()
        noise = torch.cat([1.0 + 0.1 * torch.randn(B, K, 3, generator=g2), torch.ones(B, K, 4), torch.ones(B, K, 3)], 2).to(dev)
        shift = torch.cat([torch.zeros(B, K, 3), 0.02 * torch.randn(B, K, 4, generator=g2), 0.02 * torch.randn(B, K, 3, generator=g2)], 2).to(dev)
        params = (target * noise + shift).contiguous()
    g = torch.Generator().manual_seed(77)
    dists = (1.0 + 0.5 * torch.rand(B, generator=g)).to(dev)          # rendering_metadata.txt: distance ratio (dataset.py:145-165)
    elevs = (20.0 + 20.0 * torch.rand(B, generator=g)).to(dev)        # degrees
    azims = (360.0 * torch.rand(B, generator=g)).to(dev)
    angles = torch.zeros(B, device=dev)                               # AUGMENT_3D['rotate'] = False (config.py:47)
    kinds = vpn_amd.kinds_tensor([vpn_amd.SPHERE] * K, dev)           # config.py:33-34: all spheres
    with torch.no_grad():
        gt_canon = vpn_amd.view_to_obj_points(gt_view, dists, elevs, azims, angles).contiguous()
        p2 = target if gt_mode == 'surface' else synth_inputs(B, K, 8, 4321, dev)[0]
        cam1 = torch.tensor([[1.0, 0.0, 0.0]], device=dev).expand(B, 3).contiguous()       # train.py:172-174
        a2, _ = vpn_amd.RasterFunction.apply(p2, kinds, cam1, H, H, vpn_amd.config.RASTER_SIGMA, vpn_amd.config.RASTER_GAMMA,
                                             vpn_amd.config.RASTER_Z_FAR)
    gt_sil = (a2 > 0.5).float().reshape(B, 1, H, H)
    return params, kinds, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles


C5_WEIGHTS = (1.0, 0.0, 1.0, 0.1, 1.0)      # L_VIEW_CD, L_CAN_CD, L_SIL, L_VP_DIV, L_EMD: config.py:13-17 with the render ON
# (config.py:15 has L_SIL = 0.0, for which train.py:167 returns before rendering; BASELINE config C5 names 256x256, so the
# silhouette term is evaluated here with weight 1; L_CAN_CD = 0 is the reference's value: that Chamfer is computed and weighted 0)


def train_step_block(vpn_amd, _lib, dev, B, K, n, H, steps, warmup, windows, form, with_oracle, gt_mode='uniform', use_graph=True,
                     full=True):
    """The step train.py:243-262 runs: sampler -> view-centred Chamfer + object-centred Chamfer through view_to_obj_points
    + silhouette loss + VP-diversity loss + EMD (eps 0.005, 50 rounds) -> weighted total -> backward to d/d(v,q,t).
    form 'modules': the drop-in module surface called the way train.py calls it (one autograd node per reference call);
    form 'fused': one autograd node, no ATen kernel inside the step (TrainStepLossFunction).
    With `full`, the losses come from a run under the library's launch profiler (`kernel_us`); without, from one step."""
    params, kinds, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles = c5_inputs(vpn_amd, B, K, n, H, dev, gt_mode)
    params.requires_grad_(True)
    w = C5_WEIGHTS
    ones, zeros = torch.ones(B, device=dev), torch.zeros(B, device=dev)
    cd, sil_f, div_f, emd_f = (vpn_amd.ChamferDistanceLoss(), vpn_amd.SilhouetteLoss(), vpn_amd.VPDiverseLoss(vp_num=K),
                               vpn_amd.EarthMoverDistanceLoss())
    one = torch.ones((), device=dev)
    seed_buf = torch.full((1,), 1234, dtype=torch.int64, device=dev)

    def step_modules(_i=0):
        params.grad = None
        volumes, rotates, translates = vpn_amd.split_primitives(params)
        pred = vpn_amd.Sampling.sample_primitives(params, kinds, n, seed=1234)                      # train.py:243
        view_cd = cd(pred, gt_view) * w[0]                                                           # :160
        obj_cd = cd(vpn_amd.view_to_obj_points(pred, dists, elevs, azims, angles), gt_canon) * w[1]  # :158-161
        sil = sil_f(vpn_amd.PrimitivePack(params, kinds), gt_sil, ones, zeros, zeros) * w[2]         # :169-176
        div = div_f(translates, gt_view) * w[3]                                                      # :185
        dist, _ = emd_f(pred, gt_view, 0.005, 50)                                                    # :193
        emd = torch.sqrt(dist).mean() * w[4]                                                         # :195
        total = view_cd + obj_cd + sil + div + emd                                                   # :260
        total.backward()
        return torch.stack([view_cd, obj_cd, sil, div, emd, total]).detach()

    def step_fused(_i=0):
        params.grad = None
        out = vpn_amd.TrainStepLossFunction.apply(params, kinds, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles, n,
                                                  seed_buf, 0, H, H, w, 0.005, 50, True)
        out[5].backward(one)
        return out

    compute = step_modules if form == 'modules' else step_fused
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(3):
            compute(i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    res = {'form': form}
    try:
        if not use_graph:
            raise RuntimeError('--no-graph')
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g_out = compute(0)
        run = lambda i=0: graph.replay()
        res['launch'] = 'hip-graph replay'
    except Exception as e:        # noqa: BLE001 -- e.g. a cooperative launch that cannot be captured
        torch.cuda.synchronize()
        res['launch'] = 'eager (graph capture failed: %s: %s)' % (type(e).__name__, str(e)[:200])
        run = compute
        g_out = None
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    ev = event_windows(run, steps, windows)
    ksteps = 10
    if full:
        with _lib.KernelProfile() as kp:
            for i in range(ksteps):
                out = compute(i)
        kern = kp.summary()
    else:
        out = compute(0)
    ms = ev['median']
    res.update({'workload': 'train.py:243-262 step: B=%d, K=%d spheres, n=%d pts/prim (N=M=%d), %dx%d, weights (view_cd, can_cd, sil, '
                            'vp_div, emd) = %s, EMD eps=0.005 iters=50; %s' % (B, K, n, K * n, H, H, (w,),
                            {'uniform': 'GT cloud uniform in the cube, unrelated predicted primitives (SURVEY 8d inputs: the first iterations of a run)',
                             'surface': 'GT cloud on the surfaces of a target primitive set, predicted primitives = the target perturbed by 10 % (a partly converged run)'}[gt_mode]),
                'ms_per_step': round(ms, 5), 'images_per_s': round(B / ms * 1e3, 1), 'timing': ev,
                'losses': dict(zip(('view_cd', 'obj_cd', 'sil', 'vp_div', 'emd', 'total'), [float(x) for x in out])),
                'finite_grad': bool(torch.isfinite(params.grad).all())})
    if full:
        res.update({'kernel_us': {k: {'calls_per_step': round(v[0] / ksteps, 2), 'avg_us': round(v[1] * 1e3, 2)} for k, v in kern.items()},
                    'kernel_us_sum_per_step': round(sum(v[0] * v[1] for v in kern.values()) / ksteps * 1e3, 1)})
    if with_oracle:
        res['parity_vs_oracle'] = c5_parity(vpn_amd, params.detach(), kinds, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles, K, n, H, w)
    return res, (params, kinds, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles)


def c5_parity(vpn_amd, params, kinds, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles, K, n, H, w, S=2):
    """The fused step node on S images against the CPU oracle (oracle.vpn_oracle.train_step: every term restated from the
    reference, the auction included), loss terms and gradient; host seed = the Philox key the oracle replays."""
    from oracle import vpn_oracle as O
    t0 = time.perf_counter()
    ref, gref = O.train_step(params[:S].cpu(), gt_view[:S].cpu(), gt_canon[:S].cpu(), gt_sil[:S].cpu(), dists[:S].cpu(), elevs[:S].cpu(),
                             azims[:S].cpu(), angles[:S].cpu(), [0] * K, n, H, H, w, 4242)
    cpu_s = time.perf_counter() - t0
    pg = params[:S].clone().requires_grad_(True)
    out = vpn_amd.TrainStepLossFunction.apply(pg, kinds, gt_view[:S].contiguous(), gt_canon[:S].contiguous(), gt_sil[:S].contiguous(),
                                              dists[:S].contiguous(), elevs[:S].contiguous(), azims[:S].contiguous(), angles[:S].contiguous(),
                                              n, 4242, 0, H, H, w)
    out[5].backward()
    got = torch.stack([o.detach() for o in out]).cpu()
    names = ('view_cd', 'obj_cd', 'sil', 'vp_div', 'emd', 'total')
    rel = {k: float('%.3g' % (abs(float(a) - float(b)) / max(abs(float(b)), 1e-12))) for k, a, b in zip(names, got, ref) if float(b) != 0.0}
    return {'images': S, 'loss_rel': rel, 'grad_rel': float('%.3g' % float((pg.grad.cpu() - gref).abs().max() / gref.abs().max())),
            'cpu_port_images_per_s': round(S / cpu_s, 3), 'tolerance': 1e-4}


def free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def launch_ranks(n, argv):
    """Start the n ranks of `bench.py --gpus n` as children (one process per GPU, torch.distributed.run on
    127.0.0.1) and wait for them.  Called before anything in this process has initialised the GPU; nothing is exec'd."""
    import subprocess
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n),
           '--master-addr', '127.0.0.1', '--master-port', str(free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')     # dmabuf IPC: RCCL needs it on this driver
    env.setdefault('OMP_NUM_THREADS', '4')
    # rank 0's JSON line is the only thing relayed to stdout (gloo / c10d chatter of the children goes to stderr)
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    for line in (proc.stdout or '').splitlines():
        print(line, file=sys.stdout if line.startswith('{"metric"') else sys.stderr, flush=True)
    return proc.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--workload', choices=['c3', 'c2', 'c5'], default='c3')
    ap.add_argument('--batch', type=int, default=None, help='samples per GPU (default 64 for c3, 32 for c2)')
    ap.add_argument('--global-batch', type=int, default=None,
                    help='fixed GLOBAL batch split evenly over the ranks (C4: 256): strong scaling')
    ap.add_argument('--prims', type=int, default=None)
    ap.add_argument('--points', type=int, default=256, help='sampled points per primitive')
    ap.add_argument('--kinds', choices=['spheres', 'cuboids', 'mixed'], default='spheres',
                    help='primitive kinds of the C3 workload: all spheres (reference default, config.py:33-34), all cuboids, or '
                         'half cuboids then half spheres (the order of train.py:112-116) -- SURVEY.md 8d secondary runs')
    ap.add_argument('--gt-points', type=int, default=2048)
    ap.add_argument('--size', type=int, default=None)
    ap.add_argument('--collective', choices=['allreduce', 'allgather'], default='allreduce',
                    help='the one gradient exchange per step when N>1 (north_star: RCCL all-reduce)')
    ap.add_argument('--windows', type=int, default=5, help='hipEvent windows of --steps replays each (median reported)')
    ap.add_argument('--full', action='store_true',
                    help='after the headline, also measure and check everything reported next to it (hipEvent windows, '
                         'steady state, per-kernel times and rooflines, CPU baseline, parity with the oracle, side workloads)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='--full: skip the CPU baseline and the oracle parity legs')
    ap.add_argument('--c5-form', choices=['modules', 'fused', 'both'], default='both')
    ap.add_argument('--c5-gt', choices=['uniform', 'surface'], default='uniform', help='GT cloud of the c5 workload (see c5_inputs)')
    ap.add_argument('--no-c5', action='store_true', help='--full: skip the C5 train-step measurement')
    ap.add_argument('--no-c2', action='store_true', help='--full: skip the C2 raster-only measurement')
    ap.add_argument('--no-extras', action='store_true', help='--full: skip C2, C5, EMD, the primitive-kind variants and the CPU '
                                                             'baseline (profiling runs)')
    ap.add_argument('--no-graph', action='store_true', help='launch every step eagerly instead of replaying a HIP graph')
    ap.add_argument('--dist-selftest', action='store_true',
                    help='run the multi-rank code path (RCCL group, gradient collective) even with one rank')
    ap.add_argument('--cpu-sample', type=int, default=32, help='images in the CPU baseline sample')
    ap.add_argument('--rehearse', action='store_true',
                    help='rehearsal of the N>1 code path on a ONE-GPU box: every rank uses cuda:0 and the process group '
                         'is gloo instead of RCCL (which refuses two ranks on one device); not a measurement')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step of the headline workload returned (gradient and losses) to '
                         'DIR/<name>.npy, so that two builds can be compared output for output')
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')
    if args.dump_outputs and args.workload != 'c3':
        ap.error('--dump-outputs is implemented for the headline workload (c3) only')
    if args.no_extras:
        args.no_cpu_baseline = args.no_c2 = True

    if 'WORLD_SIZE' not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` by itself: this process becomes the launcher.  It has not touched the GPU (no
        # torch.cuda call, vpn_amd not imported) and never does; the N ranks are CHILD processes started through
        # torch.distributed.run, their output is relayed and the worst return code is returned.
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))

    import torch.distributed as dist
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    args.gpus = world
    if args.rehearse:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    multi = world > 1 or args.dist_selftest
    if multi:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29511')
        if args.rehearse:
            dist.init_process_group('gloo', rank=rank, world_size=world)
        else:
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)

    import vpn_amd
    from vpn_amd import _lib
    from vpn_amd.dist import GradAllGather, GradAllReduce
    _lib.lib()

    if args.workload == 'c2':
        B = args.batch or 32
        res = raster_only(vpn_amd, _lib, dev, B, args.prims or 16, args.size or 128, args.steps, args.warmup,
                          args.windows, 'c2', not args.no_graph, args.full)
        if rank == 0:
            out = {'metric': 'raster fwd+bwd images/sec (BASELINE config C2)', 'value': res['images_per_s'],
                   'unit': 'images/s', 'n_gpus': 1, 'steps': args.steps, 'warmup': args.warmup,
                   'ms_per_step': res['ms_per_step'], 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
                   'dtype': 'f32', 'data': 'synthetic', 'launch': 'eager' if args.no_graph else 'hip-graph replay',
                   'config': {'workload': res['workload'], 'global_batch': B, 'parallelism': 'dp1'}}
            if args.full:
                domk = max(res['roofline'], key=lambda k: res['roofline'][k]['avg_launch_us'])
                dom = res['roofline'][domk]
                out['roofline'] = dict(dom.get('hbm', {}), kernel=domk, executed_work=dom.get('executed_work'))
            out['c2'] = res
            print(json.dumps(out), flush=True)
        if multi:
            dist.destroy_process_group()
        return

    if args.workload == 'c5':
        forms = [args.c5_form] if args.c5_form != 'both' else ['modules', 'fused']
        res = {f: train_step_block(vpn_amd, _lib, dev, args.batch or 64, args.prims or 64, args.points if args.points != 256 else 32,
                                   args.size or 256, args.steps, args.warmup, args.windows, f,
                                   args.full and f == 'fused' and not args.no_cpu_baseline, args.c5_gt, not args.no_graph, args.full)[0]
               for f in forms}
        if rank == 0:
            best = min(res.values(), key=lambda r: r['ms_per_step'])
            print(json.dumps({'metric': 'train.py step (5 losses) images/sec (BASELINE config C5, one GPU)', 'value': best['images_per_s'],
                              'unit': 'images/s', 'n_gpus': 1, 'steps': args.steps, 'warmup': args.warmup,
                              'ms_per_step': best['ms_per_step'], 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
                              'dtype': 'f32', 'data': 'synthetic', 'config': {'workload': best['workload']}, 'c5': res}), flush=True)
        if multi:
            dist.destroy_process_group()
        return

    K, n, M, H = args.prims or 32, args.points, args.gt_points, args.size or 256
    W = H
    if args.global_batch:
        assert args.global_batch % world == 0, '--global-batch must divide evenly over the ranks'
        B = args.global_batch // world
        scaling = 'strong'
    else:
        B = args.batch or 64
        scaling = 'weak'
    Bg = B * world
    kinds_list = {'spheres': [vpn_amd.SPHERE] * K, 'cuboids': [vpn_amd.CUBOID] * K,
                  'mixed': [vpn_amd.CUBOID] * (K // 2) + [vpn_amd.SPHERE] * (K - K // 2)}[args.kinds]
    kinds = vpn_amd.kinds_tensor(kinds_list, dev)               # reference default: all spheres (config.py:33-34)
    # rank r owns global samples [r*B, (r+1)*B)
    params_all, gt_all = synth_inputs(Bg, K, M, 1234, dev)
    params = params_all[rank * B:(rank + 1) * B].clone().requires_grad_(True)
    gt_points = gt_all[rank * B:(rank + 1) * B].contiguous()
    cam = torch.tensor([[1.0, 0.0, 0.0]], device=dev).expand(B, 3).contiguous()    # train.py:172-174
    # GT silhouette / depth of the timed run: render of a second primitive set (seed 4321), silhouette thresholded
    # at 0.5.  (The parity leg below builds its GT with the CPU oracle instead, so that it does not depend on the
    # kernel under test.)
    p2_all, _ = synth_inputs(Bg, K, M, 4321, dev)
    sigma, gamma, z_far = vpn_amd.config.RASTER_SIGMA, vpn_amd.config.RASTER_GAMMA, vpn_amd.config.RASTER_Z_FAR
    with torch.no_grad():
        a2, d2 = vpn_amd.RasterFunction.apply(p2_all[rank * B:(rank + 1) * B].contiguous(), kinds, cam, H, W, sigma, gamma,
                                              z_far)
    gt_sil = (a2 > 0.5).float()
    gt_depth = d2.clone()
    reducer = None
    if multi:
        reducer = (GradAllReduce if args.collective == 'allreduce' else GradAllGather)(Bg, K, dev, rank, world)
    one = torch.ones((), device=dev)

    def probe(tag):         # VPN_BENCH_C5_PROBE=1 (diagnostic): the fused C5 step timed at this point of the run
        if os.environ.get('VPN_BENCH_C5_PROBE') and rank == 0 and world == 1:
            r = train_step_block(vpn_amd, _lib, dev, 64, 64, 32, 256, 30, 5, 3, 'fused', False)[0]
            print('PROBE %-28s c5 fused %.3f ms %s' % (tag, r['ms_per_step'], {k: v['avg_us'] for k, v in list(r['kernel_us'].items())[:3]}),
                  file=sys.stderr, flush=True)
    probe('after setup')
    # Philox key of the step: a device counter bumped on the stream at the end of every step, read by the sampler
    # kernels, so every replay of the captured graph draws fresh surface points (the reference resamples each step)
    seed_buf = torch.full((1,), 1234, dtype=torch.int64, device=dev)
    last_out = {}

    def compute(_i=0):
        # total = ChamferDistanceLoss(sample(params), gt) + SilhouetteLoss(L1) + L1 depth loss  (train.py:243-262),
        # one autograd node: sampler -> Chamfer scans -> raster with fused image losses, and the matching backward
        params.grad = None
        # advance_seed: the launch that completes the step's losses also bumps the device step counter (no kernel of
        # its own for the RNG advance)
        out = vpn_amd.HotPathLossFunction.apply(params, kinds, cam, gt_points, gt_sil, gt_depth, n, seed_buf, rank * B,
                                                H, W, sigma, gamma, z_far, 1.0, 1.0, 1.0, 1.0, 1.0, False, True)
        out[2].backward(one)
        last_out['sil'], last_out['depth'] = out[0], out[1]     # replayed graphs rewrite these same tensors
        return out[2]

    def comm():
        if isinstance(reducer, GradAllReduce):
            reducer.allreduce()
        else:
            reducer.gather()

    def step(i=0):
        loss = compute(i)
        if reducer is not None:
            reducer.pack(params.grad, loss)
            comm()
            return reducer.views()
        return params.grad, loss

    def sync():
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    # Issued eagerly the step is launch-bound on the host (about 15 launches of 5-130 us), so the compute part is
    # captured once into a HIP graph and replayed; the collective stays outside the graph.
    use_graph = not args.no_graph
    run_step = step
    if use_graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for i in range(3):
                compute(i)                       # warm the allocator / autograd on the capture stream
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        params.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g_loss = compute(0)
            if reducer is not None:
                reducer.pack(params.grad, g_loss)          # scaled copy into the send buffer: part of the graph
        g_grad = params.grad

        def run_step(i=0):
            graph.replay()
            if reducer is not None:
                comm()                                     # the one collective of the step, outside the graph
                return reducer.views()
            return g_grad, g_loss

    # ---- the contract's timed region: W warm-up steps, then exactly K steps between barrier + synchronize
    for i in range(args.warmup):
        run_step(i)
    sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        last = run_step(args.warmup + i)
    sync()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {'grad_params': last[0], 'loss_total': last[1], 'loss_silhouette': last_out['sil'],
                                         'loss_depth': last_out['depth']})
    if multi:
        tmax = torch.tensor([dt], device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax)
    ms_per_step = dt / args.steps * 1e3
    value = Bg * args.steps / dt
    is_c3 = (B, K, n, M, H) == (64, 32, 256, 2048, 256)

    def headline(seed_after):
        """The contract's line: all a plain run prints (rank 0); --full adds what it measures after the timed region."""
        coll = 'none'
        if multi:
            nbytes = (Bg * K * 10 + 1) * 4 if args.collective == 'allreduce' else (B * K * 10 + 4) * 4
            coll = '%s %s, %d B per rank per step' % ('REHEARSAL over gloo, all ranks on one GPU:' if args.rehearse else 'rccl', 'all-reduce (sum) of the global gradient buffer'
                                                       if args.collective == 'allreduce' else 'all-gather', nbytes)
        if args.global_batch:
            name = 'C4' if (Bg, K, n, M, H) == (256, 32, 256, 2048, 256) else 'custom strong-scaling shape'
        else:
            name = 'C3' if is_c3 else 'custom shape'
        return {
            'metric': 'render+Chamfer fwd+bwd images/sec', 'value': round(value, 1), 'unit': 'images/s',
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(ms_per_step, 4),
            'higher_is_better': True, 'scaling': scaling, 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'launch': 'hip-graph replay' if use_graph else 'eager',
            'config': {'workload': '%s: B=%d/GPU (global %d), K=%d %s, %dx%d silhouette+depth, n=%d pts/prim '
                                   '(N=%d) vs M=%d GT points, Chamfer+L1 fwd+bwd'
                                   % (name if args.kinds == 'spheres' else name + ' variant', B, Bg, K,
                                      {'spheres': 'sphere primitives', 'cuboids': 'cuboid primitives',
                                       'mixed': 'primitives (%d cuboids then %d spheres)' % (K // 2, K - K // 2)}[args.kinds],
                                      H, W, n, K * n, M),
                       'global_batch': Bg, 'parallelism': 'dp%d' % world, 'collective': coll,
                       'sampling': 'fresh Philox draws every step (device step counter, %d steps drawn)' % (seed_after - 1234)},
        }

    if not args.full:
        if rank == 0:
            print(json.dumps(headline(int(seed_buf.item()))), flush=True)
        if multi:
            dist.destroy_process_group()
        return
    probe('after timed region')
    # ---- the same steps again under a HIP event pair on the launch stream: median of `windows` windows
    ev = event_windows(run_step, args.steps, args.windows)
    if multi:
        t = torch.tensor([ev['median'], ev['min'], ev['max']], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ev['median'], ev['min'], ev['max'] = (float(x) for x in t)
    # ---- sustained rate: the GPU's clocks take ~100 steps (~20 ms) of uninterrupted work to settle (measured on this
    # pool: K=20 after W=5 runs 12 % slower per step than K=20 after W=200), so a short timed region sits
    # inside the ramp.  Reported NEXT to the contract's number, never instead of it: 200 untimed steps, then 200 timed
    # ones between the same barrier + synchronize brackets.
    for i in range(200):
        run_step(i)
    sync()
    ts0 = time.perf_counter()
    for i in range(200):
        run_step(i)
    sync()
    dts = time.perf_counter() - ts0
    if multi:
        tmax = torch.tensor([dts], device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dts = float(tmax)
    steady = {'prelude_steps': 200, 'steps': 200, 'ms_per_step': round(dts / 200 * 1e3, 4), 'value': round(Bg * 200 / dts, 1),
              'unit': 'images/s', 'note': 'same step and brackets as `value`, after the clocks have settled'}
    # ---- N>1: what the process group really is and what the exchange costs, so that a SCALE record can be checked without
    # trusting the `parallelism` string: the group's own backend / world size, the RCCL version, every rank's device name,
    # and per-step device time of the compute part and of the collective (hipEvent pairs on the launch stream around each
    # of them; median over the steps, maximum over the ranks)
    dist_info = None
    if multi:
        comp_ev, coll_ev = [], []
        for i in range(max(5, min(args.steps, 50))):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            if use_graph:
                graph.replay()
            else:
                g_loss = compute(i)
                reducer.pack(params.grad, g_loss)
            e1.record()
            comm()
            e2.record()
            comp_ev.append((e0, e1)); coll_ev.append((e1, e2))
        torch.cuda.synchronize()
        med = lambda evs: statistics.median(a.elapsed_time(b) for a, b in evs) * 1e3
        tt = torch.tensor([med(comp_ev), med(coll_ev)], device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        names = [None] * world
        dist.all_gather_object(names, '%s (rank %d, local device %d)' % (torch.cuda.get_device_name(dev), rank, local_rank))
        try:
            ver = '.'.join(str(x) for x in torch.cuda.nccl.version())
        except Exception as e:                  # noqa: BLE001 -- reported in place of the version
            ver = 'unavailable: %s' % type(e).__name__
        dist_info = {'backend': dist.get_backend(), 'world_size': dist.get_world_size(), 'rccl_version': ver,
                     'device_names': names, 'compute_us': round(float(tt[0]), 2), 'collective_us': round(float(tt[1]), 2),
                     'collective': args.collective, 'rehearsal': bool(args.rehearse)}
    seed_after = int(seed_buf.item())
    probe('after steady')

    # ---- device time per C-ABI entry point and per KERNEL (HIP events on the launch stream, recorded by the
    # binding / by the library around every launch), same steps again, eagerly
    ksteps = 20
    with _lib.KernelTimer() as kt, _lib.KernelProfile() as kp:
        for i in range(ksteps):
            step(i)
        entry = kt.summary()            # entry point -> (calls, mean ms)
    kern = kp.summary()                 # kernel      -> (calls, mean ms)
    probe('after profile loop')
    entry_us = {k: round(v[1] * 1e3, 2) for k, v in entry.items()}
    kernel_us = {k: {'calls_per_step': round(v[0] / ksteps, 2), 'avg_us': round(v[1] * 1e3, 2)} for k, v in kern.items()}

    # algorithmic bytes / flops per launch (SURVEY.md 8d per-image figures x B)
    N = K * n
    nn_bytes = B * 16 * (N + M)                       # mean of the two directions: both clouds in, dist + idx out
    alg_bytes = {
        'chamfer_nn_mfma_kernel<2>': 2 * nn_bytes, 'chamfer_nn_mfma_kernel<1>': 2 * nn_bytes,
        'chamfer_nn_mfma_kernel<0>': 2 * nn_bytes,                                                 # one launch = both directions
        'chamfer_nn_kernel<R>': nn_bytes,
        'chamfer_nn_pruned_kernel<1>': nn_bytes,
        'raster_fwd_kernel<0>': B * (40 * K + 8 * H * W), 'raster_fwd_kernel<1>': B * (40 * K + 8 * H * W),
        'raster_bwd_kernel<0>': B * (8 * H * W + 80 * K), 'raster_bwd_kernel<1>': B * (8 * H * W + 80 * K),
        'raster_total_kernel': B * (40 * K + 8 * H * W) + B * (8 * H * W + 80 * K),      # forward + backward in one launch
        'sample_fwd_kernel': B * (40 * K + 12 * N), 'sample_bwd_kernel': B * (12 * N + 80 * K),
        'chamfer_bwd_lds_kernel': B * (12 * (N + M) + 8 * (N + M) + 12 * N),
        'sample_chamfer_bwd_kernel': B * (12 * (N + M) + 8 * (N + M) + 80 * K),
    }
    pmc = load_pmc('c3') if is_c3 else {}
    pair_flops = 8.0 * B * N * M                      # 8 flop per point pair (3 sub, 3 mul, 2 add  ==  K=4 MAC on the matrix pipe)
    dom = max((k for k in kern if k in alg_bytes), key=lambda k: kern[k][0] * kern[k][1])
    dom_s = kern[dom][1] * 1e-3
    hbm_gbs = alg_bytes[dom] / dom_s / 1e9
    if dom.startswith('chamfer_nn_mfma_kernel'):      # the exact scan with the matrix-pipe filter, both directions per launch
        pair_flops *= 2.0
        tf = pair_flops / dom_s / 1e12
        # EXECUTED work on the pipe the kernel runs on: matrix-pipe flops issued per 32x32 block of (target, query) pairs
        #   <2>: ONE v_mfma_f32_32x32x16_f16 = 32 flop per pair (fp32 coordinates scaled by 2^11, split into 2 fp16
        #        pieces, 12 of 16 K slots used);  <1>: 32x32x16_bf16 + 32x32x8_bf16 = 48 flop per pair;
        #   <0>: two 32x32x2_f32 = 8 flop per pair on the fp32 pipe
        per_pair, peak, pipe = {'<2>': (32.0, F16_PEAK_TFLOPS, 'fp16 matrix pipe: v_mfma_f32_32x32x16_f16, one per 32x32 pairs'),
                                '<1>': (48.0, F16_PEAK_TFLOPS, 'bf16 matrix pipe: v_mfma_f32_32x32x16_bf16 + 32x32x8_bf16 per 32x32 pairs'),
                                '<0>': (8.0, FP32_PEAK_TFLOPS, 'fp32 matrix pipe: 2 x v_mfma_f32_32x32x2_f32 per 32x32 pairs')}[dom[-3:]]
        ex_flops = 2.0 * per_pair * B * N * M
        ex = ex_flops / dom_s / 1e12
        roofline = {'bound': 'mfma', 'kernel': dom, 'achieved': round(ex, 1), 'peak': peak, 'unit': 'TFLOP/s',
                    'frac': round(ex / peak, 4), 'traffic': traffic_of(dom, pmc),
                    'basis': 'EXECUTED matrix-pipe flops per launch (MFMA instructions issued x flops each; equals PMC '
                             'SQ_INSTS_MFMA x 32768 in profiles/) / measured launch time, against the dense MFMA peak of '
                             'the input type (MI355X_MICROARCH.md).  ' + pipe,
                    'executed_flops_per_launch': ex_flops, 'avg_launch_us': round(dom_s * 1e6, 2),
                    'hbm_frac': round(hbm_gbs / HBM_PEAK_GBS, 5), 'hbm_achieved_GBps': round(hbm_gbs, 2),
                    'algorithmic_bytes_per_launch': alg_bytes[dom],
                    # the fp32 FORMULATION's flops (8 per point pair: 3 sub, 3 mul, 2 add) over the same time, against the
                    # fp32 vector peak: may exceed 1 -- it says the filter beats any fp32 implementation, not headroom
                    'algorithmic_fp32_tflops': round(tf, 2),
                    'algorithmic_fp32_vs_vector_peak': round(tf / FP32_PEAK_TFLOPS, 4)}
    else:
        roofline = {'bound': 'hbm', 'kernel': dom, 'achieved': round(hbm_gbs, 2), 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                    'frac': round(hbm_gbs / HBM_PEAK_GBS, 5), 'traffic': traffic_of(dom, pmc),
                    'algorithmic_bytes_per_launch': alg_bytes[dom], 'avg_launch_us': round(dom_s * 1e6, 2)}
        if dom.startswith('chamfer_nn'):
            roofline['valu_tflops'] = round(pair_flops / dom_s / 1e12, 2)
            roofline['valu_frac_of_fp32_peak'] = round(pair_flops / dom_s / 1e12 / FP32_PEAK_TFLOPS, 4)
    if pmc:
        roofline['traffic_source'] = os.path.relpath(PMC_FILE, ROOT) + ' (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, same workload)'
    # the raster pair: HBM view (algorithmic bytes) and the executed-work view (VALU issue) per kernel
    raster_roof = {}
    for name in ('raster_total_kernel', 'raster_fwd_kernel<1>', 'raster_bwd_kernel<1>'):
        if name in kern:
            us = kern[name][1] * 1e3
            gbs = alg_bytes[name] / (us * 1e-6) / 1e9
            raster_roof[name] = {'avg_launch_us': round(us, 2), 'algorithmic_bytes_per_launch': alg_bytes[name],
                                 'hbm_GBps': round(gbs, 2), 'hbm_frac': round(gbs / HBM_PEAK_GBS, 5),
                                 'traffic': traffic_of(name, pmc), 'executed_work': valu_issue_roofline(name, pmc, us)}

    # whole step against the HBM roofline (north_star asks for it): PMC-measured bytes of every kernel of the step / step time
    step_hbm = None
    if pmc:
        per = {k: traffic_of(k, pmc) for k in kern}
        if all(v is not None for v in per.values()):
            tot = sum(v * round(kern[k][0] / ksteps) for k, v in per.items())
            gbs = tot / (ev['median'] * 1e-3) / 1e9
            alg = sum(alg_bytes.get(k, 0) * round(kern[k][0] / ksteps) for k in kern)
            step_hbm = {'traffic_bytes_per_step': int(tot), 'achieved_GBps': round(gbs, 1), 'peak_GBps': HBM_PEAK_GBS,
                        'frac': round(gbs / HBM_PEAK_GBS, 4), 'algorithmic_bytes_per_step': int(alg),
                        'note': 'sum over the kernels of one step of FETCH_SIZE (x2 for the 16-B-per-lane streams) + '
                                'WRITE_SIZE from profiles/r04_pmc.json, over the hipEvent median step time: the step is '
                                'issue-bound (VALU / matrix pipe), not HBM-bound'}

    # The legs below are reported NEXT to the headline: a failure in one of them (host out of memory in the CPU leg, ...)
    # must not cost the line itself, so it is reported as {"error": ...} in its place
    def guarded(fn, *a):
        try:
            return fn(*a)
        except Exception as e:        # noqa: BLE001 -- reported, not swallowed
            return {'error': '%s: %s' % (type(e).__name__, e)}

    # BASELINE config C5, one GPU: the step train.py really runs (all five losses, train.py:243-262), as one fused autograd
    # node and as the module composition a train.py user writes; on a partly converged batch; and at the reference's default
    # shape (config.py:8-9,34,49: K = 16, n = 128, B = 8, 128 x 128).  (The slowdown of this block seen inside
    # the full line in round 4 -- every dispatch +45-65 us, eager and replayed -- was NOT the CPU legs: it was the EMD
    # kernel's cooperative launch in a process that had captured a HIP graph before, profiles/r04_coop_launch_side_effect.txt;
    # the kernel is launched plainly since.)
    c5 = None
    if rank == 0 and world == 1 and not args.no_extras and not args.no_c5:
        c5 = {
            'fused': guarded(lambda: train_step_block(vpn_amd, _lib, dev, 64, 64, 32, 256, 50, 10, 3, 'fused', not args.no_cpu_baseline)[0]),
            'modules': guarded(lambda: train_step_block(vpn_amd, _lib, dev, 64, 64, 32, 256, 30, 5, 3, 'modules', False)[0]),
            'fused_partly_converged': guarded(lambda: train_step_block(vpn_amd, _lib, dev, 64, 64, 32, 256, 50, 10, 3, 'fused', False, 'surface')[0]),
            'reference_default_shape_fused': guarded(lambda: train_step_block(vpn_amd, _lib, dev, 8, 16, 128, 128, 50, 10, 3, 'fused', False)[0]),
        }

    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = guarded(cpu_baseline, params_all[:args.cpu_sample].detach().cpu(), gt_all[:args.cpu_sample].cpu(),
                      p2_all[:args.cpu_sample].detach().cpu(), K, n, H, W, sigma, gamma, z_far, kinds, cam, vpn_amd)

    c2 = None
    if rank == 0 and world == 1 and not args.no_c2:
        c2 = guarded(raster_only, vpn_amd, _lib, dev, 32, 16, 128, args.steps, args.warmup, args.windows, 'c2')

    if rank == 0:
        out = headline(seed_after)
        out.update({
            'hip_event_ms_per_step': {k: (round(v, 5) if isinstance(v, float) else v) for k, v in ev.items()},
            'steady_state': steady,
            'roofline': roofline, 'raster_roofline': raster_roof, 'kernel_us': kernel_us, 'entry_us': entry_us,
        })
        assert 0.0 < roofline['frac'] <= 1.0, 'roofline.frac must be a fraction: %r' % (roofline,)
        if dist_info is not None:
            out['dist'] = dist_info
        if step_hbm is not None:
            out['step_hbm'] = step_hbm
            roofline['step_hbm_frac'] = step_hbm['frac']
        if cpu is not None:
            out['cpu_baseline'] = cpu
        if c2 is not None:
            out['c2'] = c2
        if world == 1 and not args.no_extras and args.kinds == 'spheres':
            # SURVEY.md 8d secondary runs: the same step with cuboid primitives (their sampler, raster and gradient branches)
            def variant(klist):
                kt_ = vpn_amd.kinds_tensor(klist, dev)
                pv = params.detach().clone().requires_grad_(True)
                with torch.no_grad():
                    av, dv = vpn_amd.RasterFunction.apply(p2_all[rank * B:(rank + 1) * B].contiguous(), kt_, cam, H, W, sigma, gamma, z_far)
                gs, gdp = (av > 0.5).float(), dv.clone()
                sb = torch.full((1,), 1234, dtype=torch.int64, device=dev)

                def comp(_i=0):
                    pv.grad = None
                    o = vpn_amd.HotPathLossFunction.apply(pv, kt_, cam, gt_points, gs, gdp, n, sb, rank * B, H, W, sigma, gamma, z_far,
                                                          1.0, 1.0, 1.0, 1.0, 1.0, False, True)
                    o[2].backward(one)
                    return o[2]
                sd = torch.cuda.Stream()
                sd.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(sd):
                    for i in range(3):
                        comp(i)
                torch.cuda.current_stream().wait_stream(sd)
                torch.cuda.synchronize()
                gph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gph):
                    lv = comp(0)
                for _ in range(10):
                    gph.replay()
                e = event_windows(lambda i: gph.replay(), 100, 3)
                with _lib.KernelProfile() as kpv:
                    for i in range(10):
                        comp(i)
                ku = {k: round(v[1] * 1e3, 2) for k, v in kpv.summary().items()}
                return {'ms_per_step': round(e['median'], 5), 'images_per_s': round(B / e['median'] * 1e3, 1), 'loss': float(lv),
                        'finite_grad': bool(torch.isfinite(pv.grad).all()), 'kernel_us': ku}
            out['kinds_variants'] = {'cuboids': guarded(variant, [vpn_amd.CUBOID] * K),
                                     'mixed (K/2 cuboids then spheres, train.py:112-116)':
                                         guarded(variant, [vpn_amd.CUBOID] * (K // 2) + [vpn_amd.SPHERE] * (K - K // 2))}
        if world == 1 and not args.no_extras:      # row f1, outside the metric: the auction EMD loss of the same step
            out['emd'] = guarded(emd_extra, B, M, dev, vpn_amd, cpu is not None and 'error' not in cpu)
        if c5 is not None:
            out['c5'] = c5
        print(json.dumps(out), flush=True)
    if multi:
        dist.destroy_process_group()


def dump_outputs(directory, arrays):
    """--dump-outputs: every array as DIR/<name>.npy in float32, copied to the host before any later step overwrites it.
    The inputs are seeded and the Philox counter advances once per step, so the same arguments give the same step."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(directory, name + '.npy'), t.detach().float().cpu().numpy())


def emd_extra(B, n, dev, vpn_amd, with_cpu):
    """EarthMoverDistanceLoss fwd+bwd as train.py:193 calls it (eps=0.005, 50 iterations) on B clouds of n points;
    not part of `value`.  CPU leg: the oracle's auction on one cloud."""
    gen = torch.Generator().manual_seed(3)
    x1 = torch.rand(B, n, 3, generator=gen).to(dev).requires_grad_(True)
    x2 = torch.rand(B, n, 3, generator=gen).to(dev)
    emd = vpn_amd.modules.loss.EarthMoverDistanceLoss()

    def once():
        d, _ = emd(x1, x2, 0.005, 50)
        x1.grad = None
        d.mean().backward()
    once()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        once()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / 5 * 1e3
    out = {'workload': 'EMD auction fwd+bwd, B=%d, n=m=%d, eps=0.005, iters=50' % (B, n), 'ms': round(ms, 3),
           'clouds_per_s': round(B / ms * 1e3, 1)}
    if with_cpu:
        from oracle import vpn_oracle as O
        a, b = x1.detach()[:1].cpu(), x2[:1].cpu()
        t0 = time.perf_counter()
        rd, ra = O.emd_auction(a, b, 0.005, 50)
        cpu_s = time.perf_counter() - t0
        d, idx = emd(x1.detach()[:1], x2[:1], 0.005, 50)
        out['cpu_port_clouds_per_s'] = round(1.0 / cpu_s, 2)
        out['parity_vs_oracle'] = {'assignment_equal': bool(torch.equal(idx.cpu(), ra)),
                                   'dist_bit_equal': bool(torch.equal(d.cpu(), rd))}
    return out


def cpu_baseline(params, gt_points, params2, K, n, H, W, sigma, gamma, z_far, kinds, cam, vpn_amd):
    """The oracle (CPU PyTorch restatement of the reference path, dense B*N*M Chamfer) timed on the host cores on a
    bounded sample of the same workload (median of 3 passes after a warm-up pass on one image), and the HIP path
    compared with it on exactly those samples.  The GT silhouette / depth of this leg is rendered by the ORACLE
    (second primitive set, thresholded at 0.5) so the comparison does not depend on the kernel being checked."""
    from oracle import vpn_oracle as O
    host_cores = os.cpu_count() or 1
    # threads = the cores this process may actually run on, capped at the 1-GPU box's CPU share (16 of the host's
    # cores: the box enforces that share, more threads than that only thrash); both numbers are reported
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = host_cores
    threads = min(usable, 16)
    torch.set_num_threads(threads)
    S = params.shape[0]
    seed = 1234
    u = O.philox_uniforms(seed, 0, S, K, n)
    kl = [0] * K
    camc = torch.tensor([[1.0, 0.0, 0.0]]).expand(S, 3).contiguous()
    with torch.no_grad():
        gs, gd = [], []
        for b in range(0, S, 4):
            a2, d2 = O.raster(params2[b:b + 4], kl, camc[b:b + 4], H, W, sigma, gamma, z_far)
            gs.append((a2 > 0.5).float())
            gd.append(d2)
        gt_sil, gt_depth = torch.cat(gs), torch.cat(gd)
        # The L1 depth loss differentiates through sign(D - gt_depth), which fp32 cannot decide where the predicted and
        # the GT surface cross within rounding noise; ONE flipped pixel moves the gradient by ~1e-3 relative (it carries
        # 2/(S*H*W) of weight against ~1e3 edge pixels per primitive), and a 32-image sample holds about one such pixel
        # (Finding 6).  Those pixels get their GT moved by 1e-3 so that the comparison is decidable.
        dp = torch.cat([O.raster(params[b:b + 4], kl, camc[b:b + 4], H, W, sigma, gamma, z_far)[1] for b in range(0, S, 4)])
        diff = dp - gt_depth
        near = (diff != 0) & (diff.abs() < 1e-5)
        gt_depth = torch.where(near, gt_depth - torch.where(diff >= 0, 1e-3, -1e-3), gt_depth)
        n_near = int(near.sum())

    def run(S=S):
        p = params.clone().requires_grad_(True)
        total = 0.0
        for b in range(S):                               # one image per chunk: dense tensors stay < 2 GB
            pb = p[b:b + 1]
            pts = O.sample_primitives(pb, kl, u[b:b + 1])
            cd = O.chamfer_loss(pts, gt_points[b:b + 1], each_batch=True).sum() / S
            a, d = O.raster(pb, kl, camc[b:b + 1], H, W, sigma, gamma, z_far)
            loss = cd + (a - gt_sil[b:b + 1]).abs().sum() / (S * H * W) + (d - gt_depth[b:b + 1]).abs().sum() / (S * H * W)
            loss.backward()
            total += float(loss.detach())
        return total, p.grad

    run(1)                                               # warm-up on one image
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        loss_c, grad_c = run()
        times.append(time.perf_counter() - t0)
    dt = statistics.median(times)
    # same samples on the GPU (host seed = the Philox key the oracle's draws were generated with)
    dev = cam.device
    pg = params.to(dev).requires_grad_(True)
    loss_g = vpn_amd.HotPathLossFunction.apply(pg, kinds, cam[:S].contiguous(), gt_points.to(dev), gt_sil.to(dev),
                                               gt_depth.to(dev), n, seed, 0, H, W, sigma, gamma, z_far, 1.0, 1.0, 1.0)[2]
    loss_g.backward()
    gerr = float((pg.grad.cpu() - grad_c).abs().max() / grad_c.abs().max())
    lerr = abs(float(loss_g.detach()) - loss_c) / abs(loss_c)
    return {'value': round(S / dt, 3), 'unit': 'images/s', 'cores': threads, 'host_cores': host_cores, 'kind': 'port',
            'cores_note': 'min(cores in the affinity mask = %d, the 16-core CPU share of a 1-GPU box)' % usable,
            'sample': '%d images of the same workload; 1-image warm-up, then the median of 3 timed passes (%s s), torch CPU '
                      'fp32 with %d threads on a host with %d cores, dense B*N*M Chamfer as chamfer_distance.py:14-23'
                      % (S, '/'.join('%.1f' % t for t in times), threads, host_cores),
            'parity_loss_rel': float('%.3g' % lerr), 'parity_grad_rel': float('%.3g' % gerr),
            'parity_vs_gpu': {'loss_rel': float('%.3g' % lerr), 'grad_rel': float('%.3g' % gerr),
                              'gt_images': 'rendered by the CPU oracle; %d pixels whose predicted depth lies within '
                                           '1e-5 of the GT depth (sign of the L1 term undecidable in fp32) had '
                                           'their GT moved by 1e-3' % n_near}}


if __name__ == '__main__':
    main()
