"""float64 restatement of the reference's training step (train.py:243-262) with FROZEN discrete decisions, and the cases the
training-step tests share.  TEST INFRASTRUCTURE ONLY.

`oracle.vpn_oracle.train_step` is the fp32 parity reference of TrainStepLossFunction.  `step_f64` below evaluates the same
five terms and their gradient in float64 -- the truth that bounds the fp32 rounding noise of the oracle and of the kernels --
but takes every discrete choice of the step as an INPUT instead of recomputing it: both Chamfer argmin pairs, the
VP-diversity argmin pair, the EMD assignment and the cuboid face counts.  The fp32 oracle supplies them
(`return_decisions=True`), so float64 cannot flip a near tie and move the gradient by a whole point's worth (the ReLU-mask
precedent of tests/gcn_ref.py).  The raster has no such decision the silhouette loss could flip: its ground truth is 0 / 1
and alpha lies strictly inside."""
import functools

import torch

from oracle import vpn_oracle as O

SEED = 77                    # Philox seed of every case

# name: (B, K, n, M, Mc, H, W, batch seed).  Every case is a shape TrainStepLossFunction takes (K <= 64, N M >= 512^2,
# M <= 7680) and the smallest that reaches its path (SCB_BLOCK = 128 lanes per workgroup of the backward kernel):
#   A  mixed kinds (cuboids first, train.py:112-116), partial raster tiles (40 x 24 is no multiple of 16)
#   B  n > SCB_BLOCK and no multiple of 64: the own-neighbour loop takes a second, partly filled trip
#   C  M > 8 * SCB_BLOCK: second trip of the eight-pass scatter loop with a ragged tail (1050 = 1024 + 26); the
#      VP-diversity scatter rides in it
#   D  N != M != Mc (EMD weight 0: the auction needs N = M)
#   E  K at the CFEAT_SLOTS limit, N M exactly 512^2
CASES = {
    'A': (3, 16, 32, 512, 512, 40, 24, 5),
    'B': (2, 4, 130, 520, 520, 32, 32, 6),
    'C': (2, 3, 350, 1050, 1050, 32, 32, 7),
    'D': (2, 5, 77, 700, 333, 24, 40, 18),
    'E': (1, 64, 8, 512, 512, 32, 32, 9),
}

W_ALL = (1.0, 0.7, 1.0, 0.1, 1.0)                                    # (L_VIEW_CD, L_CAN_CD, L_SIL, L_VP_DIV, L_EMD)
W_ISOLATED = {'view': (1.0, 0.0, 0.0, 0.0, 0.0), 'canon': (0.0, 0.7, 0.0, 0.0, 0.0), 'sil': (0.0, 0.0, 1.0, 0.0, 0.0),
              'vpdiv': (0.0, 0.0, 0.0, 0.1, 0.0), 'emd': (0.0, 0.0, 0.0, 0.0, 1.0)}
W_D = (1.0, 0.7, 1.0, 0.1, 0.0)                                      # case D: N != M, no EMD term
W_HOT = (1.0, 0.0, 0.8, 0.0, 0.0)                                    # what HotPathLossFunction computes: (w_cd, -, w_sil, -, -)
BLOCKS = (('v', slice(0, 3)), ('q', slice(3, 7)), ('t', slice(7, 10)))

# (id, case, kinds, weights, options): every step the parity tests compare with the oracle.  options are keywords of
# oracle.train_step / step_f64 (and, but for grad_scale, of TrainStepLossFunction)
OPTIONS = dict(cd_w1=0.5, cd_w2=2.0, sil_mse=True, sample_base=3)
STEPS = ([('A-%s-all' % kn, 'A', kn, W_ALL, {}) for kn in ('spheres', 'cuboids')]
         + [('%s-mixed-%s' % (c, wn), c, 'mixed', w, {}) for c in ('A', 'C')
            for wn, w in list(W_ISOLATED.items()) + [('all', W_ALL)]]
         + [('B-mixed-all', 'B', 'mixed', W_ALL, {}), ('D-mixed-noemd', 'D', 'mixed', W_D, {}), ('E-mixed-all', 'E', 'mixed', W_ALL, {}),
            ('A-mixed-options', 'A', 'mixed', W_ALL, OPTIONS), ('A-mixed-scale', 'A', 'mixed', W_ALL, dict(grad_scale=0.3)),
            # HotPathLossFunction's total (w_cd Chamfer + w_sil silhouette, view-centred camera, no depth term) is this step
            ('A-mixed-hot', 'A', 'mixed', W_HOT, {}), ('A-mixed-hot-scale', 'A', 'mixed', W_HOT, dict(grad_scale=0.3))])
STEP_IDS = [s[0] for s in STEPS]
STEP_BY_ID = {s[0]: s for s in STEPS}


def kinds_of(name, K):
    """'spheres', 'cuboids' or 'mixed' (the cuboids first, then the spheres: the order train.py:112-116 samples in)."""
    return {'spheres': [O.SPHERE] * K, 'cuboids': [O.CUBOID] * K, 'mixed': [O.CUBOID] * (K // 2) + [O.SPHERE] * (K - K // 2)}[name]


@functools.lru_cache(maxsize=None)
def batch(case):
    """Host inputs of a case: (params [B,K,10], gt_view [B,M,3], gt_canon [B,Mc,3], gt_sil [B,1,H,W], dists, elevs, azims,
    angles [B]).  The object-centred cloud holds Mc points of its own, not the transformed view-centred cloud: where
    Mc != M the two cannot be mixed up unnoticed.  Shared between tests: never written to."""
    B, K, n, M, Mc, H, W, seed = CASES[case]
    g = torch.Generator().manual_seed(seed)
    v = (torch.rand(B, K, 3, generator=g) + 0.1) / torch.tensor([8.0, 10.0, 10.0])
    params = torch.cat([v, torch.rand(B, K, 4, generator=g), 0.35 * (torch.rand(B, K, 3, generator=g) * 2 - 1)], 2)
    gt_view = torch.rand(B, M, 3, generator=g) - 0.5
    dists = 1.0 + 0.5 * torch.rand(B, generator=g)
    elevs = 20.0 + 20.0 * torch.rand(B, generator=g)
    azims = 360.0 * torch.rand(B, generator=g)
    angles = 30.0 * torch.rand(B, generator=g)
    gt_canon = O.view_to_obj_points(torch.rand(B, Mc, 3, generator=g) - 0.5, dists, elevs, azims, angles)
    gt_sil = (torch.rand(B, 1, H, W, generator=g) > 0.6).float()
    return params, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles


def _sample(p, kinds, u, face_counts):
    """oracle.sample_primitives with the cuboid face counts handed in (cuboid.py:30-53 rounds n * area / total half to
    even: a decision)."""
    out = []
    for k, kind in enumerate(kinds):
        v, q, t = p[:, k, 0:3], p[:, k, 3:7], p[:, k, 7:10]
        if kind == O.SPHERE:
            out.append(O.sphere_sampling(v, q, t, u[:, k, :, 0], u[:, k, :, 1]))
        else:
            out.append(O.transform_points(O.cuboid_canonical(u[:, k], face_counts[:, k]) * v[:, None, :], q, t))
    return torch.cat(out, 1)


def _pick(points, idx):
    return torch.gather(points, 1, idx.long()[..., None].expand(-1, -1, 3))


def _chamfer(p1, p2, nn, w1, w2):
    """chamfer_distance.py:14-30 with the two argmins given: sum_b (w1 mean_i |p1_i - p2[idx1_i]| + w2 mean_j |p2_j - p1[idx2_j]|) / B."""
    m1 = torch.sqrt(((p1 - _pick(p2, nn[0])) ** 2).sum(-1))
    m2 = torch.sqrt(((p2 - _pick(p1, nn[1])) ** 2).sum(-1))
    return (w1 * m1.mean(1) + w2 * m2.mean(1)).mean()


def step_f64(params, kinds, u, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles, H, W, weights, decisions,
             cd_w1=1.0, cd_w2=1.0, sil_mse=False, grad_scale=1.0, sigma=0.05, gamma=0.1, z_far=2.0):
    """The five weighted terms of oracle.train_step and their sum ([6], float64, unscaled) and d (grad_scale * total) /
    d params ([B,K,10], float64), every tensor taken to float64 first.  u [B,K,n,3]: the Philox uniforms of the step
    (oracle.philox_uniforms(seed, sample_base, B, K, n)); decisions: the dict oracle.train_step(..., return_decisions=True)
    returns.  A term of weight 0 is not evaluated (its value and its gradient are exactly 0)."""
    d64 = lambda t: t.detach().double()
    w = [float(x) for x in weights]
    B = params.shape[0]
    p = d64(params).requires_grad_(True)
    gt_view, gt_canon = d64(gt_view), d64(gt_canon)
    pred = _sample(p, kinds, d64(u), decisions['face_counts'])
    zero = torch.zeros((), dtype=torch.float64)
    view_cd = _chamfer(pred, gt_view, decisions['view_nn'], cd_w1, cd_w2) * w[0] if w[0] else zero
    obj_cd = zero
    if w[1]:
        canon = O.view_to_obj_points(pred, d64(dists), d64(elevs), d64(azims), d64(angles))
        obj_cd = _chamfer(canon, gt_canon, decisions['canon_nn'], cd_w1, cd_w2) * w[1]
    sil = zero
    if w[2]:
        cam = torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64).expand(B, 3)
        alpha, _ = O.raster(p, kinds, cam, H, W, sigma, gamma, z_far)
        d = alpha - d64(gt_sil).reshape(B, H, W)
        sil = ((d * d).mean() if sil_mse else d.abs().mean()) * w[2]
    div = _chamfer(p[:, :, 7:10], gt_view, decisions['vpdiv_nn'], 0.5, 1.0) * w[3] if w[3] else zero
    emd = zero
    if w[4]:
        emd = torch.sqrt(((pred - _pick(gt_view, decisions['emd_assign'])) ** 2).sum(-1)).mean() * w[4]
    total = view_cd + obj_cd + sil + div + emd
    total.backward(torch.tensor(float(grad_scale), dtype=torch.float64))
    return torch.stack([view_cd, obj_cd, sil, div, emd, total]).detach(), p.grad


def references_for(step_id, emd_points=None):
    """(fp32 oracle losses [6], its gradient, float64 losses [6], float64 gradient) of one entry of STEPS.  emd_points: see
    oracle.train_step (the cloud a kernel auctioned; the assignment is a decision both references then share)."""
    _, case, kn, w, opts = STEP_BY_ID[step_id]
    B, K, n, M, Mc, H, W, _ = CASES[case]
    kinds = kinds_of(kn, K)
    inputs = batch(case)
    l32, g32, dec = O.train_step(*inputs, kinds, n, H, W, w, SEED, return_decisions=True, emd_points=emd_points, **opts)
    u = O.philox_uniforms(SEED, opts.get('sample_base', 0), B, K, n)
    f64_opts = {k: v for k, v in opts.items() if k != 'sample_base'}
    l64, g64 = step_f64(inputs[0], kinds, u, *inputs[1:], H, W, w, dec, **f64_opts)
    return l32, g32, l64, g64


@functools.lru_cache(maxsize=None)
def references(step_id):
    """references_for(step_id) with the oracle's own cloud in the auction: computed once per process, shared by every test
    that needs it, never written to."""
    return references_for(step_id)


def zero_blocks(weights):
    """The gradient blocks that must be IDENTICALLY zero for a weight vector: VP-diversity reaches the centres only, so
    when nothing else is on the v and q blocks are zero."""
    w = [float(x) for x in weights]
    return ('v', 'q') if (w[3] and not (w[0] or w[1] or w[2] or w[4])) else ()
