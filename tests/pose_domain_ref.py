"""The pose (make_pose / pose_backward of csrc/vpn_common.h) over its whole parameter domain, for the tests: a fixed pose set,
a per-pose error measure and the float64 statement of every op that inlines the pose -- transform_points, the sampler, the
primitive-to-mesh op and the Chamfer loss behind the fused backward.

Reference.  oracle/vpn_oracle.py is dtype-generic: handed float64 tensors it computes in float64 (its PI stays the fp32 value
of pi the reference and the kernels use).  The reference of a test is that oracle on the fp32 inputs cast up, autograd for the
gradients.  Discrete decisions are NOT recomputed in float64: the cuboid face quotas come from the fp32 extents
(O.cuboid_face_counts, what the kernel counts), the Chamfer nearest neighbours of the fused backward from the GPU's forward.

Measure.  rel_err (max|a-b| / max|b| over a whole tensor) lets one pose with a large gradient hide another whose gradient is
entirely wrong: over the pose set the grad_q blocks span eight orders of magnitude.  block_rel_err holds every pose to
its own scale: one block per pose or primitive, the block's largest error against the block's largest component plus a floor
of 1e-3 of the median block size (a block that is zero in exact arithmetic is held to that floor)."""
import functools
import math

import torch

from oracle import vpn_oracle as O

BAR = 1e-4                     # the project's fp32 bar, here per block
REF_BAR = 5.5e-5               # the fp32 oracle's own distance from float64 by the same measure (test_pose_domain_cpu.py)
AXES = [(1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0),
        (-0.3, 0.7, -0.9), (1.0, 1.0, 1.0), (-1.0, -1.0, -1.0),
        (0.0, 0.0, 0.0), (1e-3, -2e-3, 5e-4), (3.0, -4.0, 12.0), (0.2, 0.1, -0.05)]
ANGLES = [0.0, -0.0, 1.0, -1.0,
          0.25, -0.25, 0.5, 0.75,
          1e-4, -1e-4, 0.9999, 1e-7,
          2.37, -3.62, 17.125,
          0.49999, 0.50001]
MIN_LENGTH = 0.05              # poses whose 4-vector (axis sin h, cos h) is shorter are ill-conditioned by construction
POSE_COUNT = 164               # 170 - 6: the zero and the tiny axis at the half turn and a hair on either side of it


def quat_length(q):
    """|(axis sin h, cos h)| of rotate.py:59-72 in float64 on the fp32 q: the length the 4-vector is divided by."""
    q = q.double()
    h = torch.remainder(q[:, 3], 1) * O.PI
    return torch.sqrt((q[:, :3] ** 2).sum(1) * torch.sin(h) ** 2 + torch.cos(h) ** 2)


@functools.lru_cache(maxsize=None)
def _poses():
    q = torch.tensor([list(a) + [t] for a in AXES for t in ANGLES], dtype=torch.float32)
    q = q[quat_length(q) >= MIN_LENGTH].contiguous()
    assert q.shape == (POSE_COUNT, 4), q.shape
    for t in ANGLES:                                   # no group of the product was emptied
        assert int((q[:, 3] == t).sum()) >= len(AXES) - 2
    assert int((q[:, :3] == 0).all(1).sum()) == len(ANGLES) - 3
    assert int((torch.signbit(q[:, 3]) & (q[:, 3] == 0)).sum()) == len(AXES)      # -0.0 survives the tensor
    return q


def poses():
    """[164, 4] fp32, fixed: AXES x ANGLES minus the poses shorter than MIN_LENGTH."""
    return _poses().clone()


def block_errors(a, b, floor=1e-3):
    """[P]: error of block i of a against b (both [P, ...]), max|a_i - b_i| / (max|b_i| + floor * median_j max|b_j|)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape and a.dim() >= 1, (a.shape, b.shape)
    P = a.shape[0]
    a, b = a.reshape(P, -1), b.reshape(P, -1)
    size = b.abs().amax(1)
    den = size + floor * size.median().clamp_min(1e-300)
    err = (a - b).abs().amax(1) / den
    return torch.where(torch.isfinite(a).all(1), err, torch.full_like(err, math.inf))


def block_rel_err(a, b, floor=1e-3):
    return float(block_errors(a, b, floor).max())


def prim_blocks(x, n=None):
    """Blocks of a [B, K, ...] tensor (one per primitive), or of the [B, K*n, 3] points of a sampler call."""
    if n is not None:
        B = x.shape[0]
        return x.reshape(B, -1, n, 3).reshape(-1, n, 3)
    return x.reshape(x.shape[0] * x.shape[1], -1)


GROUPS = (('v', slice(0, 3)), ('q', slice(3, 7)), ('t', slice(7, 10)))


def param_group_errors(ga, gb):
    """{'grad_v' | 'grad_q' | 'grad_t': [B*K] block errors} of two [B,K,10] parameter gradients."""
    return {'grad_' + name: block_errors(prim_blocks(ga[..., sl]), prim_blocks(gb[..., sl])) for name, sl in GROUPS}


# ----------------------------------------------------------------------------- inputs
def rand_volumes(gen, *shape):
    """Extents in the project's range (tests' rand_params: (U + 0.1) / (8, 10, 10))."""
    return (torch.rand(*shape, 3, generator=gen) + 0.1) / torch.tensor([8.0, 10.0, 10.0])


def pose_params(gen, K=2, t_max=0.35):
    """[164, K, 10]: pose b in every one of the K primitives of sample b, random extents and translations."""
    q = poses()
    B = q.shape[0]
    v = rand_volumes(gen, B, K)
    t = t_max * (torch.rand(B, K, 3, generator=gen) * 2 - 1)
    return torch.cat([v, q[:, None, :].expand(B, K, 4), t], 2).contiguous()


U0_EDGES = [0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 1.0]     # the poles: 2 sqrt(u0 (1 - u0)) against the acos chain
U1_EDGES = [0.0, 1.0 - 2.0 ** -24]


def edge_uniforms(gen, B, K, n):
    """Random [B,K,n,3] draws whose first rows hold U0_EDGES x U1_EDGES (as many of the 10 as n has room for)."""
    u = torch.rand(B, K, n, 3, generator=gen)
    for i in range(min(n, len(U0_EDGES) * len(U1_EDGES))):
        u[:, :, i, 0] = U0_EDGES[i % len(U0_EDGES)]
        u[:, :, i, 1] = U1_EDGES[i // len(U0_EDGES)]
    return u


def conditioned(make, seed, tries=64):
    """The inputs of a GPU test.  make(gen) -> (case, r64, ora): the inputs drawn from gen, their float64 reference and the
    block errors {group: figure} of the fp32 ORACLE on them.  Returns those of the first seed of seed, seed + 1, ... on which
    every figure of the oracle is within REF_BAR.

    Why inputs are chosen at all: a hair beside an integer angle (-1e-4, 0.9999) the fp32 rounding of h = pi * (q3 mod 1)
    is 2.4e-4 of sin h, in the reference's own fp32 arithmetic and in any kernel that follows it.  Only the floor of
    block_errors absorbs that, by a factor that is the size of that pose's grad_q block against the median block -- a matter
    of the random weights, 2e-5 to 1.1e-4 from draw to draw.  The 1e-4 bar of the kernels presumes the reference's own
    margin (REF_BAR); a draw on which the oracle itself has none tests the draw.  The choice looks at the CPU oracle only,
    never at a kernel's output."""
    for s in range(seed, seed + tries):
        case, r64, ora = make(torch.Generator().manual_seed(s))
        if max(ora.values()) <= REF_BAR:
            return case, r64, ora
    raise AssertionError('no draw in %d on which the fp32 oracle stays within %.1e of float64' % (tries, REF_BAR))


# ----------------------------------------------------------------------------- the float64 (or fp32) statements
def _leaf(x, dtype):
    """A fresh leaf of its own in `dtype` (x.to(dtype) of an fp32 x is x itself)."""
    return x.detach().clone().to(dtype).requires_grad_(True)


def transform_ref(points, q, t, W, dtype=torch.float64):
    """out, grad_points, grad_q, grad_t (None without t) of (transform_points(points, q, t) * W).sum() in `dtype`."""
    p = _leaf(points, dtype)
    qq = _leaf(q, dtype)
    tt = _leaf(t, dtype) if t is not None else None
    out = O.transform_points(p, qq, tt) if t is not None else O.rotate_points(p, qq)
    (out * W.to(dtype)).sum().backward()
    return out.detach(), p.grad, qq.grad, tt.grad if t is not None else None


def face_counts(params, kinds, n):
    """[B,K,6] int32 quotas of the cuboids from the fp32 extents (zero rows for spheres): handed to every precision."""
    B, K, _ = params.shape
    counts = torch.zeros(B, K, 6, dtype=torch.int32)
    for k in range(K):
        if kinds[k] == O.CUBOID:
            counts[:, k] = O.cuboid_face_counts(params[:, k, 0:3].detach().float(), n)
    return counts


def sample(params, kinds, u, counts):
    """O.sample_primitives in the dtype of `params` with the face quotas given, not recounted."""
    out = []
    dt = params.dtype
    for k in range(params.shape[1]):
        v, q, t = params[:, k, 0:3], params[:, k, 3:7], params[:, k, 7:10]
        if kinds[k] == O.SPHERE:
            out.append(O.sphere_sampling(v, q, t, u[:, k, :, 0].to(dt), u[:, k, :, 1].to(dt)))
        else:
            c = O.cuboid_canonical(u[:, k].to(dt), counts[:, k])
            out.append(O.transform_points(c * v[:, None, :], q, t))
    return torch.cat(out, 1)


def sampler_ref(params, kinds, u, W, dtype=torch.float64):
    """points [B,K*n,3] and grad_params [B,K,10] of (sample * W).sum() in `dtype`."""
    counts = face_counts(params, kinds, u.shape[2])
    p = _leaf(params, dtype)
    pts = sample(p, kinds, u, counts)
    (pts * W.to(dtype)).sum().backward()
    return pts.detach(), p.grad


def mesh_ref(params, kinds, templates, W, dtype=torch.float64):
    """vertices and grad_params of the primitive-to-mesh op: transform_points(template * v, q, t) per primitive, then cat
    (the construction of test_meshing.py), in `dtype`.  templates {kind: [P,3] fp32}."""
    p = _leaf(params, dtype)
    verts = torch.cat([O.transform_points(templates[k].to(dtype)[None] * p[:, i, None, 0:3], p[:, i, 3:7], p[:, i, 7:10])
                       for i, k in enumerate(kinds)], 1)
    (verts * W.to(dtype)).sum().backward()
    return verts.detach(), p.grad


def chamfer_sampler_ref(params, kinds, u, gt, idx1, idx2, gl, w1, w2, dtype=torch.float64):
    """grad_params [B,K,10] of  sum_b gl_b (w1/N sum_i |p_i - gt[idx1_i]| + w2/M sum_j |gt_j - p[idx2_j]|),  p = the sampled
    cloud: ChamferDistanceLoss (non-squared distances, O.chamfer_loss) with the nearest neighbours GIVEN (the GPU's)."""
    counts = face_counts(params, kinds, u.shape[2])
    p = _leaf(params, dtype)
    pts = sample(p, kinds, u, counts)
    g = gt.to(dtype)
    B, N, _ = pts.shape
    M = g.shape[1]
    near1 = torch.gather(g, 1, idx1.long()[..., None].expand(B, N, 3))
    near2 = torch.gather(pts, 1, idx2.long()[..., None].expand(B, M, 3))
    d1 = torch.sqrt(((pts - near1) ** 2).sum(-1))
    d2 = torch.sqrt(((g - near2) ** 2).sum(-1))
    loss = (gl.to(dtype) * (w1 / N * d1.sum(1) + w2 / M * d2.sum(1))).sum()
    loss.backward()
    return p.grad


# ----------------------------------------------------------------------------- cube quota ties
CUBE_TIES = {3: [0, 0, 0, 0, 0, 3], 6: [1, 1, 1, 1, 1, 1], 9: [2, 2, 2, 2, 2, -1], 15: [2, 2, 2, 2, 2, 5], 21: [4, 4, 4, 4, 4, 1]}


def cube_params(gen, extent, t_abs, B=4):
    """[B,1,10]: cubes of half extent `extent` (every n * area / total is an exact tie or an exact integer), poses from the
    set, translations with |t|_inf = t_abs."""
    q = poses()[torch.tensor([3, 20, 71, 140][:B])]
    t = t_abs * (torch.rand(B, 3, generator=gen) * 2 - 1)
    t[:, 0] = t_abs
    v = torch.full((B, 3), extent)
    return torch.cat([v, q, t], 1)[:, None, :].contiguous()
