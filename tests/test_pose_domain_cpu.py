"""The float64 reference of tests/pose_domain_ref.py checked by itself on the CPU, and the margin it leaves under the GPU bar.

The fp32 oracle against the float64 oracle over the pose set, by block_rel_err (bar REF_BAR = 5.5e-5; the GPU tests of
test_pose_domain.py hold the kernels to 1e-4 by the same measure).  Measured maxima on the inputs below:

    op          out        grad_points / grad_v   grad_q     grad_t
    transform   1.48e-06   2.12e-06               3.41e-05   9.45e-07
    sphere      2.87e-07   2.17e-06               2.78e-05   3.99e-07
    cuboid      5.04e-07   3.21e-06               3.10e-05   6.75e-07

The grad_q figure depends on the draw: a hair beside an integer angle (-1e-4, 0.9999) the fp32 rounding of h = pi * (q3 mod 1)
is 2.4e-4 of sin h, and with the zero or the tiny axis only the floor of the measure absorbs it -- by the size of that pose's
block against the median block, 2e-5 to 1.1e-4 over other seeds and point distributions (pose_domain_ref.conditioned).
"""
import pytest
import torch

import pose_domain_ref as P
from conftest import rel_err
from oracle import vpn_oracle as O

N_T, N_S = 70, 77


def test_pose_set_and_rotations():
    q = P.poses()
    assert q.shape == (P.POSE_COUNT, 4) and q.dtype == torch.float32
    assert torch.equal(q, P.poses())                                         # fixed, no randomness
    assert float(P.quat_length(q).min()) >= P.MIN_LENGTH
    R = O.rotation_matrices(q.double())
    eye = torch.eye(3, dtype=torch.float64).expand_as(R)
    assert float((R @ R.transpose(1, 2) - eye).abs().max()) <= 1e-12
    assert float((torch.linalg.det(R) - 1).abs().max()) <= 1e-12
    # periodic in the angle
    q3 = q.double().clone()
    q3[:, 3] += 3
    assert float((O.rotation_matrices(q3) - R).abs().max()) <= 1e-12
    # -0.0 is 0.0
    neg = torch.signbit(q[:, 3]) & (q[:, 3] == 0)
    pos = ~torch.signbit(q[:, 3]) & (q[:, 3] == 0)
    assert int(neg.sum()) == int(pos.sum()) == len(P.AXES) and torch.equal(q[neg, :3], q[pos, :3])
    assert torch.equal(R[neg], R[pos])
    assert torch.equal(O.rotation_matrices(q[neg]), O.rotation_matrices(q[pos]))


def test_block_rel_err_measure():
    b = torch.tensor([[1.0, -2.0], [1e-3, 0.0], [0.0, 0.0], [100.0, 1.0]])
    a = b.clone()
    assert P.block_rel_err(a, b) == 0.0
    a[1, 0] = 2e-3                                                           # a small block entirely wrong
    med = 1e-3                                                               # block sizes 0, 1e-3, 2, 100: torch.median is the lower middle one
    assert abs(P.block_rel_err(a, b) - 1e-3 / (1e-3 + 1e-3 * med)) < 1e-9
    assert rel_err(a, b) <= 1e-4                                             # ... which the norm-wise measure does not see
    a = b.clone()
    a[2, 1] = 1e-9                                                           # a block that is zero in truth: held to the floor
    assert abs(P.block_rel_err(a, b) - 1e-9 / (1e-3 * med)) < 1e-9
    a[0, 0] = float('nan')
    assert P.block_rel_err(a, b) == float('inf')


def _transform_case():
    gen = torch.Generator().manual_seed(1301)
    q = P.poses()
    B = q.shape[0]
    pts = torch.rand(B, N_T, 3, generator=gen) - 0.5
    t = 0.35 * (torch.rand(B, 3, generator=gen) * 2 - 1)
    W = torch.randn(B, N_T, 3, generator=gen)
    return pts, q, t, W


def _sampler_case(kind):
    gen = torch.Generator().manual_seed(1302 + kind)
    params = P.pose_params(gen, K=1)
    B = params.shape[0]
    u = torch.rand(B, 1, N_S, 3, generator=gen)
    W = torch.randn(B, N_S, 3, generator=gen)
    return params, [kind], u, W


def _report(name, errs):
    print('%-10s' % name + '  '.join('%s %.2e' % kv for kv in errs.items()))
    for k, e in errs.items():
        assert e <= P.REF_BAR, (name, k, e)


def test_fp32_oracle_transform_within_margin():
    pts, q, t, W = _transform_case()
    r64, r32 = P.transform_ref(pts, q, t, W), P.transform_ref(pts, q, t, W, torch.float32)
    _report('transform', {k: P.block_rel_err(a, b) for k, a, b in zip(('out', 'grad_points', 'grad_q', 'grad_t'), r32, r64)})


@pytest.mark.parametrize('kind', [O.SPHERE, O.CUBOID])
def test_fp32_oracle_sampler_within_margin(kind):
    params, kinds, u, W = _sampler_case(kind)
    (p64, g64), (p32, g32) = P.sampler_ref(params, kinds, u, W), P.sampler_ref(params, kinds, u, W, torch.float32)
    # the statement with the quotas handed over is the oracle's own sampler in fp32
    pc = params.clone().requires_grad_(True)
    assert torch.equal(O.sample_primitives(pc, kinds, u), p32)
    errs = {'out': P.block_rel_err(P.prim_blocks(p32, N_S), P.prim_blocks(p64, N_S))}
    errs.update({k: float(e.max()) for k, e in P.param_group_errors(g32, g64).items()})
    _report('sphere' if kind == O.SPHERE else 'cuboid', errs)


def test_norm_wise_measure_misses_a_wrong_pose():
    """The gap this suite closes: the grad_q block with the smallest non-zero magnitude, negated -- entirely wrong -- passes the
    norm-wise 1e-4 of every existing sampler / transform / mesh test and fails the per-block measure."""
    pts, q, t, W = _transform_case()
    gq64, gq32 = P.transform_ref(pts, q, t, W)[2], P.transform_ref(pts, q, t, W, torch.float32)[2]
    size = gq32.abs().amax(1)
    i = int(torch.where(size > 0, size, torch.full_like(size, float('inf'))).argmin())
    print('grad_q blocks: largest %.3g, median %.3g, the negated one %.3g' % (size.max(), size.median(), size[i]))
    bad = gq32.clone()
    bad[i] = -bad[i]
    assert rel_err(bad, gq64) <= 1e-4
    assert P.block_rel_err(bad, gq64) > 1e-4
    assert P.block_rel_err(gq32, gq64) <= P.REF_BAR


@pytest.mark.parametrize('n,counts', sorted(P.CUBE_TIES.items()))
def test_cube_quota_ties(n, counts):
    v = torch.full((1, 3), 0.1)
    assert O.cuboid_face_counts(v, n).tolist() == [counts]
    assert O.cuboid_face_counts(v.double(), n).tolist() == [counts]
    assert P.face_counts(torch.cat([v, torch.zeros(1, 7)], 1)[:, None], [O.CUBOID], n).tolist() == [[counts]]
    if n == 9:
        # a negative last quota, a fifth range [8, 10) that runs past n: points 0..8 snap to faces 0,0,1,1,2,2,3,3,4
        u = torch.full((1, n, 3), 0.75)
        c = O.cuboid_canonical(u, torch.tensor([counts], dtype=torch.int32))[0]
        faces = [0, 0, 1, 1, 2, 2, 3, 3, 4]
        for p, f in enumerate(faces):
            want = [0.5, 0.5, 0.5]
            want[f // 2] = -1.0 if f % 2 else 1.0
            assert c[p].tolist() == want, (p, f, c[p])
