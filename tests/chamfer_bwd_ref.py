"""The Chamfer backward (vpn_chamfer_bwd, csrc/chamfer.hip) stated in float64, the bar it is held to per element, and the
cases it is held on.  Plain numpy on the CPU: nothing here imports the package or the oracle (the fused-kernel batches at the
end use the float64 sampler of tests/pose_domain_ref.py, imported where they are built).

THE STATEMENT (`statement`).  loss_b = wA/Na sum_r |A_r - B_iA[r]| + wB/Nb sum_e |B_e - A_iB[e]| with the nearest neighbours
GIVEN (iA [B,Na] into cloud B, iB [B,Nb] into cloud A), upstream gradient g_b.  Row r of d/dA:

    ca (A_r - B_iA[r]) / |A_r - B_iA[r]|  +  sum over e with iB[e] == r of  cb (A_r - B_e) / |A_r - B_e|,
    ca = g_b wA / Na,  cb = g_b wB / Nb.

The distances are recomputed in float64 from the fp32 points and the index, never taken from the kernel's `dist` input: a stale
or mis-indexed dist shows.  Swapping the roles of the clouds gives the other gradient.  Dense autograd cannot be this
reference: torch's sqrt backward puts 0/0 = NaN on every zero-distance entry of the [N,M] matrix, selected or not.
Beside the gradient: n_r, the number of scatter terms of row r, and S_r[c] = sum_k |t_k[c]| over the row's n_r + 1 terms.

NaN rows.  A coincident selected pair is 0/0 = NaN, in the statement as in the kernel ("a coincident pair gives NaN like the
reference's autograd", include/vpn_hip.h): the query's row, and the target's row of the other gradient.  A point with a NaN
coordinate makes every term it enters NaN.  An index outside the other cloud (what the filtered scans return for a query with
a NaN or infinite coordinate) is a query without a neighbour: its own row is NaN, it scatters nothing.

THE BAR (`bar`), element-wise, derived and not measured:   |got - ref64| <= (n_r + 8) * 2^-23 * S_r[c].
With u = 2^-24, the unit roundoff of fp32 (chamfer.hip is built with -ffp-contract=off and without fast-math, build.py:
every operation below is one correctly rounded IEEE operation, the divide and the square root included, which is hipcc's
default and is what the file's bit-exactness contract of the forward already relies on):
  * one term t = fl(fl(fl(fl(g w) / N) / d) * fl(a - c)): two roundings for g w / N ((float)N is exact), one for the divide
    by d, one for the subtraction, one for the product: 5 u |t|;
  * d itself is the FORWARD's fp32 value sqrtf(((dx dx) + (dy dy)) + (dz dz)), not one rounding of the true distance: each
    difference carries u, each square 2 u + u, the two additions one u each on top of the largest summand error (all summands
    are positive: no cancellation), so d^2 carries at most 5 u and d at most 2.5 u + u = 3.5 u.  (The issue that asked for
    this test counted one rounding for d, six per term; the count from the code is 8.5.)
  * accumulating the n_r + 1 terms of a row in any order (both launch paths add with float atomics: the order is arbitrary)
    costs at most n_r roundings of a partial sum, each partial sum at most S: n_r u S.
First order, every term at its worst at once:  (n_r + 8.5) u S.  The bar is (n_r + 8) * 2 u * S = (2 n_r + 16) u S: the
constant 8 of the issue stands, it covers the first-order bound with a factor >= 1.88 left for the second-order terms
((1 + u)^k - 1 - k u, below 1e-5 of the first order for k <= 12300 + 9).  The bar is relative to S_r, not to |ref|: a row
whose own term and scatter terms cancel is held to the size of its terms.
Domain of the non-coincident cases: |coordinate| <= 2000 and selected distances >= 1e-6, so no term (>= 1e-10 for the
weights used) or sum underflows and the relative bounds above hold.

The norm-wise bar of the rest of the suite, max|got - ref| / max|ref| <= 1e-4 over a tensor, is kept as a second assertion."""
import functools

import numpy as np

U23 = 2.0 ** -23
NORM_BAR = 1e-4


# ----------------------------------------------------------------------------- the statement
def statement(pa, pb, iA, iB, gl, wA, wB, dtype=np.float64):
    """d/dA of the loss above: (grad [B,Na,3], n [B,Na] int64, S [B,Na,3]) in `dtype` from fp32 pa [B,Na,3], pb [B,Nb,3],
    integer iA [B,Na], iB [B,Nb], gl [B].  Rows that are NaN under the contract are NaN in grad."""
    pa, pb = np.asarray(pa, np.float32).astype(dtype), np.asarray(pb, np.float32).astype(dtype)
    iA, iB, gl = np.asarray(iA).astype(np.int64), np.asarray(iB).astype(np.int64), np.asarray(gl, np.float32).astype(dtype)
    B, Na, _ = pa.shape
    Nb = pb.shape[1]
    grad, S, n = np.zeros((B, Na, 3), dtype), np.zeros((B, Na, 3), dtype), np.zeros((B, Na), np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        for b in range(B):
            ca, cb = gl[b] * dtype(wA) / dtype(Na), gl[b] * dtype(wB) / dtype(Nb)
            ok = (iA[b] >= 0) & (iA[b] < Nb)
            diff = pa[b] - pb[b][np.where(ok, iA[b], 0)]
            t = ca * diff / np.sqrt((diff * diff).sum(1))[:, None]
            t[~ok] = np.nan
            grad[b], S[b] = t, np.abs(t)
            e = np.nonzero((iB[b] >= 0) & (iB[b] < Na))[0]
            r = iB[b][e]
            diff = pa[b][r] - pb[b][e]
            t = cb * diff / np.sqrt((diff * diff).sum(1))[:, None]
            np.add.at(grad[b], r, t)
            np.add.at(S[b], r, np.abs(t))
            n[b] = np.bincount(r, minlength=Na)
    return grad, n, S


def both(case, i1, i2, dtype=np.float64):
    """((grad_p1, n, S), (grad_p2, n, S)) of a case with idx1 [B,N] and idx2 [B,M]."""
    return (statement(case['p1'], case['p2'], i1, i2, case['gl'], case['w1'], case['w2'], dtype),
            statement(case['p2'], case['p1'], i2, i1, case['gl'], case['w2'], case['w1'], dtype))


_NN = {}


def neighbours(case, nn):
    """(idx1 [B,N], idx2 [B,M]) int64 of the dense CPU search nn(p1, p2) -> (_, idx1, _, idx2) on torch tensors (the oracle's
    chamfer_nn_ieee), one sample at a time; computed once per case and shared by the tests that need it."""
    import torch
    if case['name'] not in _NN:
        res = [nn(torch.from_numpy(case['p1'][b:b + 1]), torch.from_numpy(case['p2'][b:b + 1])) for b in range(len(case['gl']))]
        _NN[case['name']] = tuple(np.concatenate([r[k].numpy() for r in res]).astype(np.int64) for k in (1, 3))
    return _NN[case['name']]


def bar(n, S):
    return (n[..., None] + 8.0) * U23 * S


def forward_dist32(pa, pb, iA):
    """The forward's fp32 distance of every (r, iA[r]): sqrtf(((dx dx) + (dy dy)) + (dz dz)), each operation rounded."""
    pa, pb = np.asarray(pa, np.float32), np.asarray(pb, np.float32)
    d = pa - np.take_along_axis(pb, np.asarray(iA).astype(np.int64)[..., None], 1)
    return np.sqrt(((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2]))


def evaluate32(pa, pb, iA, iB, gl, wA, wB, rng=None, dist_a=None, dist_b=None):
    """The closed form the way the kernels evaluate it, in fp32 numpy: coef = ((g w) / N) / d with the forward's fp32 d, the
    term coef * (a - c), the row's terms added one by one in fp32 -- the own term first, the scatter terms in the order of a
    permutation drawn from `rng` (None: index order).  grad [B,Na,3] fp32.  In-range indices only."""
    f = np.float32
    pa, pb, gl = np.asarray(pa, f), np.asarray(pb, f), np.asarray(gl, f)
    iA, iB = np.asarray(iA).astype(np.int64), np.asarray(iB).astype(np.int64)
    B, Na, _ = pa.shape
    Nb = pb.shape[1]
    dA = forward_dist32(pa, pb, iA) if dist_a is None else dist_a
    dB = forward_dist32(pb, pa, iB) if dist_b is None else dist_b
    out = np.zeros((B, Na, 3), f)
    with np.errstate(invalid='ignore', divide='ignore'):
        for b in range(B):
            ca, cb = (gl[b] * f(wA)) / f(Na), (gl[b] * f(wB)) / f(Nb)
            acc = (ca / dA[b])[:, None] * (pa[b] - pb[b][iA[b]])
            order = np.arange(Nb) if rng is None else rng.permutation(Nb)
            t = (cb / dB[b][order])[:, None] * (pa[b][iB[b][order]] - pb[b][order])
            rows = iB[b][order]
            # fp32 sequential adds in `order`: rows are independent, so add the k-th term of every row at once
            rank = np.zeros(Nb, np.int64)
            seen = {}
            for pos, r in enumerate(rows.tolist()):
                rank[pos] = seen.get(r, 0)
                seen[r] = rank[pos] + 1
            by_rank = np.argsort(rank, kind='stable')
            cut = np.searchsorted(rank[by_rank], np.arange(int(rank.max()) + 2))
            for k in range(len(cut) - 1):
                sel = by_rank[cut[k]:cut[k + 1]]
                acc[rows[sel]] = acc[rows[sel]] + t[sel]
            out[b] = acc
    return out


# ----------------------------------------------------------------------------- the launch path of a shape
def path_of(N, M, cb_max_points, lds_default):
    """'global' | 'lds_raised' | 'lds' as vpn_chamfer_bwd decides: the LDS kernel when both clouds have at most
    cb_max_points points, its dynamic LDS (12 B per point of the cloud whose gradient it writes) above lds_default bytes
    needs the raised limit."""
    if N > cb_max_points or M > cb_max_points:
        return 'global'
    return 'lds_raised' if max(N, M) * 12 > lds_default else 'lds'


# ----------------------------------------------------------------------------- the cases
def _case(name, p1, p2, gl, w1=0.7, w2=1.3, **meta):
    f = np.float32
    p1, p2 = np.ascontiguousarray(p1, f), np.ascontiguousarray(p2, f)
    meta.setdefault('nan', False)
    meta.setdefault('path', 'lds')
    return {'name': name, 'p1': p1, 'p2': p2, 'gl': np.asarray(gl, f), 'w1': float(w1), 'w2': float(w2),
            'N': p1.shape[1], 'M': p2.shape[1], 'meta': meta}


def _gl(B):
    return np.array([0.7, 0.0, -1.3, 1.1, -0.6][:B] if B == 3 else [1.1, -0.6, 0.8][:B], np.float32)


def _clouds(seed, B, N, M):
    rng = np.random.RandomState(seed)
    return rng.rand(B, N, 3).astype(np.float32) - 0.5, rng.rand(B, M, 3).astype(np.float32) - 0.5, rng


def plain(name, N, M, B, seed, path):
    """Uniform clouds in [-0.5, 0.5)^3; gl of B = 3 holds a 0 and a negative entry."""
    p1, p2, _ = _clouds(seed, B, N, M)
    return _case(name, p1, p2, _gl(B), path=path)


def hub(N, M, hubs=1, seed=11, B=2):
    """The query cloud p1 in a ball of radius 0.05 about the origin; `hubs` points of p2 at distance 0.3 from it on the x axis
    (one on either side for two), every other point of p2 between 5 and 9 away.  The hub rows of grad_p2 receive all N
    scatter terms between them, every other row of grad_p2 none."""
    rng = np.random.RandomState(seed)
    d = rng.randn(B, N, 3)
    p1 = 0.05 * d / np.linalg.norm(d, axis=2, keepdims=True) * rng.rand(B, N, 1) ** (1.0 / 3.0)
    d = rng.randn(B, M, 3)
    p2 = d / np.linalg.norm(d, axis=2, keepdims=True) * (5.0 + 4.0 * rng.rand(B, M, 1))
    rows = [M // 3] if hubs == 1 else [M // 3, M - 1]
    for h, x in zip(rows, (0.3, -0.3)):
        p2[:, h] = (x, 0.0, 0.0)
    return _case('hub%d_%dx%d' % (hubs, N, M), p1, p2, _gl(B), hub_rows=rows, hub_total=N,
                 path='global' if max(N, M) > 12288 else 'lds')


def unreferenced(seed=12):
    """(200, 300): the last 40 points of p2 lie 10 and more away from everything: nobody's nearest neighbour, so their rows
    of grad_p2 are their direct term alone (n_r = 0)."""
    p1, p2, rng = _clouds(seed, 2, 200, 300)
    far = np.arange(260, 300)
    p2[:, far] = 10.0 + 5.0 * rng.rand(2, 40, 3).astype(np.float32)
    return _case('unreferenced', p1, p2, _gl(2), unref_p2=far.tolist())


def cancel(seed=13):
    """(64, 64), w1 = w2, so ca = cb = c.  p1[0] = P; p2[0] = P + 0.01 x is P's nearest neighbour (own term -c x, and its
    scatter term -c x again); p2[1], p2[2] = P - 0.02 x -+ 1e-4 y have P as their nearest neighbour too (+c x each, up to
    the tilt): the four terms of row 0 of grad_p1 cancel to 1e-2 of their size.  Everything else lies 2 to 3 away."""
    p1, p2, _ = _clouds(seed, 2, 64, 64)
    p1, p2 = p1 + 2.5, p2 + 2.5
    P = np.array([0.125, -0.25, 0.0625], np.float32)
    p1[:, 0] = P
    p2[:, 0] = P + np.array([0.01, 0.0, 0.0], np.float32)
    p2[:, 1] = P + np.array([-0.02, 1e-4, 0.0], np.float32)
    p2[:, 2] = P + np.array([-0.02, -1e-4, 0.0], np.float32)
    return _case('cancel', p1, p2, np.array([1.1, 0.8], np.float32), w1=1.0, w2=1.0, cancel_row=0)


def translated(case):
    """The case shifted by (1000, -1000, 500) and rounded to fp32: new fp32 inputs on which the differences are as exact as
    before relative to their own size, so the bar is unchanged."""
    s = np.array([1000.0, -1000.0, 500.0], np.float32)
    meta = dict(case['meta'])
    return _case(case['name'] + '_translated', case['p1'] + s, case['p2'] + s, case['gl'], case['w1'], case['w2'], **meta)


def close(seed=14):
    """(130, 140): points 5 k of p1, k < 8, have a point of p2 at 1e-6 beside them (an offset of some 30 ulp of the coordinate:
    the direction is well defined on the fp32 inputs), among ordinary pairs."""
    p1, p2, _ = _clouds(seed, 2, 130, 140)
    rows = [5 * k for k in range(8)]
    for k, r in enumerate(rows):
        q = p1[:, r].copy()
        q[:, k % 3] += np.float32(1e-6)
        short = q[:, k % 3].astype(np.float64) - p1[:, r, k % 3] < 1e-6          # the fp32 sum fell just short of 1e-6: one ulp on
        q[:, k % 3] = np.where(short, np.nextafter(q[:, k % 3], np.float32(np.inf)), q[:, k % 3])
        p2[:, 7 * k + 1] = q
    return _case('close', p1, p2, _gl(2), close_p1=rows, close_p2=[7 * k + 1 for k in range(8)])


def zero_weight(which, seed=15):
    p1, p2, _ = _clouds(seed, 3, 63, 65)
    w = (0.0, 1.3) if which == 1 else (0.7, 0.0)
    return _case('zero_w%d' % which, p1, p2, _gl(3), w1=w[0], w2=w[1], zero=which)


def coincident(seed=16, k=3):
    """(200, 150): p1[17 i] == p2[11 i + 2] bit for bit, i < k.  Those rows of grad_p1 and of grad_p2 are NaN (0/0)."""
    p1, p2, _ = _clouds(seed, 2, 200, 150)
    r1, r2 = [17 * i for i in range(k)], [11 * i + 2 for i in range(k)]
    p1[:, r1] = p2[:, r2]
    return _case('coincident', p1, p2, _gl(2), nan=True, nan_p1=r1, nan_p2=r2)


def nan_points(N, M, seed=17):
    """One point of all NaN in each cloud, sample 0: p1[0, N // 2] and p2[0, M // 3].  Indices come from the forward under
    test; the rows that touch a NaN point (its own, and a row that scatters from it or to it) are NaN, every other is held."""
    p1, p2, _ = _clouds(seed, 2, N, M)
    p1[0, N // 2] = np.nan
    p2[0, M // 3] = np.nan
    return _case('nan_%dx%d' % (N, M), p1, p2, _gl(2), nan=True, nan_p1=[N // 2], nan_p2=[M // 3])


RAGGED = ((1, 1), (1, 7), (5, 1), (63, 65), (1025, 1023))
LDS_RAISE = ((5461, 40), (5462, 40), (40, 5462))
LDS_MAX = ((12288, 33), (33, 12288))
GLOBAL_MIN = ((12289, 33), (33, 12289), (12289, 700))
HUBS = ((700, 64), (12289, 33), (33, 12289))


@functools.lru_cache(maxsize=None)
def cases():
    """{name: case}, in an order in which no shape that needs the raised LDS limit is the first LDS-path shape."""
    out = []
    for i, (N, M) in enumerate(RAGGED):
        out.append(plain('ragged_%dx%d' % (N, M), N, M, 3, 100 + i, 'lds'))
    for i, (N, M) in enumerate(LDS_RAISE):
        out.append(plain('lds_raise_%dx%d' % (N, M), N, M, 2, 110 + i, 'lds' if max(N, M) == 5461 else 'lds_raised'))
    for i, (N, M) in enumerate(LDS_MAX):
        out.append(plain('lds_max_%dx%d' % (N, M), N, M, 2, 120 + i, 'lds_raised'))
    for i, (N, M) in enumerate(GLOBAL_MIN):
        out.append(plain('global_min_%dx%d' % (N, M), N, M, 2, 130 + i, 'global'))
    for N, M in HUBS:
        out.append(hub(N, M))
    out.append(hub(700, 64, hubs=2))
    out.append(hub(12289, 33, hubs=2))
    out += [unreferenced(), cancel(), close(), zero_weight(1), zero_weight(2), coincident()]
    by = {c['name']: c for c in out}
    for name in ('ragged_63x65', 'hub1_700x64', 'hub1_12289x33', 'cancel', 'unreferenced'):
        out.append(translated(by[name]))
    return {c['name']: c for c in out}


def case_names():
    return list(cases())


# ----------------------------------------------------------------------------- batches of the fused kernel
FUSED_K, FUSED_N = 4, 64
FUSED_M = (129, 300, 1025, 7680)


def fused_batch(gen, M, hub_batch, B=2, K=FUSED_K):
    """params [B,K,10], kinds, gt [B,M,3], gl [B] for vpn_sample_chamfer_bwd, drawn from the torch generator `gen`.  Poses from
    the pose set, extents in [0.06, 0.1].  hub_batch: primitive 0 at the origin, the others (K <= 7) at distance 1 along the axes --
    the edge of the translations' domain, |t|_inf <= 1 (the network's head, and the |t| = 1 of test_pose_domain's thin cases) --
    and the GT cloud within 0.3 of the origin: a GT point is at most 0.3 + 0.1 sqrt(3) from a point of primitive 0 and at least
    1 - 0.3 - 0.1 sqrt(3) from any other -- every GT point's nearest predicted point lies on primitive 0, so each wave of that
    primitive's workgroup finds a match in every entry it scans and its match list fills to its capacity.  Otherwise the
    primitives sit at the corners (+-0.25 each coordinate: within the |t| <= 0.35 of the suite's random parameters) of a
    tetrahedron and the GT is drawn beside them in equal parts, in the octant
    beyond each centre: the M / K scatter terms of a primitive then add up instead of cancelling, which keeps the fp32
    oracle's own sum (the measure the draws are chosen by) well conditioned at M = 7680."""
    import torch
    import pose_domain_ref as P
    q = P.poses()[torch.randperm(P.POSE_COUNT, generator=gen)[:B * K]].reshape(B, K, 4)
    v = 0.06 + 0.04 * torch.rand(B, K, 3, generator=gen)
    if hub_batch:
        t = torch.zeros(B, K, 3)
        for k in range(1, K):
            t[:, k, (k - 1) % 3] = -1.0 if (k - 1) // 3 % 2 else 1.0
        d = torch.randn(B, M, 3, generator=gen)
        gt = 0.3 * d / d.norm(dim=2, keepdim=True) * torch.rand(B, M, 1, generator=gen)
    else:
        corners = 0.25 * torch.tensor([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
        t = corners[torch.arange(K) % 4][None].expand(B, K, 3).clone()
        gt = t[:, torch.arange(M) % K] + 0.05 + 0.15 * torch.rand(B, M, 3, generator=gen)
    params = torch.cat([v, q, t], 2).contiguous()
    gl = torch.rand(B, generator=gen) + 0.5
    return params, [k % 2 for k in range(K)], gt.contiguous(), gl
