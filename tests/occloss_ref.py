"""Float64 restatement of the occupancy loss (csrc/occloss.hip; include/vpn_hip.h, vpn_occloss_fwd / vpn_occloss_bwd; DESIGN.md
4.31) in plain numpy: the forward and the ANALYTIC gradient as the header states them, no autograd.  With dtype=np.float32
every operation is rounded by itself (numpy's own arithmetic), which measures what fp32 costs: the `own` error of the tests."""
import math

import numpy as np

SPHERE, CUBOID = 0, 1
PI32 = 3.1415927410125732          # the fp32 pi of csrc/vpn_common.h


def _quiet():
    return np.errstate(all='ignore')


def pose(q, dt=np.float64):
    """make_pose of csrc/vpn_common.h on q [...,4] -> dict: R [...,3,3], the unit quaternion x y z w, sh, ch, inv_len."""
    q = np.asarray(q).astype(dt)
    two, pi = dt(2), dt(PI32)
    r = q[..., 3] - np.floor(q[..., 3])
    h = ((r * two) * pi) / two
    sh, ch = np.sin(h), np.cos(h)
    a, b, c, d = q[..., 0] * sh, q[..., 1] * sh, q[..., 2] * sh, ch
    ln = np.sqrt(a * a + b * b + c * c + d * d)
    x, y, z, w = a / ln, b / ln, c / ln, d / ln
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    R = np.stack([np.stack([x2 - y2 - z2 + w2, two * (xy - zw), two * (xz + yw)], -1),
                  np.stack([two * (xy + zw), -x2 + y2 - z2 + w2, two * (yz - xw)], -1),
                  np.stack([two * (xz - yw), two * (yz + xw), -x2 - y2 + z2 + w2], -1)], -2)
    return dict(R=R, x=x, y=y, z=z, w=w, sh=sh, ch=ch, inv_len=dt(1) / ln)


def pose_backward(P, q, g):
    """dL/dR g [...,3,3] (g[..., j, i] = dL/dR[j][i]) -> dL/dq [...,4]: through the matrix entries, the normalisation and the
    half-angle map, pose_backward of csrc/vpn_common.h."""
    dt = g.dtype.type
    x, y, z, w, two = P['x'], P['y'], P['z'], P['w'], dt(2)
    G = lambda j, i: g[..., j, i]
    gx = two * (x * G(0, 0) + y * G(0, 1) + z * G(0, 2) + y * G(1, 0) - x * G(1, 1) - w * G(1, 2) + z * G(2, 0) + w * G(2, 1) - x * G(2, 2))
    gy = two * (-y * G(0, 0) + x * G(0, 1) + w * G(0, 2) + x * G(1, 0) + y * G(1, 1) + z * G(1, 2) - w * G(2, 0) + z * G(2, 1) - y * G(2, 2))
    gz = two * (-z * G(0, 0) - w * G(0, 1) + x * G(0, 2) + w * G(1, 0) - z * G(1, 1) + y * G(1, 2) + x * G(2, 0) + y * G(2, 1) + z * G(2, 2))
    gw = two * (w * G(0, 0) - z * G(0, 1) + y * G(0, 2) + z * G(1, 0) + w * G(1, 1) - x * G(1, 2) - y * G(2, 0) + x * G(2, 1) + w * G(2, 2))
    dot = x * gx + y * gy + z * gz + w * gw
    ha, hb, hc, hd = ((gx - x * dot) * P['inv_len'], (gy - y * dot) * P['inv_len'], (gz - z * dot) * P['inv_len'],
                      (gw - w * dot) * P['inv_len'])
    q = np.asarray(q).astype(dt)
    gh = (q[..., 0] * ha + q[..., 1] * hb + q[..., 2] * hc) * P['ch'] - hd * P['sh']
    return np.stack([ha * P['sh'], hb * P['sh'], hc * P['sh'], gh * dt(PI32)], -1)


def sigmoid(z):
    """1 / (1 + exp(-z)) for z >= 0, exp(z) / (1 + exp(z)) below."""
    one = z.dtype.type(1)
    with _quiet():
        e = np.exp(-np.abs(z))
        return np.where(z >= 0, one, e) / (one + e)


def _per_sample(queries, B):
    queries = np.asarray(queries)
    return np.broadcast_to(queries[None], (B,) + queries.shape) if queries.ndim == 2 else queries


def local(params, kinds, queries, dt=np.float64):
    """x~ [B,Q,K,3] = R^T (x - t) / v and m [B,Q,K] (x~.x~ for a sphere, max |x~_i| for a cuboid, NaN where any x~_i is one), with
    the pose of every primitive."""
    p = np.asarray(params).astype(dt)
    B = p.shape[0]
    x = _per_sample(queries, B).astype(dt)
    v, t, P = p[:, :, 0:3], p[:, :, 7:10], pose(p[:, :, 3:7], dt)
    R = P['R']
    with _quiet():
        d = x[:, :, None, :] - t[:, None, :, :]
        y = np.stack([R[:, None, :, 0, i] * d[..., 0] + R[:, None, :, 1, i] * d[..., 1] + R[:, None, :, 2, i] * d[..., 2]
                      for i in range(3)], -1) / v[:, None]
        sphere = y[..., 0] * y[..., 0] + y[..., 1] * y[..., 1] + y[..., 2] * y[..., 2]
        cuboid = np.where(np.isnan(y).any(-1), dt(np.nan), np.abs(y).max(-1))
    is_sphere = np.array([k == SPHERE for k in kinds])
    return y, np.where(is_sphere[None, None, :], sphere, cuboid), v, P


def labels_float(labels, dt=np.float64):
    labels = np.asarray(labels)
    return (labels != 0).astype(dt) if labels.dtype == np.uint8 else labels.astype(dt)


def forward(params, kinds, queries, labels, tau, dt=np.float64):
    """dict: out [2] = (sum bce, sum ov) / (B Q); lse [B,Q], s [B,Q]; bce, ov [B,Q] (0 where skipped); skipped bool [B,Q];
    n_skipped; and what the gradient reuses (y, z, live)."""
    tau = dt(tau)
    y, m, v, P = local(params, kinds, queries, dt)
    B, Q, K = m.shape
    live = np.isfinite(m)                                                      # the primitives of a query that take part
    with _quiet():
        d = m - dt(1)
        z = np.where(live, -d / tau, dt(-np.inf))
        zmax = z.max(-1)
        total = np.where(live, np.exp(z - zmax[..., None]), dt(0)).sum(-1, dtype=dt)
        lse = np.where(np.isfinite(zmax), zmax + np.log(total), zmax)           # -inf: nothing left; +inf: a z_k is
        s = np.where(live, sigmoid(z), dt(0)).sum(-1, dtype=dt)
        x = _per_sample(queries, B)
        yl = np.broadcast_to(labels_float(labels, dt), (B, Q)) if labels is not None else np.zeros((B, Q), dt)
        skipped = ~np.isfinite(x).all(-1) | np.isnan(yl) | ~np.isfinite(lse)
        l0 = np.where(skipped, dt(0), lse)
        bce = np.where(skipped, dt(0), (np.maximum(l0, dt(0)) + np.log1p(np.exp(-np.abs(l0)))) - np.where(skipped, dt(0), yl) * l0)
        r = s - dt(1)
        ov = np.where(skipped | ~(r > 0), dt(0), r * r)
    count = float(B) * float(Q)
    out = np.array([bce.sum(dtype=dt) / dt(count), ov.sum(dtype=dt) / dt(count)], dt)
    return dict(out=out, lse=lse, s=s, bce=bce, ov=ov, skipped=skipped, n_skipped=int(skipped.sum()), y=y, z=z, live=live, v=v,
                pose=P, labels=yl)


def backward(params, kinds, queries, labels, tau, g=(1.0, 0.0), dt=np.float64, fwd=None):
    """dparams [B,K,10] = d (g[0] out[0] + g[1] out[1]) / d params, analytically: c_k, dL/dm_k = -c_k / tau, dm/dx~, the twelve
    sums of a primitive, then (t, v, R) and R -> q."""
    f = fwd if fwd is not None else forward(params, kinds, queries, labels, tau, dt)
    tau, g0, g1 = dt(tau), dt(g[0]), dt(g[1])
    y, z, live, v, P = f['y'], f['z'], f['live'], f['v'], f['pose']
    B, Q, K = z.shape
    count = dt(float(B) * float(Q))
    use = live & ~f['skipped'][..., None]
    with _quiet():
        l = np.where(f['skipped'], dt(0), f['lse'])[..., None]
        yl = np.where(f['skipped'], dt(0), f['labels'])[..., None]
        r = np.where(f['skipped'], dt(0), f['s'] - dt(1))[..., None]
        zz = np.where(use, z, dt(0))
        sg = sigmoid(zz)
        # dL/dm_k = -c_k / tau in the kernel's order: the two factors of c_k that belong to the query are divided by B Q and by
        # -tau first, then meet the factors that belong to the primitive (so the fp32 mode rounds where the kernel rounds)
        a = -(((g0 * (sigmoid(l) - yl)) / count) / tau)
        b = -(((g1 * (dt(2) * np.maximum(r, dt(0)))) / count) / tau)
        dm = np.where(use, a * np.exp(zz - l) + b * (sg * (dt(1) - sg)), dt(0))    # [B,Q,K]
        ys = np.where(use[..., None], y, dt(0))
        axis = np.abs(ys).argmax(-1)                                              # the LOWEST axis attaining the maximum
        onehot = (axis[..., None] == np.arange(3)).astype(dt)
        dcub = onehot * np.sign(ys)                                               # sign(0) = 0
        dsph = dt(2) * ys
        is_sphere = np.array([k == SPHERE for k in kinds])[None, None, :, None]
        gamma = dm[..., None] * np.where(is_sphere, dsph, dcub)                   # [B,Q,K,3]
        Sg = gamma.sum(1, dtype=dt)                                               # [B,K,3]
        G = np.einsum('bqki,bqkl->bkil', gamma, ys).astype(dt)                    # [B,K,3,3]: sum gamma_i x~_l
        R = P['R']                                                                # [B,K,3,3]
        dtr = -np.einsum('bkji,bki->bkj', R, Sg / v)
        dv = -np.stack([G[..., i, i] for i in range(3)], -1) / v
        dR = np.einsum('bkjl,bkl,bkil->bkji', R, v, G) / v[:, :, None, :]         # dR[j][i] = sum_l R[j][l] v_l G[i][l] / v_i
        dq = pose_backward(P, np.asarray(params)[:, :, 3:7], dR.astype(dt))
        t = np.asarray(params).astype(dt)[:, :, 7:10]
        alive = (np.isfinite(v) & (v != 0) & np.isfinite(t)).all(-1) & np.isfinite(R).all((-1, -2))
        out = np.concatenate([dv, dq, dtr], -1).astype(dt)
    return np.where(alive[..., None], out, dt(0))


def errors(params, kinds, queries, labels, tau, g=(1.0, 0.0)):
    """`own`: what fp32 arithmetic alone costs on this input, (losses relative to 1 + |value|, logit and overlap sum per query
    relative to 1 + |value|, gradient relative to max |grad|), the fp32 mode against float64."""
    a, b = forward(params, kinds, queries, labels, tau), forward(params, kinds, queries, labels, tau, np.float32)
    ga, gb = backward(params, kinds, queries, labels, tau, g, fwd=a), backward(params, kinds, queries, labels, tau, g, np.float32, fwd=b)
    rel = lambda got, want: float(np.max(np.abs(got.astype(np.float64) - want) / (1 + np.abs(want)))) if want.size else 0.0
    ok = np.isfinite(a['lse'])
    return (rel(b['out'], a['out']), max(rel(b['lse'][ok], a['lse'][ok]), rel(b['s'], a['s'])),
            float(np.abs(gb.astype(np.float64) - ga).max() / max(np.abs(ga).max(), 1e-300)))


# ---- inputs

def case(B, kinds, Q, seed, shift=0.05, shared=True):
    """Random assemblies as the tests draw them: v in [0.05, 0.3], q012 in (-1, 1), q3 in [-1, 2), t in 0.35 U(-1, 1); queries
    in the cube (-0.5, 0.5)^3; labels uint8 = the occupancy of the SAME assembly shifted by `shift` along every axis."""
    rng = np.random.default_rng(seed)
    K = len(kinds)
    v = rng.uniform(0.05, 0.3, (B, K, 3))
    q = np.concatenate([rng.uniform(-1, 1, (B, K, 3)), rng.uniform(-1, 2, (B, K, 1))], -1)
    t = 0.35 * rng.uniform(-1, 1, (B, K, 3))
    params = np.concatenate([v, q, t], -1).astype(np.float32)
    queries = rng.uniform(-0.5, 0.5, (Q, 3) if shared else (B, Q, 3)).astype(np.float32)
    target = params.copy()
    target[:, :, 7:10] += np.float32(shift)
    return params, queries, occupancy(target, kinds, queries)


def occupancy(params, kinds, queries):
    """uint8 [B,Q]: m <= 1 for some primitive, in float64 on the fp32 inputs."""
    with _quiet():
        return (local(params, kinds, queries)[1] <= 1).any(-1).astype(np.uint8)


def grid_queries(R, lo=-0.5, hi=0.5):
    c = lo + (np.arange(R, dtype=np.float64) + 0.5) * (hi - lo) / R
    z, y, x = np.meshgrid(c, c, c, indexing='ij')
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)


def iou(params, kinds, queries, labels):
    a, b = occupancy(params, kinds, queries).astype(bool), np.asarray(labels) != 0
    return float((a & b).sum()) / max(float((a | b).sum()), 1.0)


def descent_case():
    """One sphere from a displaced start towards a target sphere: (start params fp32 [1,1,10], kinds, queries fp32 [8^3 + 257, 3],
    labels uint8 [1,Q])."""
    rng = np.random.default_rng(5)
    queries = np.concatenate([grid_queries(8), rng.uniform(-0.5, 0.5, (257, 3)).astype(np.float32)])
    target = np.array([[[0.25, 0.2, 0.3, 0.2, -0.4, 0.3, 0.15, 0.05, -0.04, 0.03]]], np.float32)
    start = np.array([[[0.15, 0.15, 0.15, 0.1, 0.2, -0.1, 0.4, -0.08, 0.06, -0.05]]], np.float32)
    return start, (SPHERE,), queries, occupancy(target, (SPHERE,), queries)
