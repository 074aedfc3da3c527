"""Restatement of the volumetric evaluation (csrc/occupancy.hip) in torch, in a chosen dtype (float64 by
default), and the inputs its tests share: grid queries, occupancy of a primitive assembly, the generalized winding number of a
triangle mesh in both layouts, the IoU row from two occupancies, the bookkeeping as a plain Python loop; boxes, ellipsoids over
icospheres, and queries drawn by rejection so that every decision the GPU test compares has a margin."""
import functools
import math

import torch

import pointmesh_ref as PM
import surfeval_ref as SR

SPHERE, CUBOID = 0, 1
W = 5                                   # iou precision recall vol_pred vol_gt
PI32 = 3.1415927410125732               # the fp32 pi of rotate.py:4 (VPN_PI)
FOUR_PI = 4 * math.pi


# ---- queries

def grid_queries(R, lo=-0.5, hi=0.5):
    """fp32 [R^3,3] cell centres: index (iz R + iy) R + ix, coordinate lo + (i + 0.5) (hi - lo) / R in float64, rounded once."""
    c = [lo + (i + 0.5) * (hi - lo) / R for i in range(R)]
    return torch.tensor([[c[ix], c[iy], c[iz]] for iz in range(R) for iy in range(R) for ix in range(R)], dtype=torch.float64).float()


def _per_sample(queries, B):
    return queries[None].expand(B, -1, -1) if queries.dim() == 2 else queries


# ---- primitives

def rotations(q, dtype=torch.float64):
    """make_pose of csrc/vpn_common.h (rotate.py:28-46,59-72) on q [...,4] -> R [...,3,3] in `dtype`."""
    q = q.to(dtype)
    r = q[..., 3] - torch.floor(q[..., 3])
    h = ((r * 2) * PI32) / 2
    sh, ch = torch.sin(h), torch.cos(h)
    a, b, c, d = q[..., 0] * sh, q[..., 1] * sh, q[..., 2] * sh, ch
    l = torch.sqrt(a * a + b * b + c * c + d * d)
    x, y, z, w = a / l, b / l, c / l, d / l
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    rows = [torch.stack([x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw)], -1),
            torch.stack([2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw)], -1),
            torch.stack([2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2], -1)]
    return torch.stack(rows, -2)


def prim_m(params, kinds, queries, dtype=torch.float64):
    """m [B,Q,K]: x~ = R^T (x - t) / v, m = x~.x~ (sphere) or max |x~_i| (cuboid), a NaN where any x~_i is one."""
    B = params.shape[0]
    p, x = params.to(dtype), _per_sample(queries, B).to(dtype)
    v, t, R = p[:, :, 0:3], p[:, :, 7:10], rotations(p[:, :, 3:7], dtype)
    d = x[:, :, None, :] - t[:, None, :, :]                                      # [B,Q,K,3]
    y = torch.stack([R[:, None, :, 0, i] * d[..., 0] + R[:, None, :, 1, i] * d[..., 1] + R[:, None, :, 2, i] * d[..., 2]
                     for i in range(3)], -1) / v[:, None]
    sphere = y[..., 0] * y[..., 0] + y[..., 1] * y[..., 1] + y[..., 2] * y[..., 2]
    cuboid = y.abs().max(-1).values
    cuboid = torch.where(torch.isnan(y).any(-1), torch.full_like(cuboid, math.nan), cuboid)
    is_sphere = torch.tensor([k == SPHERE for k in kinds])
    return torch.where(is_sphere[None, None, :], sphere, cuboid)


def prim_occupancy(params, kinds, queries, dtype=torch.float64):
    """(occ uint8 [B,Q], owner int32 [B,Q]): inside iff m <= 1 (a NaN is outside); the lowest k that holds the point, -1."""
    inside = prim_m(params, kinds, queries, dtype) <= 1
    K = inside.shape[-1]
    owner = torch.where(inside, torch.arange(K)[None, None, :], K).min(-1).values
    owner = torch.where(owner == K, -1, owner).to(torch.int32)
    return (owner >= 0).to(torch.uint8), owner


def prim_plain(prm, kind, x):
    """m of ONE primitive (10 Python floats) at ONE point, in plain Python."""
    v, q, t = prm[0:3], prm[3:7], prm[7:10]
    h = (((q[3] - math.floor(q[3])) * 2) * PI32) / 2
    r = [q[0] * math.sin(h), q[1] * math.sin(h), q[2] * math.sin(h), math.cos(h)]
    l = math.sqrt(sum(c * c for c in r))
    qx, qy, qz, qw = (c / l for c in r)
    R = [[qx * qx - qy * qy - qz * qz + qw * qw, 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
         [2 * (qx * qy + qz * qw), -qx * qx + qy * qy - qz * qz + qw * qw, 2 * (qy * qz - qx * qw)],
         [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), -qx * qx - qy * qy + qz * qz + qw * qw]]
    d = [x[k] - t[k] for k in range(3)]
    y = [(R[0][i] * d[0] + R[1][i] * d[1] + R[2][i] * d[2]) / v[i] for i in range(3)]
    return sum(c * c for c in y) if kind == SPHERE else max(abs(c) for c in y)


# ---- the winding number

def _map(corners, xf):
    """corners [B,F,3], xf [B,3,4]: m0 x + m1 y + m2 z + m3 per row."""
    return (xf[:, None, :, 0] * corners[..., 0:1] + xf[:, None, :, 1] * corners[..., 1:2] + xf[:, None, :, 2] * corners[..., 2:3]
            + xf[:, None, :, 3])


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def winding(verts, faces, queries, xforms=None, dtype=torch.float64):
    """w [B,Q] of the batched layout: verts [B,P,3], faces [F,3], queries [Q,3] or [B,Q,3], xforms [B,3,4] or None.  A face
    with a vertex index outside [0,P) or with (v1 - v0) x (v2 - v0) = (0,0,0) adds nothing; num == 0 adds exactly 0; a query that is not finite, or a live face with
    a corner that is not finite, gives NaN."""
    B, P = verts.shape[0], verts.shape[1]
    v, f, x = verts.to(dtype), faces.long(), _per_sample(queries, B).to(dtype)
    live = ((f >= 0) & (f < P)).all(-1)                                          # [F]
    fc = f.clamp(0, P - 1)
    corners = [v[:, fc[:, k]] for k in range(3)]                                 # each [B,F,3]
    if xforms is not None:
        corners = [_map(c, xforms.to(dtype)) for c in corners]
    e1, e2 = corners[1] - corners[0], corners[2] - corners[0]
    area = torch.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                        e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], -1)
    live = live[None, :] & ~(area == 0).all(-1)                                  # [B,F]: e1 x e2 = (0,0,0) is a face of no area
    a, b, c = (k[:, None, :, :] - x[:, :, None, :] for k in corners)            # [B,Q,F,3]
    la, lb, lc = torch.sqrt(_dot(a, a)), torch.sqrt(_dot(b, b)), torch.sqrt(_dot(c, c))
    n = torch.stack([b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1], b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2],
                     b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]], -1)
    num = _dot(a, n)
    den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
    term = torch.where(num == 0, torch.zeros_like(num), 2 * torch.atan2(num, den))
    term = torch.where(live[:, None, :], term, torch.zeros_like(term))
    w = term.sum(-1) / FOUR_PI
    bad_face = (~torch.isfinite(torch.stack(corners, -2)).all(-1).all(-1) & live).any(-1)                # [B]
    bad = bad_face[:, None] | ~torch.isfinite(x).all(-1)
    return torch.where(bad, torch.full_like(w, math.nan), w)


def ragged_winding(verts, faces, vert_offset, face_offset, queries, xforms=None, dtype=torch.float64):
    """w [S,Q] of the ragged layout, mesh by mesh through `winding`: sample b is mesh b."""
    S = vert_offset.numel() - 1
    x = _per_sample(queries, S)
    out = []
    for s in range(S):
        v0, v1, f0, f1 = int(vert_offset[s]), int(vert_offset[s + 1]), int(face_offset[s]), int(face_offset[s + 1])
        out.append(winding(verts[v0:v1][None], faces[f0:f1], x[s:s + 1], None if xforms is None else xforms[s:s + 1], dtype)[0])
    return torch.stack(out)


def winding_plain(verts, faces, x, xform=None):
    """w of ONE mesh (verts [P][3], faces [F][3]) at ONE point in Python floats."""
    total = 0.0
    for f in faces:
        if not all(0 <= i < len(verts) for i in f):
            continue
        c = [list(verts[i]) for i in f]
        if xform is not None:
            c = [[xform[r][0] * p[0] + xform[r][1] * p[1] + xform[r][2] * p[2] + xform[r][3] for r in range(3)] for p in c]
        e1, e2 = [c[1][k] - c[0][k] for k in range(3)], [c[2][k] - c[0][k] for k in range(3)]
        if e1[1] * e2[2] - e1[2] * e2[1] == 0 and e1[2] * e2[0] - e1[0] * e2[2] == 0 and e1[0] * e2[1] - e1[1] * e2[0] == 0:
            continue
        a, b, cc = ([p[k] - x[k] for k in range(3)] for p in c)
        dot = lambda u, v: u[0] * v[0] + u[1] * v[1] + u[2] * v[2]
        la, lb, lc = math.sqrt(dot(a, a)), math.sqrt(dot(b, b)), math.sqrt(dot(cc, cc))
        n = [b[1] * cc[2] - b[2] * cc[1], b[2] * cc[0] - b[0] * cc[2], b[0] * cc[1] - b[1] * cc[0]]
        num = dot(a, n)
        den = la * lb * lc + dot(a, b) * lc + dot(b, cc) * la + dot(cc, a) * lb
        total += 0.0 if num == 0 else 2 * math.atan2(num, den)
    return total / FOUR_PI


# ---- the IoU row and the bookkeeping

def iou_counts(occ_pred, occ_gt):
    """int64 [B,4] = (I, U, Np, Ng)."""
    p, g = occ_pred != 0, occ_gt != 0
    return torch.stack([(p & g).sum(1), (p | g).sum(1), p.sum(1), g.sum(1)], 1)


def iou_rows(occ_pred, occ_gt):
    """(rows fp32 [B,5], counts int64 [B,4]): each quotient formed in float64 from the integers and rounded once, 0 where its
    denominator is 0."""
    counts = iou_counts(occ_pred, occ_gt)
    Q = occ_pred.shape[1]
    c = counts.double()
    num = torch.stack([c[:, 0], c[:, 0], c[:, 0], c[:, 2], c[:, 3]], 1)
    den = torch.stack([c[:, 1], c[:, 2], c[:, 3], torch.full_like(c[:, 0], Q), torch.full_like(c[:, 0], Q)], 1)
    rows = torch.where(den > 0, num / den.clamp_min(1), torch.zeros_like(num))
    return rows.float(), counts


def bookkeeping(batches, C):
    """The state after `batches` = [(rows [B,5] on the host, counts [B,4], class indices)] as a plain loop in Python floats,
    in sample order: (sums: (1 + C) W floats -- total[W], class_sum[C][W] --, counts: [n_samples, n_batches, n_empty,
    n_invalid] + class_n[C])."""
    sums, counts = [0.0] * ((1 + C) * W), [0] * (4 + C)
    for rows, cnt, idx in batches:
        assert rows.shape[1] == W
        for b in range(rows.shape[0]):
            c = int(idx[b])
            for k in range(W):
                x = float(rows[b, k])
                sums[k] += x
                if 0 <= c < C:
                    sums[(1 + c) * W + k] += x
            if 0 <= c < C:
                counts[4 + c] += 1
            else:
                counts[3] += 1
            counts[2] += int(cnt[b, 1]) == 0
        counts[0] += rows.shape[0]
        counts[1] += 1
    return sums, counts


def state_tensor(sums, counts):
    return torch.cat([torch.tensor(sums, dtype=torch.float64), torch.tensor(counts, dtype=torch.int64).view(torch.float64)])


# ---- shared meshes

BOX_FACES = [[0, 2, 3], [0, 3, 1], [0, 1, 5], [0, 5, 4], [2, 7, 3], [2, 6, 7], [0, 4, 6], [0, 6, 2], [1, 7, 5], [1, 3, 7],
             [4, 7, 6], [4, 5, 7]]               # outward; the last two are the top (z+)


def box(centre=(0.0, 0.0, 0.0), half=(0.25, 0.25, 0.25)):
    """(verts float64 [8,3], faces int64 [12,3]) of an axis-aligned box, faces outward, vertex 4 z + 2 y + x."""
    v = [[centre[0] + (2 * (i & 1) - 1) * half[0], centre[1] + (2 * ((i >> 1) & 1) - 1) * half[1],
          centre[2] + (2 * ((i >> 2) & 1) - 1) * half[2]] for i in range(8)]
    return torch.tensor(v, dtype=torch.float64), torch.tensor(BOX_FACES, dtype=torch.int64)


def two_boxes():
    """Half-extent-0.25 boxes at x = 0 and x = 0.25 as ONE mesh of 16 vertices and 24 faces: w = 2 in the overlap."""
    (va, fa), (vb, fb) = box(), box((0.25, 0.0, 0.0))
    return torch.cat([va, vb]), torch.cat([fa, fb + 8])


def two_box_params():
    """params [1,2,10] of the same two boxes as cuboids: identity rotation (q3 = 0)."""
    return torch.tensor([[[0.25, 0.25, 0.25, 0, 0, 1, 0, 0, 0, 0], [0.25, 0.25, 0.25, 0, 0, 1, 0, 0.25, 0, 0]]], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def ellipsoids(level, B, seed=0):
    """fp32 [B,V,3]: the icosphere as an ellipsoid per sample (semi-axes 0.25 .. 0.4: volume >= 0.065; centre within 0.1 of
    the origin) with a displacement of 2 % of an edge per vertex."""
    v, _ = SR.icosphere(level)
    g = torch.Generator().manual_seed(57 * level + B + 1000 * seed)
    axes = 0.25 + 0.15 * torch.rand(B, 1, 3, generator=g, dtype=torch.float64)
    centre = 0.2 * torch.rand(B, 1, 3, generator=g, dtype=torch.float64) - 0.1
    edge = 0.25 * {1: 0.55, 2: 0.28, 3: 0.14}[level]
    return (v[None] * axes + centre + 0.02 * edge * torch.randn(B, v.shape[0], 3, generator=g, dtype=torch.float64)).float().contiguous()


# ---- queries by rejection: the first Q candidates that pass are kept, so no case is left out afterwards

MIN_DISTANCE, MIN_W_MARGIN, MIN_M_MARGIN = 1e-3, 0.05, 1e-4


def mesh_margins(x, verts, faces, xforms=None):
    """(float64 distance to the nearest triangle [B,n], |w64 - 0.5| [B,n]) of fp32 candidates x [B,n,3]."""
    v = verts.double()
    if xforms is not None:
        v = _map(v, xforms.double())
    d = PM.pair_table(x.double(), v, faces).min(2).values.sqrt()
    return d, (winding(verts, faces, x, xforms) - 0.5).abs()


def draw_queries(seed, Q, ok, span=0.6, shape=()):
    """fp32 [*shape,Q,3] uniform in [-span, span]^3: per leading index the first Q candidates for which ok(x [*shape,n,3]) ->
    bool [*shape,n] holds."""
    g = torch.Generator().manual_seed(seed)
    kept = None
    while True:
        x = ((torch.rand(*shape, 4 * Q + 64, 3, generator=g, dtype=torch.float64) * 2 - 1) * span).float()
        good = ok(x)
        flat_x, flat_g = x.reshape(-1, x.shape[-2], 3), good.reshape(-1, x.shape[-2])
        rows = [flat_x[i][flat_g[i]] for i in range(flat_x.shape[0])]
        kept = rows if kept is None else [torch.cat([k, r]) for k, r in zip(kept, rows)]
        if min(k.shape[0] for k in kept) >= Q:
            return torch.stack([k[:Q] for k in kept]).reshape(*shape, Q, 3).contiguous()


def _mesh_ok(verts, faces, xforms=None, shared=False):
    def ok(x):
        xb = x[None].expand(verts.shape[0], -1, -1) if shared else x
        d, m = mesh_margins(xb, verts, faces, xforms)
        good = (d >= MIN_DISTANCE) & (m >= MIN_W_MARGIN)
        return good.all(0) if shared else good
    return ok


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    """The batched-layout cases of the GPU test: dict(verts fp32 [B,P,3], faces int64 [F,3], queries fp32 ([Q,3] shared or
    [B,Q,3]), xforms)."""
    if name == 'cube':                                     # F = 12, B = 1, Q = 1
        v, f = box()
        verts = v.float()[None].contiguous()
        return dict(verts=verts, faces=f, queries=draw_queries(1, 1, _mesh_ok(verts, f), shape=(1,)), xforms=None)
    if name == 'ico2':                                     # F = 320, B = 3, Q = 257, ONE query set for the batch
        verts, f = ellipsoids(2, 3), SR.icosphere(2)[1]
        return dict(verts=verts, faces=f, queries=draw_queries(2, 257, _mesh_ok(verts, f, shared=True), span=0.45), xforms=None)
    if name == 'ico3':                                     # F = 1280, B = 1, Q = 257
        verts, f = ellipsoids(3, 1), SR.icosphere(3)[1]
        return dict(verts=verts, faces=f, queries=draw_queries(3, 257, _mesh_ok(verts, f), span=0.45, shape=(1,)), xforms=None)
    raise KeyError(name)


def ragged_meshes():
    """[(verts float64, faces)]: the cube, the icosphere of level 1 and of level 3 as spheres of radius 0.35 and 0.3."""
    return [box(), (SR.icosphere(1)[0] * 0.35, SR.icosphere(1)[1]), (SR.icosphere(3)[0] * 0.3 + 0.05, SR.icosphere(3)[1])]


@functools.lru_cache(maxsize=None)
def ragged_case():
    """dict(meshes, verts fp32 [sumP,3], faces [sumF,3], vert_offset, face_offset, xforms fp32 [3,3,4] (view_center_xforms),
    queries fp32 [3,300,3])."""
    from vpn_amd.modules.dataset import view_center_xforms
    meshes = ragged_meshes()
    xf = view_center_xforms([1.0, 1.2, 1.1], [25.0, 10.0, 40.0], [140.0, 30.0, 300.0]).contiguous()
    vo, fo = [0], [0]
    for v, f in meshes:
        vo.append(vo[-1] + v.shape[0])
        fo.append(fo[-1] + f.shape[0])
    verts, faces = torch.cat([v for v, _ in meshes]).float(), torch.cat([f for _, f in meshes])

    def ok(x):
        out = []
        for s, (v, f) in enumerate(meshes):
            d, m = mesh_margins(x[s:s + 1], v.float()[None], f, xf[s:s + 1])
            out.append(((d >= MIN_DISTANCE) & (m >= MIN_W_MARGIN))[0])
        return torch.stack(out)

    return dict(meshes=meshes, verts=verts, faces=faces, vert_offset=torch.tensor(vo, dtype=torch.int32),
                face_offset=torch.tensor(fo, dtype=torch.int32), xforms=xf, queries=draw_queries(4, 300, ok, shape=(3,)))


@functools.lru_cache(maxsize=None)
def prim_case():
    """K = 3 (cuboid, sphere, sphere), B = 3, poses from pose_domain_ref.pose_params, extents of at least 0.15; queries: the 8^3
    grid plus 257 drawn ones, shared by the batch, every |m64 - 1| >= 1e-4."""
    import pose_domain_ref as PD
    g = torch.Generator().manual_seed(5)
    params = PD.pose_params(g, K=3)[[3, 77, 140]].clone()
    params[:, :, 0:3] = 0.15 + 0.2 * torch.rand(3, 3, 3, generator=g)
    params = params.float().contiguous()
    kinds = (CUBOID, SPHERE, SPHERE)
    ok = lambda x: ((prim_m(params, kinds, x) - 1).abs() >= MIN_M_MARGIN).all(-1).all(0)
    grid = grid_queries(8)
    assert bool(ok(grid).all()), 'a grid centre lies within 1e-4 of a primitive boundary'
    queries = torch.cat([grid, draw_queries(6, 257, ok)]).contiguous()
    return dict(params=params, kinds=kinds, queries=queries)
