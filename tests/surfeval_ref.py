"""Restatement of the surface evaluation (csrc/surfeval.hip) in torch, in a chosen dtype, and the inputs its
tests share: unit normals of the faces sampled points lie on (both layouts, with and without affine maps), the per-sample row
from (dist, idx, normals, thr2), the bookkeeping as a plain Python loop; icospheres, point clouds, a float64 brute-force
nearest-neighbour scan and thresholds placed in gaps of its distances."""
import functools
import math

import torch

MAX_T = 8


def width(T):
    return 6 + 3 * T


# ---- normals

def _map(corners, xf):
    """corners [..., 3 (corner), 3], xf [..., 3, 4] broadcast over the leading dims: R c + t."""
    return (xf[..., None, :, :3] * corners[..., None, :]).sum(-1) + xf[..., None, :, 3]


def _unit(corners):
    e1, e2 = corners[..., 1, :] - corners[..., 0, :], corners[..., 2, :] - corners[..., 0, :]
    c = torch.cross(e1, e2, dim=-1)
    cc = (c * c).sum(-1, keepdim=True)
    ok = (cc > 0) & torch.isfinite(cc)
    return torch.where(ok, c / torch.sqrt(torch.where(ok, cc, torch.ones_like(cc))), torch.zeros_like(c))


def face_normals(verts, faces, fidx, xforms=None, dtype=torch.float64):
    """The batched layout: verts [B,P,3], faces [F,3], fidx [B,n] -> [B,n,3] in `dtype`; (0,0,0) for a face index outside
    [0,F), a vertex index outside [0,P) and a face without area."""
    B, P, F = verts.shape[0], verts.shape[1], faces.shape[0]
    v, f, fi = verts.to(dtype), faces.long(), fidx.long()
    f_ok = (fi >= 0) & (fi < F)
    tri = f[fi.clamp(0, F - 1)]                                             # [B,n,3]
    v_ok = ((tri >= 0) & (tri < P)).all(-1)
    corners = v[torch.arange(B)[:, None, None], tri.clamp(0, P - 1)]          # [B,n,3 (corner),3]
    if xforms is not None:
        corners = _map(corners, xforms.to(dtype)[:, None])
    return torch.where((f_ok & v_ok)[..., None], _unit(corners), torch.zeros((), dtype=dtype))


def ragged_normals(verts, faces, vert_offset, face_offset, fidx, sets=1, xforms=None, dtype=torch.float64):
    """The ragged layout: verts [sumP,3], mesh-local faces [sumF,3], offsets [S+1], fidx [S,sets,n] mesh-local, xforms
    [S,sets,3,4] -> [S,sets,n,3].  Mesh by mesh through face_normals."""
    S = vert_offset.numel() - 1
    out = []
    for s in range(S):
        v0, v1, f0, f1 = int(vert_offset[s]), int(vert_offset[s + 1]), int(face_offset[s]), int(face_offset[s + 1])
        v = verts[v0:v1][None].expand(sets, -1, -1)
        out.append(face_normals(v, faces[f0:f1], fidx[s], None if xforms is None else xforms[s], dtype))
    return torch.stack(out)


def normals_plain(verts, faces, fidx, xform=None):
    """One sample in Python floats: verts [P][3], faces [F][3], fidx [n], xform [3][4] or None -> [n][3]."""
    out = []
    for f in fidx:
        n = [0.0, 0.0, 0.0]
        if 0 <= f < len(faces) and all(0 <= i < len(verts) for i in faces[f]):
            c = [list(verts[i]) for i in faces[f]]
            if xform is not None:
                c = [[sum(xform[r][k] * p[k] for k in range(3)) + xform[r][3] for r in range(3)] for p in c]
            e1, e2 = [c[1][k] - c[0][k] for k in range(3)], [c[2][k] - c[0][k] for k in range(3)]
            x = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            cc = x[0] * x[0] + x[1] * x[1] + x[2] * x[2]
            if cc > 0 and math.isfinite(cc):
                n = [t / math.sqrt(cc) for t in x]
        out.append(n)
    return out


# ---- the per-sample row

def sample_rows(d1, i1, d2, i2, thr2, n_pred=None, n_gt=None, dtype=torch.float64):
    """(rows [B, 6 + 3 T] in `dtype`, counts int64 [B,2,T]) from the distances d1 [B,N] / d2 [B,M] as the nearest-neighbour
    scan writes them -- Euclidean, NOT squared --, neighbour indices (clamped into range) and SQUARED thresholds thr2 [T].
    The square is formed in float64 (exact for fp32 inputs) and the threshold test is made on it; everything else in
    `dtype`."""
    B, N, M, T = d1.shape[0], d1.shape[1], d2.shape[1], thr2.numel()
    rows = torch.zeros((B, width(T)), dtype=dtype)
    q1, q2 = d1.double() * d1.double(), d2.double() * d2.double()
    rows[:, 0], rows[:, 1] = q1.to(dtype).mean(1), q2.to(dtype).mean(1)
    rows[:, 2], rows[:, 3] = d1.to(dtype).mean(1), d2.to(dtype).mean(1)
    if n_pred is not None:
        a, b = n_pred.to(dtype), n_gt.to(dtype)
        j1 = i1.long().clamp(0, M - 1)[..., None].expand(-1, -1, 3)
        j2 = i2.long().clamp(0, N - 1)[..., None].expand(-1, -1, 3)
        rows[:, 4] = (a * torch.gather(b, 1, j1)).sum(-1).abs().mean(1)
        rows[:, 5] = (b * torch.gather(a, 1, j2)).sum(-1).abs().mean(1)
    counts = torch.stack([(q1[:, :, None] < thr2[None, None, :].double()).sum(1),
                          (q2[:, :, None] < thr2[None, None, :].double()).sum(1)], 1)
    p, r = counts[:, 0].to(dtype) / N, counts[:, 1].to(dtype) / M
    rows[:, 6:6 + T], rows[:, 6 + T:6 + 2 * T] = p, r
    rows[:, 6 + 2 * T:] = torch.where(p + r > 0, 2 * p * r / (p + r).clamp_min(1e-300), torch.zeros_like(p))
    return rows, counts


def rows_plain(d1, i1, d2, i2, thr2, n_pred=None, n_gt=None):
    """One sample in Python floats and loops: lists in (d1, d2: distances, NOT squared; thr2: squared), the row as a list out."""
    T, N, M = len(thr2), len(d1), len(d2)
    row = [sum(x * x for x in d1) / N, sum(x * x for x in d2) / M, sum(d1) / N, sum(d2) / M, 0.0, 0.0]
    if n_pred is not None:
        dot = lambda a, b: abs(a[0] * b[0] + a[1] * b[1] + a[2] * b[2])
        row[4] = sum(dot(n_pred[i], n_gt[min(max(i1[i], 0), M - 1)]) for i in range(N)) / N
        row[5] = sum(dot(n_gt[j], n_pred[min(max(i2[j], 0), N - 1)]) for j in range(M)) / M
    p = [sum(1 for x in d1 if x * x < t) / N for t in thr2]
    r = [sum(1 for x in d2 if x * x < t) / M for t in thr2]
    return row + p + r + [2 * a * b / (a + b) if a + b > 0 else 0.0 for a, b in zip(p, r)]


# ---- the bookkeeping

def bookkeeping(batches, C, T):
    """The state after `batches` = [(rows [B,W] on the host, class indices)] as a plain loop in Python floats, in sample
    order: (sums: list of (1 + C) W floats -- total[W], class_sum[C][W] --, counts: [n_samples, n_batches, n_invalid] +
    class_n[C])."""
    W = width(T)
    sums, counts = [0.0] * ((1 + C) * W), [0] * (3 + C)
    for rows, idx in batches:
        assert rows.shape[1] == W
        for b in range(rows.shape[0]):
            c = int(idx[b])
            for k in range(W):
                x = float(rows[b, k])
                sums[k] += x
                if 0 <= c < C:
                    sums[(1 + c) * W + k] += x
            if 0 <= c < C:
                counts[3 + c] += 1
            else:
                counts[2] += 1
        counts[0] += rows.shape[0]
        counts[1] += 1
    return sums, counts


def state_tensor(sums, counts):
    return torch.cat([torch.tensor(sums, dtype=torch.float64), torch.tensor(counts, dtype=torch.int64).view(torch.float64)])


# ---- shared inputs

@functools.lru_cache(maxsize=None)
def icosphere(level):
    """(unit vertices float64 [V,3], faces int64 [F,3]) of an icosahedron subdivided `level` times: level 1 has 42 vertices
    and 80 faces, level 2 162 and 320.  Every face is close to equilateral."""
    t = (1 + math.sqrt(5)) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
         [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [[x / math.sqrt(1 + t * t) for x in p] for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = [(v[a][k] + v[b][k]) / 2 for k in range(3)]
                l = math.sqrt(sum(x * x for x in m))
                v.append([x / l for x in m])
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return torch.tensor(v, dtype=torch.float64), torch.tensor(f, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def mesh_vertices(level, B, seed=0):
    """fp32 [B,V,3]: the icosphere as an ellipsoid per sample (semi-axes 0.2 .. 0.4, centre within 0.1 of the origin) with a
    displacement of 2 % of an edge per vertex, so no two samples and no two faces are alike."""
    v, _ = icosphere(level)
    g = torch.Generator().manual_seed(31 * level + B + 1000 * seed)
    axes = 0.2 + 0.2 * torch.rand(B, 1, 3, generator=g, dtype=torch.float64)
    centre = 0.2 * torch.rand(B, 1, 3, generator=g, dtype=torch.float64) - 0.1
    edge = 0.2 * (0.55 if level == 1 else 0.28)
    return (v[None] * axes + centre + 0.02 * edge * torch.randn(B, v.shape[0], 3, generator=g, dtype=torch.float64)).float().contiguous()


def face_shape(verts, faces):
    """(the smallest sin of an angle, the shortest edge) over all faces of verts [B,V,3] in float64."""
    c = verts.double()[:, faces.long()]                                     # [B,F,3,3]
    worst_sin, worst_edge = 1.0, float('inf')
    for k in range(3):
        a, b = c[:, :, (k + 1) % 3] - c[:, :, k], c[:, :, (k + 2) % 3] - c[:, :, k]
        la, lb = a.norm(dim=-1), b.norm(dim=-1)
        worst_sin = min(worst_sin, float((torch.cross(a, b, dim=-1).norm(dim=-1) / (la * lb)).min()))
        worst_edge = min(worst_edge, float(la.min()))
    return worst_sin, worst_edge


@functools.lru_cache(maxsize=None)
def clouds(kind, B=3, N=257, M=300):
    """(prediction [B,N,3], ground truth [B,M,3]) fp32 in [-0.5, 0.5]^3: 'uniform', or 'clustered' around eight shared blobs."""
    g = torch.Generator().manual_seed({'uniform': 7, 'clustered': 8}[kind] + 100 * N + M)
    if kind == 'uniform':
        return torch.rand(B, N, 3, generator=g) - 0.5, torch.rand(B, M, 3, generator=g) - 0.5
    centres = torch.rand(B, 8, 3, generator=g) * 0.6 - 0.3
    out = []
    for n in (N, M):
        which = torch.randint(0, 8, (B, n), generator=g)
        pts = torch.gather(centres, 1, which[..., None].expand(-1, -1, 3)) + 0.05 * torch.randn(B, n, 3, generator=g)
        out.append(pts.clamp(-0.5, 0.5).contiguous())
    return tuple(out)


def brute_nn(p, q):
    """Float64 brute force over fp32 clouds: (d1 [B,N], i1, d2 [B,M], i2), SQUARED distances (the scan's are their roots)."""
    d = ((p.double()[:, :, None, :] - q.double()[:, None, :, :]) ** 2).sum(-1)
    d1, i1 = d.min(2)
    d2, i2 = d.min(1)
    return d1, i1, d2, i2


@functools.lru_cache(maxsize=None)
def gap_thresholds(kind):
    """Three distance thresholds for clouds(kind), each the midpoint of the widest gap among the 33 sorted float64
    nearest-neighbour distances (both directions, all samples) around the 30 %, 60 % and 90 % quantile."""
    d1, _, d2, _ = brute_nn(*clouds(kind))
    d = torch.sort(torch.sqrt(torch.cat([d1.flatten(), d2.flatten()])))[0]
    taus = []
    for q in (0.3, 0.6, 0.9):
        at = int(q * d.numel())
        w = d[at - 16:at + 17]
        k = int(torch.argmax(w[1:] - w[:-1]))
        taus.append(float((w[k] + w[k + 1]) / 2))
    return tuple(taus)


def thr2_of(taus):
    """float32(tau * tau), the product formed in float64: what the meter uploads."""
    return torch.tensor([t * t for t in taus], dtype=torch.float64).to(torch.float32)
