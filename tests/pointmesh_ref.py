"""The point-to-surface distance (vpn_amd.point_mesh_distance, csrc/pointmesh.hip) stated in plain torch, in a
chosen dtype (float64 is the specification).  Shared by tests/test_pointmesh_cpu.py and tests/test_pointmesh.py, with the
inputs both use; the meshes and vertices() are those of tests/meshreg_ref.py.

points [B,P,3], verts [B,V,3], one face list [F,3] for the batch.

  d(p, T)    min over the simplex w of |p - (w0 v0 + w1 v1 + w2 v2)|^2, the squared distance to the closed triangle, formed
             from p - c.  Per pair: the plane candidate (the foot of the perpendicular, when the triangle has area and the foot
             lies in it) and the three segment candidates v0..v1, v1..v2, v0..v2 (a segment of length 0 is its start point);
             the least, the first on ties.  A triangle without area is the segment or point it degenerates to.
  region     of the closest point: 0 face, 1 + j on edge j (strictly inside segment j), 4 + k at corner k.
  dist_p     min over the faces, face_of_point the lowest face that gives it; dist_f, point_of_face likewise over the points.
  out        (mean of dist_p over (b, i), mean of dist_f over (b, f)).
  gradient   at given index tensors: d d / d p = 2 (p - c), d d / d v_k = -2 w_k (p - c) of every (point, face) record.
"""
import functools
import math

import torch

import meshreg_ref as M

FACE, EDGE0, EDGE1, EDGE2, CORNER0, CORNER1, CORNER2 = range(7)
REGIONS = ('face', 'edge 0', 'edge 1', 'edge 2', 'corner 0', 'corner 1', 'corner 2')
SEGMENTS = ((0, 1), (1, 2), (0, 2))               # segment j runs from corner a to corner b with parameter u


def closest(p, v0, v1, v2):
    """(d [...], w [...,3], region [...]) of points p [...,3] against triangles (v0, v1, v2) [...,3], broadcast, in p's dtype."""
    dt = p.dtype
    corners = (v0, v1, v2)
    e1, e2, d = v1 - v0, v2 - v0, p - v0
    a, b, c = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    d1, d2 = (e1 * d).sum(-1), (e2 * d).sum(-1)
    det = a * c - b * b
    safe = torch.where(det > 0, det, torch.ones_like(det))
    s, t = (c * d1 - b * d2) / safe, (a * d2 - b * d1) / safe
    inside = (det > 0) & (s >= 0) & (t >= 0) & (s + t <= 1)
    inf = torch.full_like(det, math.inf)
    cand_w = [torch.stack([1 - s - t, s, t], -1)]
    cand_region = [torch.zeros_like(det, dtype=torch.long)]
    live = [inside]
    for j, (ia, ib) in enumerate(SEGMENTS):
        ab, ap = corners[ib] - corners[ia], p - corners[ia]
        l = (ab * ab).sum(-1)
        u = torch.where(l > 0, (ab * ap).sum(-1) / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(l)).clamp(0, 1)
        w = [torch.zeros_like(u)] * 3
        w[ia], w[ib] = 1 - u, u
        cand_w.append(torch.stack(torch.broadcast_tensors(*w), -1))
        cand_region.append(torch.where(u <= 0, CORNER0 + ia, torch.where(u >= 1, CORNER0 + ib, EDGE0 + j)))
        live.append(torch.ones_like(inside))
    cand_d = []
    for w, ok in zip(cand_w, live):
        r = d - w[..., 1:2] * e1 - w[..., 2:3] * e2                         # p - c
        cand_d.append(torch.where(ok, (r * r).sum(-1), inf))
    cand_d = torch.stack(cand_d)                                             # [4,...]: argmin takes the first of equal values
    pick = torch.argmin(cand_d, 0, keepdim=True)
    dist = torch.gather(cand_d, 0, pick)[0]
    w = torch.gather(torch.stack(cand_w), 0, pick[..., None].expand(1, *cand_w[0].shape))[0]
    region = torch.gather(torch.stack(torch.broadcast_tensors(*cand_region)), 0, pick)[0]
    return dist.to(dt), w, region


def _corners(verts, faces):
    f = faces.long()
    return verts[:, f[:, 0]], verts[:, f[:, 1]], verts[:, f[:, 2]]          # each [B,F,3]


def pair_table(points, verts, faces):
    """d [B,P,F] of every pair, in points' dtype."""
    v0, v1, v2 = _corners(verts, faces)
    return closest(points[:, :, None], v0[:, None], v1[:, None], v2[:, None])[0]


def nearest(points, verts, faces, dtype=torch.float64):
    """(dist_p [B,P], face_of_point, dist_f [B,F], point_of_face, table [B,P,F]) of the restatement in `dtype`: the lowest index
    among equal values."""
    table = pair_table(points.to(dtype), verts.to(dtype), faces)
    dist_p, fop = table.min(2)
    dist_f, pof = table.min(1)
    # torch.min with a dim makes no promise about ties: the lowest index holding the minimum, stated outright
    F, P = table.shape[2], table.shape[1]
    fop = torch.where(table == dist_p[:, :, None], torch.arange(F)[None, None], F).min(2).values
    pof = torch.where(table == dist_f[:, None, :], torch.arange(P)[None, :, None], P).min(1).values
    return dist_p, fop, dist_f, pof, table


def records(points, verts, faces, fop, pof):
    """The (point, face) records of both directions at the given indices: (d, w, region, p - c) of the points against their
    faces [B,P,...] and of the faces against their points [B,F,...], in points' dtype."""
    v0, v1, v2 = _corners(verts, faces)
    out = []
    for pts, tri in ((points, [torch.gather(v, 1, fop.long()[..., None].expand(-1, -1, 3)) for v in (v0, v1, v2)]),
                     (torch.gather(points, 1, pof.long()[..., None].expand(-1, -1, 3)), [v0, v1, v2])):
        d, w, region = closest(pts, *tri)
        r = pts - (w[..., 0:1] * tri[0] + w[..., 1:2] * tri[1] + w[..., 2:3] * tri[2])
        out.append((d, w, region, r))
    return out


def gradient(points, verts, faces, fop, pof, upstream=(1.0, 1.0), dtype=torch.float64):
    """(dpoints [B,P,3], dverts [B,V,3]) of upstream . out in `dtype`, at the minimisers the index tensors name."""
    points, verts = points.to(dtype), verts.to(dtype)
    B, P, _ = points.shape
    F = faces.shape[0]
    f = faces.long()
    (_, wp, _, rp), (_, wf, _, rf) = records(points, verts, faces, fop, pof)
    cp, cf = 2.0 * upstream[0] / (B * P), 2.0 * upstream[1] / (B * F)
    dpoints = cp * rp
    dpoints = dpoints.scatter_add(1, pof.long()[..., None].expand(-1, -1, 3), cf * rf)
    dverts = torch.zeros_like(verts)
    for k in range(3):
        dverts = dverts.scatter_add(1, f[fop.long(), k][..., None].expand(-1, -1, 3), -cp * wp[..., k:k + 1] * rp)
        dverts = dverts.scatter_add(1, f[:, k][None, :, None].expand(B, -1, 3), -cf * wf[..., k:k + 1] * rf)
    return dpoints, dverts


# ---- inputs

@functools.lru_cache(maxsize=None)
def cloud(name, B, P):
    """fp32 [B,P,3] near the surface of M.vertices(name, B): barycentric samples on random faces, pushed off by 0.05 randn."""
    faces, _ = M.mesh(name)
    verts = M.vertices(name, B)
    gen = torch.Generator().manual_seed(7919 * B + 31 * P + sum(map(ord, name)))
    pick = torch.randint(0, faces.shape[0], (B, P), generator=gen)
    w = torch.rand(B, P, 2, generator=gen)
    w = torch.where(w.sum(-1, keepdim=True) > 1, 1 - w, w)
    w = torch.cat([w, 1 - w.sum(-1, keepdim=True)], -1)
    corners = torch.stack([torch.gather(verts, 1, faces[pick][..., k, None].expand(-1, -1, 3)) for k in range(3)], 2)   # [B,P,3,3]
    return ((w[..., None] * corners).sum(2) + 0.05 * torch.randn(B, P, 3, generator=gen)).float().contiguous()


# (mesh, B, P): the smallest shapes that cross a wave, a point tile, a face slice and the composed mesh's face count
CASES = [('tetrahedron', 1, 1), ('tetrahedron', 1, 65), ('strip_65', 1, 63), ('irregular', 1, 64), ('fan_70', 1, 65), ('uv_sphere', 3, 257),
         ('two_components', 1, 64), ('composed', 1, 300)]
UPSTREAM = (0.3, -2.0)


def case_inputs(name, B, P):
    return cloud(name, B, P), M.vertices(name, B), M.mesh(name)[0]


@functools.lru_cache(maxsize=None)
def reference64(name, B, P):
    """(dist_p, face_of_point, dist_f, point_of_face, table, out [2]) in float64."""
    dist_p, fop, dist_f, pof, table = nearest(*case_inputs(name, B, P))
    return dist_p, fop, dist_f, pof, table, torch.stack([dist_p.mean(), dist_f.mean()])


@functools.lru_cache(maxsize=None)
def reference32(name, B, P):
    dist_p, fop, dist_f, pof, table = nearest(*case_inputs(name, B, P), dtype=torch.float32)
    return dist_p, fop, dist_f, pof, table, torch.stack([dist_p.mean(), dist_f.mean()])


def index_excess(table64, dist64, index, dim):
    """For every query the float64 distance of the pair `index` names over the float64 minimum, as a fraction of the largest
    minimum of the sample: [B,Q].  dim = 2: index is face_of_point [B,P]; dim = 1: point_of_face [B,F]."""
    chosen = torch.gather(table64, dim, index.long().unsqueeze(dim)).squeeze(dim)
    return (chosen - dist64) / dist64.max(1, keepdim=True).values.clamp_min(1e-300)


def one_triangle():
    """(points [N,1,3], verts [N,3,3], faces [1,3], regions [N]): N samples of ONE point against ONE scalene triangle, several
    in each of the seven regions, above and below the triangle's plane, so that every value and gradient is that of one pair."""
    v = torch.tensor([[0.1, -0.2, 0.05], [0.9, 0.1, 0.3], [0.3, 0.6, -0.1]], dtype=torch.float64)
    n = torch.linalg.cross(v[1] - v[0], v[2] - v[0])
    n = n / n.norm()
    pts, regions = [], []
    for h in (0.2, -0.35, 0.0125):
        for w in ((0.2, 0.3, 0.5), (0.6, 0.3, 0.1), (0.1, 0.1, 0.8)):                      # inside the face
            pts.append(sum(wk * vk for wk, vk in zip(w, v)) + h * n)
            regions.append(FACE)
        for j, (ia, ib) in enumerate(SEGMENTS):                                          # beyond edge j, beside its inside
            ab = v[ib] - v[ia]
            other = v[3 - ia - ib] - v[ia]
            out = -(other - ab * (other @ ab) / (ab @ ab))
            out = out / out.norm()
            for u in (0.25, 0.7):
                pts.append(v[ia] + u * ab + 0.3 * out + h * n)
                regions.append(EDGE0 + j)
        for k in range(3):                                                               # beyond corner k, in the wedge of its two edge normals
            away = (v[k] - v[(k + 1) % 3]) / (v[k] - v[(k + 1) % 3]).norm() + (v[k] - v[(k + 2) % 3]) / (v[k] - v[(k + 2) % 3]).norm()
            away = away / away.norm()
            for s in (0.1, 0.4):
                pts.append(v[k] + s * away + h * n)
                regions.append(CORNER0 + k)
    pts = torch.stack(pts).float()
    N = pts.shape[0]
    return pts[:, None].contiguous(), v.float()[None].repeat(N, 1, 1).contiguous(), torch.tensor([[0, 1, 2]]), torch.tensor(regions)
