"""numpy restatement of csrc/acdmix.hip (include/vpn_hip.h): float32 arithmetic rounded per operation,
dot(p, d) = (px dx + py dy) + pz dz.  numpy's float32 arrays round every operation by itself, which is the arithmetic the
kernels are built for (-ffp-contract=off); np.argmax returns the FIRST extreme element, which is the rule for equal
support values.  Also the inputs the tests share: boxes and ellipsoids as hulls along a set of directions, and points on their surfaces."""
import numpy as np

from reconstruct_ref import dot

F = np.float32
TURNS = (90.0, -90.0, 0.0, 180.0, -180.0)            # acd.py:59


def is_center(hull):
    """acd.py:31-34 on the D vertices [D,3] of one hull."""
    z = hull[:, 2]
    return bool(((z > 0).any() and (z < 0).any()) or np.abs(z).min() < F(0.05))


def turn_xy(x, y, turn):
    """The exact signed swap of rotate_points about (0,0,1): R = [[c,-s],[s,c]], angle TURNS[turn]."""
    if turn == 0:
        return -y, x
    if turn == 1:
        return y, -x
    if turn in (3, 4):
        return -x, -y
    return x, y


def hull_augment(verts, group, coin, u_num, scale, turn, shift, u_hull):
    """verts [S,G,D,3], group [G], per (sample, object) [S,O]: coin, u_num, scale, turn, shift; u_hull [S,G]
    -> out [S,G,D,3] float32, keep [S,G] int32."""
    verts = np.asarray(verts, F)
    group = np.asarray(group, np.int32)
    coin, turn = np.asarray(coin, np.int32), np.asarray(turn, np.int32)
    u_num, scale, shift, u_hull = (np.asarray(a, F) for a in (u_num, scale, shift, u_hull))
    S, G, D, _ = verts.shape
    O = coin.shape[1]
    out = np.empty_like(verts)
    keep = np.zeros((S, G), np.int32)
    for s in range(S):
        for o in range(O):
            members = [g for g in range(G) if group[g] == o]
            C = [g for g in members if is_center(verts[s, g])]
            if not C:
                kept = list(members)                                   # the deviation: nothing to choose from
            elif coin[s, o] != 0 and len(C) > 1:
                t = np.floor(u_num[s, o] * F(len(C) - 1))
                ncut = 1 + int(np.fmin(np.fmax(t, F(0)), F(len(C) - 2)))
                order = sorted(C, key=lambda g: (u_hull[s, g], g))      # smallest key first, equal keys: lowest index
                cut = set(order[:ncut])
                kept = [g for g in members if g not in cut]
            else:
                kept = list(C)
            for g in kept:
                keep[s, g] = 1
        for g in range(G):
            o = int(group[g])
            if not (0 <= o < O) or not keep[s, g]:
                out[s, g] = verts[s, g, 0]                             # collapsed onto its first vertex
                continue
            v = verts[s, g] * scale[s, o]
            x, y = turn_xy(v[:, 0], v[:, 1], int(turn[s, o]))
            out[s, g] = np.stack([x, y + shift[s, o], v[:, 2]], 1)
    return out, keep


def support_values(verts, dirs):
    """verts [S,G,D,3], dirs [D,3] -> [S,G,D] float32: the first of the largest dot(vert[h,j], dirs[d]) over j."""
    verts, dirs = np.asarray(verts, F), np.asarray(dirs, F)
    val = dot(verts[:, :, :, None, :], dirs[None, None, None, :, :])                  # [S,G,j,d]
    first = np.argmax(val, 2)
    return np.take_along_axis(val, first[:, :, None, :], 2)[:, :, 0, :]


def union_surface(verts, keep, dirs, cand, cand_hull, margin, n_out):
    """-> support [S,G,D], outside [S,nc] int32, points [S,n_out,3], src [S,n_out] int32, count [S] int32."""
    verts, dirs, cand = np.asarray(verts, F), np.asarray(dirs, F), np.asarray(cand, F)
    keep, cand_hull = np.asarray(keep, np.int32), np.asarray(cand_hull, np.int32)
    S, G, D, _ = verts.shape
    nc = cand.shape[1]
    sup = support_values(verts, dirs)
    thr = (sup - F(margin)).astype(F)
    outside = np.zeros((S, nc), np.int32)
    points = np.empty((S, n_out, 3), F)
    src = np.empty((S, n_out), np.int32)
    count = np.zeros((S,), np.int32)
    for s in range(S):
        val = dot(cand[s][:, None, :], dirs[None, :, :])                               # [nc,D]
        own = cand_hull[s]
        valid = (own >= 0) & (own < G)
        alive = valid & (keep[s][np.clip(own, 0, G - 1)] != 0)
        for h in range(G):
            if not keep[s, h]:
                continue
            inside = ~(val > thr[s, h][None, :]).any(1)
            alive &= ~(inside & (own != h))
        outside[s] = alive
        idx = np.nonzero(alive)[0]
        count[s] = idx.size
        i = np.arange(n_out)
        src[s] = idx[i % idx.size] if idx.size else i % nc
        points[s] = cand[s, src[s]]
    return sup, outside, points, src, count


# ---- inputs shared by the tests

def box_hull(lo, hi, dirs):
    """A box as a hull of D vertices: vertex d is the corner farthest along dirs[d] (the first of equals), what
    vpn_support_hulls makes of the box's corners."""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    corners = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)], F)
    return corners[np.argmax(dot(corners[:, None, :], np.asarray(dirs, F)[None]), 0)]


def ellipsoid_hull(centre, radii, dirs):
    """The support points of an ellipsoid along dirs: x = c + r * (r * d) / |r * d|, rounded to float32."""
    d = np.asarray(dirs, np.float64) * np.asarray(radii, np.float64)
    return (np.asarray(centre, np.float64) + np.asarray(radii, np.float64) * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


def lattice_dirs():
    """Six axis directions: support values of lattice hulls are exact."""
    return np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)


def box_points(lo, hi, n, seed):
    """n uniform points on the surface of a box (CPU stand-in for the mesh sampler) -> [n,3] float32."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    area = np.array([ext[1] * ext[2], ext[0] * ext[2], ext[0] * ext[1]])
    axis = rng.choice(3, n, p=area / area.sum())
    p = lo + rng.random((n, 3)) * ext
    p[np.arange(n), axis] = np.where(rng.random(n) < 0.5, lo[axis], hi[axis])
    return p.astype(F)


def ellipsoid_points(centre, radii, n, seed):
    """n points on an ellipsoid (normalised Gaussian directions, scaled) -> [n,3] float32."""
    v = np.random.default_rng(seed).standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (np.asarray(centre, np.float64) + v * np.asarray(radii, np.float64)).astype(F)


def inside_fp64(p, hull, dirs, slack):
    """fp64: is p [n,3] inside the outer polytope of hull [D,3] shrunk by `slack` -> [n] bool."""
    d = np.asarray(dirs, np.float64)
    s = (hull.astype(np.float64) @ d.T).max(0)
    return ((np.asarray(p, np.float64) @ d.T) <= s[None] - slack).all(1)
