"""numpy restatement of csrc/reconstruct.hip (include/vpn_hip.h): float32 arithmetic rounded per operation,
sums x, y, z from the left, int64 fixed-point means.  numpy's float32 arrays round every operation by itself, which is the
arithmetic the kernels are built for (-ffp-contract=off); np.argmax / np.argmin return the FIRST extreme element, which is
the tie rule (lowest point index, lowest centre)."""
import numpy as np

FIX = np.float32(2.0 ** 20)


def int_mean(pts):
    """[m,3] float32, m >= 1 -> [3] float32: sum of rint(x * 2^20) as int64, one division in double, one rounding."""
    s = np.rint(pts.astype(np.float32) * FIX).astype(np.int64).sum(0)
    return (s.astype(np.float64) / (np.float64(pts.shape[0]) * 2.0 ** 20)).astype(np.float32)


def dist2(p, c):
    """p [...,3], c [...,3] float32 -> ((dx dx + dy dy) + dz dz), every operation rounded to float32."""
    d = (p - c).astype(np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def dot(p, d):
    return (p[..., 0] * d[..., 0] + p[..., 1] * d[..., 1]) + p[..., 2] * d[..., 2]


def cluster_one(p, H, iters):
    p = np.ascontiguousarray(p, dtype=np.float32)
    n = p.shape[0]
    centres = np.empty((H, 3), np.float32)
    mind = dist2(p, int_mean(p)[None])
    for k in range(H):
        j = int(np.argmax(mind))                          # first of the largest: the lowest point index
        centres[k] = p[j]
        d = dist2(p, centres[k][None])
        mind = d if k == 0 else np.minimum(mind, d)

    def assign():
        d = np.stack([dist2(p, centres[h][None]) for h in range(H)], 1)      # [n,H]
        return np.argmin(d, 1).astype(np.int32)           # first of the smallest: the lowest centre

    for _ in range(iters):
        lab = assign()
        for h in range(H):
            if (lab == h).any():
                centres[h] = int_mean(p[lab == h])        # an empty cluster keeps its centre
    lab = assign()
    assert n == lab.shape[0]
    return lab, centres, np.bincount(lab, minlength=H).astype(np.int32)


def cluster_points(points, H, iters):
    """points [B,n,3] -> labels [B,n] int32, centres [B,H,3] float32, counts [B,H] int32."""
    out = [cluster_one(p, H, iters) for p in np.asarray(points, dtype=np.float32)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def support_hulls(points, labels, centres, dirs):
    """-> verts [B,H*D,3] float32, support [B,H*D] int32."""
    points, dirs = np.asarray(points, dtype=np.float32), np.asarray(dirs, dtype=np.float32)
    B, n, _ = points.shape
    H, D = centres.shape[1], dirs.shape[0]
    verts = np.empty((B, H * D, 3), np.float32)
    support = np.empty((B, H * D), np.int32)
    for b in range(B):
        for h in range(H):
            idx = np.nonzero(labels[b] == h)[0]
            if idx.size == 0:
                verts[b, h * D:(h + 1) * D] = centres[b, h]
                support[b, h * D:(h + 1) * D] = -1
                continue
            val = dot(points[b, idx][:, None, :], dirs[None, :, :])          # [m,D]
            win = idx[np.argmax(val, 0)]                  # first of the largest: the lowest point index
            verts[b, h * D:(h + 1) * D] = points[b, win]
            support[b, h * D:(h + 1) * D] = win
    return verts, support


def hull_faces(template_faces, H, D):
    """The template's faces repeated with a per-hull vertex offset -> [H*Ft,3] int32."""
    f = np.asarray(template_faces, dtype=np.int64)
    return np.concatenate([f + h * D for h in range(H)]).astype(np.int32)


def atlas(H, D, colors):
    """The uv / texture rule of convex_decomposition.py:32-53 for H hulls of D vertices: uv [H*D,2] float32 with every vertex
    of hull i at i/H + 0.01 (the Python double, rounded to float32 by torch.full), texture [3,1,H] with texel i = colors[i]."""
    uv = np.repeat(np.array([i / H + 0.01 for i in range(H)], dtype=np.float64).astype(np.float32), D)
    return np.stack([uv, uv], 1), np.asarray(colors, dtype=np.float32).T.reshape(3, 1, H)


def lattice_cloud(side=6):
    """side^3 points on a dyadic lattice in [-0.5, 0.5): distances and axis-aligned support values are exact, so equal
    values abound and only the tie rules decide."""
    g = (np.arange(side, dtype=np.float32) - side // 2) / np.float32(8.0)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)


AXIS_DIRS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [0, -1, -1]], dtype=np.float32)


def random_dirs(D, seed=0):
    v = np.random.default_rng(seed).standard_normal((D, 3)).astype(np.float32)
    return (v / np.sqrt((v * v).sum(1, keepdims=True))).astype(np.float32)
