"""Restatement of the ground-truth stage (modules/dataset.py::sample_gt_points, csrc/gtpoints.hip) in numpy:
area-weighted surface samples of a ragged batch of meshes, every fp32 operation rounded by itself (numpy's float32
arithmetic does that), the cumulative areas summed sequentially in float64 and rounded to fp32 where they are compared.
The GPU tests hold the kernels to this file bit for bit; tests/test_gtpoints_cpu.py holds this file to the oracle's
mesh_sample.  kaolin's TriangleMesh.sample is absent: parity with it stays unpinned (tests/test_mesh_path.py)."""
import numpy as np
import torch

from oracle import vpn_oracle as O

F32 = np.float32


def icosphere(sub=1, radius=1.0, stretch=(1.0, 1.0, 1.0)):
    """A subdivided icosahedron (20 * 4^sub faces) scaled per axis: (verts [P,3] fp32, faces [F,3] int64) as torch tensors.
    The same construction as tests/test_mesh_path.py::icosphere."""
    t = (1.0 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [list(np.array(p, np.float64) / np.linalg.norm(p)) for p in v]
    for _ in range(sub):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = (np.array(v[a]) + np.array(v[b])) / 2
                v.append(list(m / np.linalg.norm(m)))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    verts = (np.array(v, np.float64) * radius * np.array(stretch, np.float64)).astype(F32)
    return torch.from_numpy(verts), torch.tensor(f, dtype=torch.int64)


def corners(verts, faces):
    """The three corners [F,3] of every face, vertex indices clamped to [0, P - 1] as on the device."""
    v = np.asarray(verts, F32)
    f = np.clip(np.asarray(faces, np.int64), 0, v.shape[0] - 1)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def face_areas(verts, faces):
    """0.5f * sqrtf(nx nx + ny ny + nz nz), n = (b - a) x (c - a): fp32, every operation rounded by itself."""
    a, b, c = corners(verts, faces)
    u, w = b - a, c - a
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    return F32(0.5) * np.sqrt(nx * nx + ny * ny + nz * nz)


def cumulative_areas(areas):
    """Inclusive prefix sums in face order, accumulated sequentially in float64, rounded to fp32."""
    return np.cumsum(areas.astype(np.float64)).astype(F32)


def exact_sum_margin(areas):
    """F * (max area / min non-zero area): below 2^29 every float64 sum of these fp32 areas is exact in any order (each
    area is a multiple of 2^-24 of the smallest, every partial sum is below F times the largest: 53 bits suffice)."""
    nz = areas[areas > 0].astype(np.float64)
    return len(areas) * float(nz.max() / nz.min())


def uniforms(seed, mesh_index, set_index, n):
    """The Philox4x32-10 draws of (mesh, set): counter (point, 0xFFFFFFFF - set, mesh lo, mesh hi), key = seed; u = (word >> 8)
    2^-24.  Set 0 is oracle.vpn_oracle.philox_uniforms_mesh."""
    i = np.arange(n, dtype=np.uint32)
    ctr = np.stack([i, np.full(n, 0xFFFFFFFF - set_index, np.uint32), np.full(n, mesh_index & 0xFFFFFFFF, np.uint32),
                    np.full(n, (mesh_index >> 32) & 0xFFFFFFFF, np.uint32)], 1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    out = O.philox4x32_10(ctr, key)
    return (out[:, :3] >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)


def choose_faces(cum, u0):
    """The first face whose cumulative area exceeds u0 * total (fp32), else the last face."""
    target = np.asarray(u0, F32) * cum[-1]
    return np.minimum(np.searchsorted(cum, target, side='right'), len(cum) - 1)


def sample(verts, faces, u, xform=None):
    """One mesh, one set: u [n,3] -> (face [n] int64, bary [n,3], points [n,3]); xform [3,4] or None."""
    u = np.asarray(u, F32)
    a, b, c = corners(verts, faces)
    idx = choose_faces(cumulative_areas(face_areas(verts, faces)), u[:, 0])
    r = np.sqrt(u[:, 1])
    w0, w1, w2 = F32(1.0) - r, r * (F32(1.0) - u[:, 2]), r * u[:, 2]
    p = (w0[:, None] * a[idx] + w1[:, None] * b[idx]) + w2[:, None] * c[idx]
    if xform is not None:
        m = np.asarray(xform, F32)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        p = np.stack([((m[r_, 0] * x + m[r_, 1] * y) + m[r_, 2] * z) + m[r_, 3] for r_ in range(3)], 1)
    return idx, np.stack([w0, w1, w2], 1), p


def sample_batch(meshes, n, sets=1, *, seed=0, mesh_base=0, u=None, xforms=None, xform_mask=None):
    """sample_gt_points on a list of (verts, faces): (face [S,T,n], bary [S,T,n,3], points [S,T,n,3]) as torch tensors."""
    S = len(meshes)
    mask = (1 << sets) - 1 if xform_mask is None else xform_mask
    face = np.zeros((S, sets, n), np.int64)
    bary = np.zeros((S, sets, n, 3), F32)
    pts = np.zeros((S, sets, n, 3), F32)
    for s, (v, f) in enumerate(meshes):
        v, f = np.asarray(v, F32), np.asarray(f, np.int64)
        for t in range(sets):
            ut = np.asarray(u[s][t], F32) if u is not None else uniforms(seed, mesh_base + s, t, n)
            xf = np.asarray(xforms[s][t], F32) if xforms is not None and (mask >> t) & 1 else None
            face[s, t], bary[s, t], pts[s, t] = sample(v, f, ut, xf)
    return torch.from_numpy(face), torch.from_numpy(bary), torch.from_numpy(pts)
