"""Restatement of the outer-surface extraction (csrc/isosurface.hip) in vectorised numpy, stated twice: in
fp32 with every operation rounded by itself (what the kernels compute, bit for bit) and in float64; a plain triple loop of the
same definition; the checks a closed oriented mesh has to pass; and the inputs the tests share (four fixtures, two K = 16
assemblies of the benchmark's parameter distribution, a hand-made field)."""
import functools
import math

import numpy as np
import torch

import occupancy_ref as OR

SPHERE, CUBOID = OR.SPHERE, OR.CUBOID
FLT_MAX = float(np.finfo(np.float32).max)
AXES = ((0, 1, 2), (1, 2, 0), (2, 0, 1))                  # (a, u, v): the axis and the two others in cyclic order
EDGE_OFFSETS = ((0, 0), (1, 0), (0, 1), (1, 1))           # (ou, ov)


# ---- the lattice and the field

def lattice(dims, lo=-0.5, hi=0.5):
    """(cx, cy, cz, queries): the cell centres of the box [lo, hi] cut into dims = N or (Nx, Ny, Nz) cells, lo + (i + 0.5) (hi
    - lo) / N in float64 rounded to fp32 once; queries fp32 [Nz Ny Nx, 3], node (iz Ny + iy) Nx + ix."""
    dims = (dims,) * 3 if isinstance(dims, int) else tuple(dims)
    lo = (lo,) * 3 if isinstance(lo, (int, float)) else tuple(lo)
    hi = (hi,) * 3 if isinstance(hi, (int, float)) else tuple(hi)
    c = [np.array([lo[a] + (i + 0.5) * (hi[a] - lo[a]) / dims[a] for i in range(dims[a])], dtype=np.float64).astype(np.float32)
         for a in range(3)]
    z, y, x = np.meshgrid(c[2], c[1], c[0], indexing='ij')
    return c[0], c[1], c[2], np.stack([x, y, z], -1).reshape(-1, 3)


def prim_field(params, kinds, queries, dtype=torch.float64):
    """f [B,Q] = min_k (m_k - 1) over the primitives whose m_k is no NaN, +inf when none is left (torch, in `dtype`)."""
    m = OR.prim_m(params, kinds, queries, dtype) - 1
    return torch.where(torch.isnan(m), torch.full_like(m, math.inf), m).min(-1).values


def params_of(rows):
    """params fp32 [1,K,10] and kinds of fixture rows (kind, v, q, t)."""
    return (torch.tensor([[list(v) + list(q) + list(t) for _, v, q, t in rows]], dtype=torch.float64).float(),
            tuple(k for k, _, _, _ in rows))


Q0, T0 = (0.3, 0.5, 0.2, 0.13), (0.02, -0.03, 0.01)
FIXTURES = {
    'ellipsoid': [(SPHERE, (0.31, 0.22, 0.27), Q0, T0)],
    'cuboid': [(CUBOID, (0.25, 0.18, 0.3), Q0, T0)],
    'union3': [(CUBOID, (0.2, 0.12, 0.15), Q0, (-0.1, -0.03, 0.01)),
               (SPHERE, (0.18, 0.2, 0.12), (0.1, 0.2, 0.9, 0.31), (0.12, 0.05, 0.0)),
               (SPHERE, (0.1, 0.1, 0.25), (0.7, 0.1, 0.2, 0.77), (0.0, 0.1, -0.1))],
    'two_apart': [(SPHERE, (0.12, 0.1, 0.11), Q0, (-0.25, 0.0, 0.0)),
                  (CUBOID, (0.1, 0.12, 0.11), (0.1, 0.2, 0.9, 0.31), (0.25, 0.05, 0.0))],
    # crosses the lattice boundary on purpose: the sphere's centre is 0.1 from the face x = 0.5
    'crossing': [(SPHERE, (0.25, 0.2, 0.2), Q0, (0.4, 0.0, 0.0))],
}
COMPONENTS = {'ellipsoid': 1, 'cuboid': 1, 'union3': 1, 'two_apart': 2}
ELLIPSOID_VOLUME = 4.0 / 3.0 * math.pi * 0.31 * 0.22 * 0.27


def mixed(parts):
    """At how many positions the bool arrays `parts` (one shape) hold both values: bool array."""
    n = sum(x.astype(np.int64) for x in parts)
    return (n != 0) & (n != len(parts))


def lattice_topology(inside):
    """What the inside flags [Nz,Ny,Nx] alone say about the boundary of the solid, without any mesh: (Euler number = mixed
    cells - mixed lattice faces + sign-changing lattice edges, components = the connected components of the mixed cells, two
    cells being joined where the lattice face between them is mixed)."""
    cells = mixed([_corner(inside, i) for i in range(8)])                       # [ncz, ncy, ncx]
    index = np.arange(cells.size).reshape(cells.shape)
    n_faces, parent = 0, list(range(cells.size))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for ax in range(3):                                                         # the lattice faces normal to array axis `ax`
        b = np.moveaxis(inside, ax, 0)
        face = mixed([b[:, o1:b.shape[1] - 1 + o1, o2:b.shape[2] - 1 + o2] for o1 in (0, 1) for o2 in (0, 1)])
        n_faces += int(face.sum())
        idx = np.moveaxis(index, ax, 0)
        inner = face[1:-1]                                                      # a face between cell k - 1 and cell k along `ax`
        for lo, hi in zip(idx[:-1][inner].tolist(), idx[1:][inner].tolist()):
            ra, rb = find(lo), find(hi)
            if ra != rb:
                parent[ra] = rb
    n_edges = sum(int((np.take(inside, range(0, inside.shape[ax] - 1), ax) != np.take(inside, range(1, inside.shape[ax]), ax)).sum())
                  for ax in range(3))
    components = len({find(x) for x in index[cells].tolist()})
    return int(cells.sum()) - n_faces + n_edges, components


def on_boundary(a):
    """The part of a node array [Nz,Ny,Nx] in the six boundary faces of the lattice."""
    b = np.zeros(a.shape, dtype=bool)
    b[[0, -1]] = b[:, [0, -1]] = b[:, :, [0, -1]] = True
    return a[b]


def assembly(spread, seed=1234, K=16, tries=4096, sizes=(12, 16)):
    """params fp32 [1,K,10] and kinds of the benchmark's distribution (bench.py: v = (U + 0.1) / (8, 10, 10), q = U^4, t =
    spread (2 U - 1); K / 2 cuboids then spheres): the FIRST draw of the generator for which, on the lattices of N^3 cell
    centres of [-0.5, 0.5]^3 for every N of `sizes`, the float64 inside flags (a) hold no node in a boundary face of the
    lattice (the solid stays inside) and (b) bound a solid of sphere-like pieces: the lattice's own Euler number is twice its
    number of components (lattice_topology).  The rule replaces a draw whose solid leaves the lattice or has handles, voids or
    pinched sheets at this step; it looks at the parameters and the lattice alone, never at an extracted mesh."""
    g = torch.Generator().manual_seed(seed)
    kinds = (CUBOID,) * (K // 2) + (SPHERE,) * (K - K // 2)
    nodes = [torch.from_numpy(lattice(N)[3]) for N in sizes]
    for _ in range(tries):
        v = (torch.rand(1, K, 3, generator=g) + 0.1) / torch.tensor([8.0, 10.0, 10.0])
        q = torch.rand(1, K, 4, generator=g)
        t = spread * (torch.rand(1, K, 3, generator=g) * 2 - 1)
        params = torch.cat([v, q, t], 2).float().contiguous()
        for N, x in zip(sizes, nodes):
            inside = (prim_field(params, kinds, x).numpy() <= 0).reshape(N, N, N)
            if on_boundary(inside).any():
                break
            chi, components = lattice_topology(inside)
            if chi != 2 * components:
                break
        else:
            return params, kinds
    raise AssertionError('no draw passes the rule')


@functools.lru_cache(maxsize=None)
def case_params(name):
    if name in FIXTURES:
        return params_of(FIXTURES[name])
    return assembly({'assembly35': 0.35, 'assembly15': 0.15}[name])


@functools.lru_cache(maxsize=None)
def case_field(name, N):
    """(float64 field [N,N,N] of the float64 restatement on the fp32 lattice, (cx, cy, cz))."""
    cx, cy, cz, q = lattice(N)
    params, kinds = case_params(name)
    f = prim_field(params, kinds, torch.from_numpy(q)).numpy().reshape(N, N, N)
    return f, (cx, cy, cz)


def hand_field():
    """A (5,4,3) lattice (Nx = 5, Ny = 4, Nz = 3) with unequal steps and a field that is inside at five interior nodes, one
    of them by exactly 0: (field [3,4,5] fp32, (cx, cy, cz))."""
    cx = np.array([-0.5, -0.2, 0.0, 0.3, 0.7], dtype=np.float32)
    cy = np.array([-0.4, -0.1, 0.25, 0.5], dtype=np.float32)
    cz = np.array([-0.3, 0.1, 0.6], dtype=np.float32)
    f = np.full((3, 4, 5), 1.0, dtype=np.float32)
    f += (np.arange(60, dtype=np.float32).reshape(3, 4, 5) % 7) * np.float32(0.125)
    for (iz, iy, ix), v in (((1, 1, 1), -0.75), ((1, 1, 2), -0.25), ((1, 2, 2), -1.5), ((1, 2, 3), 0.0), ((1, 1, 3), -0.5)):
        f[iz, iy, ix] = v
    return f, (cx, cy, cz)


# ---- surface nets, vectorised, in one dtype

def signed(field, level, dtype):
    """s = field - level in `dtype` (fp32: the kernel's subtraction), NaN -> +FLT_MAX, clamped to +-FLT_MAX."""
    with np.errstate(over='ignore', invalid='ignore'):
        s = np.asarray(field, dtype=np.float32).astype(dtype) - np.float32(level).astype(dtype)
    s = np.where(np.isnan(s), dtype(FLT_MAX), s)
    return np.clip(s, dtype(-FLT_MAX), dtype(FLT_MAX)).astype(dtype)


def _corner(a, i):
    """The values of corner i = ox + 2 oy + 4 oz of every cell: [Nz-1, Ny-1, Nx-1]."""
    ox, oy, oz = i & 1, (i >> 1) & 1, i >> 2
    return a[oz:a.shape[0] - 1 + oz, oy:a.shape[1] - 1 + oy, ox:a.shape[2] - 1 + ox]


def surface_nets(field, coords, level=0.0, dtype=np.float64):
    """One sample: field [Nz,Ny,Nx] -> dict(verts [n_verts,3] `dtype`, faces int64 [n_faces,3], n_open, inside bool
    [Nz,Ny,Nx], cell_vertex int64 [cells] (-1: not active), t_min, t_max (the crossing parameters met))."""
    dtype = np.dtype(dtype).type
    s = signed(field, level, dtype)
    Nz, Ny, Nx = s.shape
    inside = s <= 0
    c = [np.asarray(coords[a], dtype=np.float32).astype(dtype) for a in range(3)]
    sc = [_corner(s, i) for i in range(8)]
    ic = [_corner(inside, i) for i in range(8)]
    n_in = sum(x.astype(np.int64) for x in ic)
    active = (n_in != 0) & (n_in != 8)
    shape = active.shape                                                        # (ncz, ncy, ncx)
    cell_vertex = np.where(active.ravel(), np.cumsum(active.ravel()) - 1, -1)
    # node coordinates of the low and the high corner of every cell along each axis
    grid = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing='ij')       # cz, cy, cx
    cell = (grid[2], grid[1], grid[0])                                          # by axis x, y, z
    lo = [c[a][cell[a]] for a in range(3)]
    hi = [c[a][cell[a] + 1] for a in range(3)]
    total = [np.zeros(shape, dtype=dtype) for _ in range(3)]
    count = np.zeros(shape, dtype=dtype)
    t_min, t_max = math.inf, -math.inf
    for a, u, v in AXES:
        for ou, ov in EDGE_OFFSETS:
            i = (ou << u) | (ov << v)
            j = i | (1 << a)
            change = ic[i] != ic[j]
            with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
                t = sc[i] / (sc[i] - sc[j])
                p = [None] * 3
                p[a] = lo[a] + t * (hi[a] - lo[a])
                p[u] = hi[u] if ou else lo[u]
                p[v] = hi[v] if ov else lo[v]
                for k in range(3):
                    total[k] = np.where(change, total[k] + p[k], total[k])
            count = np.where(change, count + dtype(1), count)
            if change.any():
                t_min, t_max = min(t_min, float(t[change].min())), max(t_max, float(t[change].max()))
    with np.errstate(invalid='ignore', divide='ignore'):
        verts = np.stack([(total[k] / count)[active] for k in range(3)], -1).astype(dtype)
    # faces: by owner cell, then axis, then the two triangles
    vid = cell_vertex.reshape(shape)
    step = {0: (0, 0, 1), 1: (0, 1, 0), 2: (1, 0, 0)}                           # the (cz, cy, cx) offset of a step along x, y, z
    keys, tris = [], []
    index = np.arange(active.size).reshape(shape)
    for a, u, v in AXES:
        own = (ic[0] != ic[1 << a]) & (cell[u] >= 1) & (cell[v] >= 1)
        z, y, x = np.nonzero(own)
        du, dv = step[u], step[v]
        c2 = vid[z, y, x]
        c0 = vid[z - du[0] - dv[0], y - du[1] - dv[1], x - du[2] - dv[2]]
        c1 = vid[z - dv[0], y - dv[1], x - dv[2]]
        c3 = vid[z - du[0], y - du[1], x - du[2]]
        out = ic[0][z, y, x]                                                    # the edge runs from inside to outside
        b1, b3 = np.where(out, c1, c3), np.where(out, c3, c1)
        tris.append(np.stack([np.stack([c0, b1, c2], -1), np.stack([c0, c2, b3], -1)], 1))       # [n,2,3]
        keys.append(index[z, y, x] * 3 + a)
    keys, tris = np.concatenate(keys), np.concatenate(tris)
    order = np.argsort(keys, kind='stable')
    faces = tris[order].reshape(-1, 3).astype(np.int64)
    # open edges: every sign-changing lattice edge in one of the six boundary faces
    n_open = 0
    iz, iy, ix = np.meshgrid(np.arange(Nz), np.arange(Ny), np.arange(Nx), indexing='ij')
    edge_z, edge_y, edge_x = (iz == 0) | (iz == Nz - 1), (iy == 0) | (iy == Ny - 1), (ix == 0) | (ix == Nx - 1)
    n_open += int(((inside[:, :, :-1] != inside[:, :, 1:]) & (edge_y | edge_z)[:, :, :-1]).sum())
    n_open += int(((inside[:, :-1, :] != inside[:, 1:, :]) & (edge_z | edge_x)[:, :-1, :]).sum())
    n_open += int(((inside[:-1, :, :] != inside[1:, :, :]) & (edge_x | edge_y)[:-1, :, :]).sum())
    return dict(verts=verts, faces=faces, n_open=n_open, inside=inside, cell_vertex=cell_vertex, t_min=t_min, t_max=t_max)


def padded(result, max_verts, max_faces):
    """(verts fp32 [max_verts,3], faces int32 [max_faces,3], counts [4]) as the kernels write one sample."""
    nv, nf = result['verts'].shape[0], result['faces'].shape[0]
    verts, faces = np.zeros((max_verts, 3), dtype=np.float32), np.zeros((max_faces, 3), dtype=np.int32)
    overflow = int(nv > max_verts or nf > max_faces)
    if not overflow:
        verts[:nv], faces[:nf] = result['verts'].astype(np.float32), result['faces']
    return verts, faces, np.array([nv, nf, result['n_open'], overflow], dtype=np.int32)


# ---- the same definition as plain loops, in Python floats

def surface_nets_plain(field, coords, level=0.0):
    """(verts list of [x,y,z], faces list of [a,b,c], n_open) by loops over cells and edges."""
    f = np.asarray(field, dtype=np.float32)
    Nz, Ny, Nx = f.shape
    N, cs = (Nx, Ny, Nz), [[float(x) for x in coords[a]] for a in range(3)]

    def s(n):                                                                   # n = (ix, iy, iz)
        x = float(f[n[2], n[1], n[0]]) - float(np.float32(level))
        return FLT_MAX if math.isnan(x) else max(-FLT_MAX, min(FLT_MAX, x))

    def unit(a):
        return tuple(1 if k == a else 0 for k in range(3))

    def add(n, *ds):
        return tuple(n[k] + sum(d[k] for d in ds) for k in range(3))

    cells = [(x, y, z) for z in range(Nz - 1) for y in range(Ny - 1) for x in range(Nx - 1)]
    verts, number = [], {}
    for cell in cells:
        total, n = [0.0, 0.0, 0.0], 0
        corners = [s(add(cell, (i & 1, (i >> 1) & 1, i >> 2))) <= 0 for i in range(8)]
        if all(corners) or not any(corners):
            continue
        for a, u, v in AXES:
            for ou, ov in EDGE_OFFSETS:
                off = [0, 0, 0]
                off[u], off[v] = ou, ov
                na = add(cell, off)
                nb = add(na, unit(a))
                sa, sb = s(na), s(nb)
                if (sa <= 0) == (sb <= 0):
                    continue
                t = sa / (sa - sb)
                p = [cs[k][na[k]] for k in range(3)]
                p[a] = cs[a][na[a]] + t * (cs[a][nb[a]] - cs[a][na[a]])
                total, n = [total[k] + p[k] for k in range(3)], n + 1
        number[cell] = len(verts)
        verts.append([x / n for x in total])
    faces, n_open = [], 0
    for cell in cells:
        for a, u, v in AXES:
            sa, sb = s(cell), s(add(cell, unit(a)))
            if (sa <= 0) == (sb <= 0) or cell[u] < 1 or cell[v] < 1:
                continue
            du, dv = tuple(-x for x in unit(u)), tuple(-x for x in unit(v))
            c0, c1, c2, c3 = number[add(cell, du, dv)], number[add(cell, dv)], number[cell], number[add(cell, du)]
            faces += [[c0, c1, c2], [c0, c2, c3]] if sa <= 0 else [[c0, c3, c2], [c0, c2, c1]]
    for a, u, v in AXES:
        for n in [(x, y, z) for z in range(Nz) for y in range(Ny) for x in range(Nx)]:
            if n[a] + 1 < N[a] and (s(n) <= 0) != (s(add(n, unit(a))) <= 0) and (n[u] in (0, N[u] - 1) or n[v] in (0, N[v] - 1)):
                n_open += 1
    return verts, faces, n_open


# ---- what a closed oriented mesh has to pass

def unmatched_edges(faces):
    """The directed edges (a, b) of `faces` that are not matched by (b, a) as often as they occur: int64 [n,2]."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    width = int(e.max()) + 1 if e.size else 1
    fwd, n_fwd = np.unique(e[:, 0] * width + e[:, 1], return_counts=True)
    back = dict(zip(*(x.tolist() for x in np.unique(e[:, 1] * width + e[:, 0], return_counts=True))))
    bad = [k for k, n in zip(fwd.tolist(), n_fwd.tolist()) if back.get(k, 0) != n]
    return np.array([[k // width, k % width] for k in bad], dtype=np.int64).reshape(-1, 2)


def euler_and_components(n_verts, faces):
    """(V - E + F with E the undirected edges, the number of connected components of the vertices over the edges)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    e = np.unique(e, axis=0)
    parent = list(range(n_verts))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in e.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    return n_verts - e.shape[0] + f.shape[0], len({find(x) for x in range(n_verts)})


def mesh_volume(verts, faces):
    """The signed volume of a closed mesh, in float64: sum of a . (b x c) / 6."""
    v = np.asarray(verts, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return float((v[:, 0] * np.cross(v[:, 1], v[:, 2])).sum() / 6)


def winding_at(verts, faces, points, chunk=512):
    """float64 winding numbers of one mesh at points [Q,3] through occupancy_ref.winding, a chunk of queries at a time."""
    v, f = torch.as_tensor(np.asarray(verts, dtype=np.float64))[None], torch.as_tensor(np.asarray(faces, dtype=np.int64))
    x = torch.as_tensor(np.asarray(points, dtype=np.float64))
    return torch.cat([OR.winding(v, f, x[i:i + chunk])[0] for i in range(0, x.shape[0], chunk)]).numpy()
