"""The mesh regularisers (vpn_amd.mesh_regularizers, csrc/meshreg.hip) stated in plain torch, in the dtype of
the vertices (float64 is the specification), with the topology built by plain Python loops, independently of
ops.mesh_topology.  Shared by tests/test_meshreg_cpu.py and tests/test_meshreg.py, with the meshes and inputs both use.

verts [B,V,3], one face list [F,3] for the batch.

  topology  unique undirected edges (a < b), E of them.  A face with a repeated index gives its edges but is no face for the
            normal term.  Every edge with exactly two distinct incident faces is one pair (f, g, s), f < g: s = +1 when the
            two faces traverse the edge in opposite directions (consistent winding), else -1.  An edge of one face is a
            boundary edge, one of three or more is non-manifold; neither gives a pair.
  edge      mean over (b, e) of (|v_a - v_b| - l0)^2; with l0 = 0 it is |d|^2 without a root; with l0 > 0 an edge of length
            exactly 0 has gradient 0.  0 when E = 0.
  lap       delta_i = (1 / deg_i) sum_{j in N(i)} v_j - v_i, 0 for a vertex in no edge; mean over (b, i), all V vertices, of
            |delta_i|^2.
  normal    n_f = (v1 - v0) x (v2 - v0); cos = s n_f.n_g / (max(|n_f|, 1e-8) max(|n_g|, 1e-8)), a clamped norm being a
            constant in the gradient; mean over (b, pair) of 1 - cos.  0 when there is no pair.
"""
import functools
import math

import torch

TERMS = ('edge', 'lap', 'normal')
NORM_FLOOR = 1e-8


def topology(faces, n):
    """dict(edges [(a, b)] sorted, neighbours [sorted list per vertex], pairs [(f, g, s)] sorted, n_boundary, n_nonmanifold)."""
    faces = [tuple(int(i) for i in f) for f in faces.tolist()]
    edges, incident = set(), {}
    for fi, (a, b, c) in enumerate(faces):
        assert 0 <= min(a, b, c) and max(a, b, c) < n
        real = len({a, b, c}) == 3
        for p, q in ((a, b), (b, c), (c, a)):
            if p == q:
                continue
            e = (min(p, q), max(p, q))
            edges.add(e)
            if real:
                incident.setdefault(e, []).append((fi, p < q))
    neighbours = [set() for _ in range(n)]
    for a, b in edges:
        neighbours[a].add(b)
        neighbours[b].add(a)
    pairs, n_boundary, n_nonmanifold = [], 0, 0
    for e, inc in incident.items():
        if len(inc) == 1:
            n_boundary += 1
        elif len(inc) >= 3:
            n_nonmanifold += 1
        else:
            (f, df), (g, dg) = sorted(inc)
            pairs.append((f, g, 1 if df != dg else -1))
    return dict(edges=sorted(edges), neighbours=[sorted(s) for s in neighbours], pairs=sorted(pairs), n_boundary=n_boundary,
                n_nonmanifold=n_nonmanifold)


def regularizers(verts, faces, l0=0.0, terms=TERMS, topo=None):
    """[3] = (edge, lap, normal) in verts' dtype, differentiable; a term outside `terms` is 0."""
    B, V, _ = verts.shape
    topo = topo or topology(faces, V)
    zero = verts.new_zeros(())
    out = [zero, zero, zero]
    if 'edge' in terms and topo['edges']:
        e = torch.tensor(topo['edges'], dtype=torch.long)
        d = verts[:, e[:, 0]] - verts[:, e[:, 1]]
        q = (d * d).sum(-1)
        if l0 == 0.0:
            out[0] = q.mean()
        else:
            hit = q > 0
            length = torch.sqrt(torch.where(hit, q, torch.ones_like(q)))          # no root at 0: the gradient there is 0
            out[0] = torch.where(hit, (length - l0) ** 2, torch.full_like(q, l0 * l0)).mean()
    if 'lap' in terms and topo['edges']:
        rows = torch.tensor([i for i, nb in enumerate(topo['neighbours']) for _ in nb], dtype=torch.long)
        cols = torch.tensor([j for nb in topo['neighbours'] for j in nb], dtype=torch.long)
        deg = torch.tensor([len(nb) for nb in topo['neighbours']], dtype=verts.dtype)
        s = verts.new_zeros(B, V, 3).index_add(1, rows, verts[:, cols])
        has = (deg > 0)[None, :, None]
        delta = torch.where(has, s / deg.clamp_min(1)[None, :, None] - verts, torch.zeros_like(verts))
        out[1] = (delta * delta).sum(-1).mean()
    if 'normal' in terms and topo['pairs']:
        f = faces.long()
        n = torch.cross(verts[:, f[:, 1]] - verts[:, f[:, 0]], verts[:, f[:, 2]] - verts[:, f[:, 0]], dim=-1)
        sq = (n * n).sum(-1)
        root = torch.sqrt(torch.where(sq > 0, sq, torch.ones_like(sq)))                 # no root at 0, as for the edges
        norm = torch.where((sq > 0) & (root > NORM_FLOOR), root, torch.full_like(sq, NORM_FLOOR))   # clamped: a constant
        p = torch.tensor(topo['pairs'], dtype=torch.long)
        cos = p[:, 2].to(verts.dtype) * (n[:, p[:, 0]] * n[:, p[:, 1]]).sum(-1) / (norm[:, p[:, 0]] * norm[:, p[:, 1]])
        out[2] = (1 - cos).mean()
    return torch.stack(out)


def reference(verts, faces, l0=0.0, terms=TERMS, upstream=(1.0, 1.0, 1.0), dtype=torch.float64):
    """(values [3], dverts [B,V,3]) of the restatement in `dtype` for loss = sum_k upstream[k] values[k]."""
    v = verts.detach().to(dtype).clone().requires_grad_(True)
    out = regularizers(v, faces, l0, terms)
    loss = (out * torch.tensor(upstream, dtype=dtype)).sum()
    dv = torch.autograd.grad(loss, v, allow_unused=True)[0] if loss.requires_grad else None
    return out.detach(), dv if dv is not None else torch.zeros_like(v)


# ---- meshes: (faces [F,3] int64, n)

def tetrahedron():
    return torch.tensor([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]]), 4


def tetrahedron_flipped():
    """The tetrahedron with face 1 traversed the other way: its three pairs have s = -1."""
    return torch.tensor([[0, 1, 2], [0, 3, 2], [0, 3, 1], [1, 3, 2]]), 4


def strip(n):
    """An open triangle strip over n vertices (n - 2 faces, consistent winding): vertex i neighbours i +- 1, i +- 2."""
    return torch.tensor([[i, i + 1, i + 2] if i % 2 == 0 else [i + 1, i, i + 2] for i in range(n - 2)]), n


def irregular():
    import gcn_input_ref as G
    return G.irregular_mesh()


def fan(valence=70):
    """A closed fan around vertex 0: valence `valence`, more than a wave."""
    return torch.tensor([[0, 1 + i, 1 + (i + 1) % valence] for i in range(valence)]), valence + 1


def sphere():
    from vpn_amd.modules.meshing import uv_sphere
    v, f = uv_sphere()
    return f.long(), int(v.shape[0])


def two_components():
    """A tetrahedron and, apart from it, a strip of 5 vertices."""
    t, _ = tetrahedron()
    s, _ = strip(5)
    return torch.cat([t, s + 4]), 9


def composed(k=16):
    """k uv_sphere()s on consecutive index ranges: the topology of the composed primitive mesh (k = 16: V = 2048)."""
    f, n = sphere()
    return torch.cat([f + i * n for i in range(k)]), k * n


MESHES = {'tetrahedron': tetrahedron, 'tetrahedron_flipped': tetrahedron_flipped, 'strip_7': lambda: strip(7),
          'irregular': irregular, 'fan_70': fan, 'uv_sphere': sphere, 'two_components': two_components,
          'strip_65': lambda: strip(65), 'strip_130': lambda: strip(130)}


@functools.lru_cache(maxsize=None)
def mesh(name):
    return composed() if name == 'composed' else MESHES[name]()


@functools.lru_cache(maxsize=None)
def vertices(name, B):
    """fp32 [B,V,3] for mesh `name`: a shape that belongs to the topology (so the faces have area and the normals a
    direction), scaled and moved per sample, plus 0.1 tanh(0.1 randn), the size of a refinement step."""
    faces, n = mesh(name)
    gen = torch.Generator().manual_seed(1000 * B + sum(map(ord, name)))
    if name in ('uv_sphere', 'composed'):
        from vpn_amd.modules.meshing import uv_sphere
        k = n // 128
        scale = 0.05 + 0.35 * torch.rand(B, k, 1, 3, generator=gen)
        offset = torch.rand(B, k, 1, 3, generator=gen) - 0.5
        base = (uv_sphere()[0].float()[None, None] * scale + offset).reshape(B, n, 3)
    elif name.startswith('strip'):
        i = torch.arange(n, dtype=torch.float32)
        base = torch.stack([0.05 * i, 0.1 * (i % 2), 0.03 * torch.sin(0.7 * i)], 1)[None].repeat(B, 1, 1)
    elif name == 'fan_70':
        a = torch.arange(70, dtype=torch.float32) * (2 * math.pi / 70)
        rim = torch.stack([0.4 * torch.cos(a), 0.4 * torch.sin(a), 0.05 * torch.cos(3 * a)], 1)
        base = torch.cat([torch.tensor([[0.0, 0.0, 0.2]]), rim])[None].repeat(B, 1, 1)
    else:
        base = torch.rand(B, n, 3, generator=gen) - 0.5
    noise = 0.1 * torch.tanh(0.1 * torch.randn(B, n, 3, generator=gen))
    return (base + noise).float().contiguous()


@functools.lru_cache(maxsize=None)
def reference64(name, B, l0, terms=TERMS, upstream=(1.0, 1.0, 1.0)):
    return reference(vertices(name, B), mesh(name)[0], l0, terms, upstream)


@functools.lru_cache(maxsize=None)
def reference32(name, B, l0, terms=TERMS, upstream=(1.0, 1.0, 1.0)):
    return reference(vertices(name, B), mesh(name)[0], l0, terms, upstream, dtype=torch.float32)


def degenerate():
    """(verts [1,6,3] fp32, faces, l0): every coordinate a small multiple of 1/4, so every product below is exact in fp32
    and float64 alike.  Face (0, 1, 2) has area 0 (2 = the midpoint side: collinear), vertices 4 and 5 coincide, so edge
    (4, 5) has length 0 and faces (3, 4, 5) has area 0 as well; faces (0, 2, 3) and (2, 1, 3) are sound."""
    v = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.5, 1.0, 0.25], [1.5, 1.0, 0.0], [1.5, 1.0, 0.0]]])
    f = torch.tensor([[0, 1, 2], [0, 2, 3], [2, 1, 3], [3, 4, 5], [1, 4, 3]])
    return v, f, 0.25
