"""The plain GCN input op (ops.GcnInputFunction, vpn_gcn_input_fwd / _bwd of csrc/gcn.hip) for the tests: the
cases both test files share and their float64 statement through tests/gcn_ref.py -- the row cat(encoding | pooled | global)
as gcn_factored_ref.plain forms it with weight = identity, loss = (x * R).sum().  Every case is fp32, seeded and built on the
CPU.  Also here: the meshes of the aggregation edge cases and the images of the bounds cases.

Decidability.  The bilinear weight is continuous across a cell edge, its derivative is not: a vertex whose fp32 and float64
floor(ix) differ has no comparable gradient.  build() returns a mask of the vertices within EDGE_PX of a cell edge at any
level (except coordinates that are the same integer in both precisions: both floor them alike) and asserts that the floors
of every other vertex agree; the masked rows leave the dverts comparisons only."""
import functools

import torch

import gcn_factored_ref as F
import gcn_ref as R

SMALL_SQUARE = [(4, 32, 32), (8, 16, 16), (16, 8, 8), (32, 4, 4)]
EDGE_PX = 1e-4
MAX_MASKED = 0.01
# name -> dict(maps [(C, H, W)], img (H, W) of the images the bounds come from, G, venc, B, N)
_BASE = dict(maps=SMALL_SQUARE, img=(64, 64), G=16, venc=39, B=2, N=256)
CASES = {
    'small_square': dict(_BASE),
    'nonsquare': dict(_BASE, maps=[(5, 12, 16), (3, 6, 8), (7, 3, 4), (2, 1, 2)], img=(48, 64), G=3, N=300),
    'channel_tails': dict(_BASE, maps=[(65, 8, 8), (130, 4, 4)], G=0, venc=3, N=203),
    'two_levels_no_enc': dict(_BASE, maps=SMALL_SQUARE[:2], venc=0),
    'one_level_1x1': dict(_BASE, maps=[(6, 1, 1)], G=0, venc=3, N=64),
    'ties': dict(_BASE),
    'empty_image': dict(_BASE),
    'one_column': dict(_BASE),
    'corners_outside': dict(_BASE),
    'crowded': dict(_BASE),
    'n1025': dict(_BASE, N=1025),
    'n8192': dict(_BASE, G=0, venc=3, B=1, N=8192),
    'n8193': dict(_BASE, G=0, venc=3, B=1, N=8193),          # one beyond the sort's limit: see test_gcn_input.py
}
PARITY_CASES = [k for k in CASES if k != 'n8193']
# the planted ties: vertex indices per extent.  13 holds zmax and ymax; no group starts at 0, every group's lowest index has
# a near neighbour in another group, so "last wins" and "any wins" both give another dverts
TIE_GROUPS = {'zmax': [11, 13, 57, 130, 251], 'zmin': [9, 12, 77], 'ymax': [10, 13, 90, 201], 'ymin': [14, 15]}
TIE_VALUE = 0.625                                            # beyond the cube [-0.5, 0.5), dyadic


def _box_images(B, H, W, gen):
    rgbs = torch.zeros(B, 3, H, W)
    for b in range(B):
        y0, x0 = int(torch.randint(1, H // 4, (1,), generator=gen)), int(torch.randint(1, W // 4, (1,), generator=gen))
        rgbs[b, :, y0:H - y0, x0:W - 2 * x0] = 0.5
    return rgbs


def grid_coordinates(verts, bounds, maps):
    """Per level (ix, iy) [B,N] in the dtype of verts: gcn.py:152-153 operation for operation, then grid_sample's
    align_corners source index."""
    zmax, zmin = verts[..., 2].max(1, keepdim=True)[0], verts[..., 2].min(1, keepdim=True)[0]
    ymax, ymin = verts[..., 1].max(1, keepdim=True)[0], verts[..., 1].min(1, keepdim=True)[0]
    b = bounds[:, None, :]
    gx = b[..., 0] + (1 - (verts[..., 2] - zmin) / (zmax - zmin)) * (b[..., 1] - b[..., 0])
    gy = b[..., 2] + (1 - (verts[..., 1] - ymin) / (ymax - ymin)) * (b[..., 3] - b[..., 2])
    return [(((gx + 1) / 2) * (W - 1), ((gy + 1) / 2) * (H - 1)) for _, H, W in maps]


def extent_rows(verts):
    """[B,N] bool: the vertices holding zmin, zmax, ymin or ymax of their sample in float64, every vertex of a tie included."""
    v = verts.double()
    z, y = v[..., 2], v[..., 1]
    return ((z == z.max(1, keepdim=True)[0]) | (z == z.min(1, keepdim=True)[0]) |
            (y == y.max(1, keepdim=True)[0]) | (y == y.min(1, keepdim=True)[0]))


def undecidable_rows(verts, bounds, maps):
    """[B,N] bool mask of the module docstring; asserts that fp32 and float64 floors agree outside it."""
    shapes = [tuple(m.shape[1:]) for m in maps]
    c32 = grid_coordinates(verts, bounds, shapes)
    c64 = grid_coordinates(verts.double(), bounds.double(), shapes)
    mask = torch.zeros(verts.shape[:2], dtype=torch.bool)
    sized = [(a32, a64, n) for (_, H, W), l32, l64 in zip(shapes, c32, c64) for a32, a64, n in zip(l32, l64, (W, H))]
    for a32, a64, n in sized:                               # the edges are the integers -1 .. n; beyond them nothing is read
        near = ((a64 - a64.round()).abs() < EDGE_PX) & (a64.round() >= -1) & (a64.round() <= n)
        same_integer = (a32.double() == a64) & (a64 == a64.round())
        mask |= near & ~same_integer
    for a32, a64, n in sized:
        f32, f64 = a32.double().floor().clamp(-2, n), a64.floor().clamp(-2, n)
        assert torch.equal(f32[~mask], f64[~mask])
    return mask


def cell_counts(verts, bounds, H, W):
    """Per sample the vertex counts of the non-empty bilinear cells (x0 + 1, y0 + 1) of an H x W level, from the float64 grid
    (every vertex of the cases that use this has a corner in range)."""
    ix, iy = grid_coordinates(verts.double(), bounds.double(), [(0, H, W)])[0]
    assert bool(((ix > -1) & (ix < W) & (iy > -1) & (iy < H)).all())
    cell = (iy.floor().long() + 1) * (W + 1) + ix.floor().long() + 1
    return [torch.bincount(c)[torch.bincount(c) > 0] for c in cell]


def _plant_ties(verts):
    for b in range(verts.shape[0]):
        verts[b, TIE_GROUPS['zmax'], 2] = TIE_VALUE
        verts[b, TIE_GROUPS['zmin'], 2] = -TIE_VALUE
        verts[b, TIE_GROUPS['ymax'], 1] = TIE_VALUE
        verts[b, TIE_GROUPS['ymin'], 1] = -TIE_VALUE


def _crowd(verts, gen):
    """198 vertices in a box of side 1e-3, clusters of 7, 4 and 5 in boxes of their own, each at a (y, z) centre (cell counts of every residue mod 4:
    the unrolled loop of gcn_pool_bwd_kernel and each length of its tail), the other 42 spread, four of them pinned to the
    cube's faces so that the extents do not depend on the crowd."""
    n = 0
    for count, centre in ((198, (0.1332, -0.1839)), (7, (-0.3047, 0.2514)), (4, (0.3561, 0.1203)), (5, (-0.1523, -0.3581))):
        for b in range(verts.shape[0]):
            verts[b, n:n + count, 1:] = torch.tensor(centre) + (torch.rand(count, 2, generator=gen) - 0.5) * 1e-3
        n += count
    verts[:, n, 2], verts[:, n + 1, 2], verts[:, n + 2, 1], verts[:, n + 3, 1] = 0.5, -0.5, 0.5, -0.5


def build(name):
    """dict(verts [B,N,3], bounds [B,4], glob [B,G] | None, venc, maps, R [B,N,ctot], masked [B,N] bool, extent [B,N] bool)
    in fp32, with the case's own conditions asserted."""
    spec = CASES[name]
    gen = torch.Generator().manual_seed(2000 + sorted(CASES).index(name))
    B, N, G, venc = spec['B'], spec['N'], spec['G'], spec['venc']
    verts = torch.rand(B, N, 3, generator=gen) - 0.5
    H, W = spec['img']
    rgbs = _box_images(B, H, W, gen)
    if name == 'ties':
        _plant_ties(verts)
    elif name == 'crowded':
        _crowd(verts, gen)
    elif name == 'empty_image':
        rgbs.zero_()
    elif name == 'one_column':
        rgbs.zero_()
        rgbs[:, :, 10:51, 20] = 0.5
    bounds = torch.tensor([F.WIDE_BOUNDS] * B) if name == 'corners_outside' else R.bounds(rgbs)
    maps = [torch.randn(B, c, h, w, generator=gen) for c, h, w in spec['maps']]
    glob = torch.randn(B, G, generator=gen) if G else None
    ctot = venc + sum(c for c, _, _ in spec['maps']) + G
    case = dict(name=name, verts=verts, bounds=bounds, glob=glob, venc=venc, maps=maps,
                R=torch.randn(B, N, ctot, generator=gen))
    case['masked'] = undecidable_rows(verts, bounds, maps)
    case['extent'] = extent_rows(verts)
    assert float(case['masked'].double().mean()) <= MAX_MASKED, (name, int(case['masked'].sum()))
    assert not bool((case['masked'] & case['extent']).any()), name
    if name == 'empty_image':
        assert torch.equal(bounds, torch.tensor([[-1.0, 1.0, -1.0, 1.0]] * B))
    elif name == 'one_column':
        assert bool((bounds[:, 0] == bounds[:, 1]).all()) and bool((bounds[:, 2] < bounds[:, 3]).all())
    elif name == 'corners_outside':
        out, inside = F.outside_fractions(verts, bounds, 32)
        assert out >= 0.2 and inside >= 0.2, (out, inside)
    elif name == 'crowded':
        for counts in cell_counts(verts, bounds, 32, 32):
            assert int(counts.max()) >= 128 and set((counts % 4).tolist()) == {0, 1, 2, 3}, counts
    elif name == 'ties':
        check_tie_layout(case)
    return case


@functools.lru_cache(maxsize=None)
def case(name):
    """build(name), once per process: shared by the tests, which leave it unchanged."""
    return build(name)


@functools.lru_cache(maxsize=None)
def reference64(name):
    return reference(case(name))


@functools.lru_cache(maxsize=None)
def reference32(name):
    """The restatement evaluated in fp32 on the CPU: its distance from reference64 is the reference's own fp32 error."""
    return reference(case(name), torch.float32)


def check_tie_layout(case):
    v = case['verts']
    groups = sorted(TIE_GROUPS.values())
    assert [len(TIE_GROUPS[k]) for k in ('zmax', 'zmin', 'ymax', 'ymin')] == [5, 3, 4, 2]
    assert len(set(TIE_GROUPS['zmax']) & set(TIE_GROUPS['ymax'])) == 1
    for g in groups:
        low = min(g)
        assert low != 0 and any(abs(low - i) <= 2 for h in groups if h is not g for i in h)
    for b in range(v.shape[0]):
        for key, col, pick in (('zmax', 2, torch.max), ('zmin', 2, torch.min), ('ymax', 1, torch.max), ('ymin', 1, torch.min)):
            hold = (v[b, :, col] == pick(v[b, :, col])).nonzero().flatten().tolist()
            assert hold == TIE_GROUPS[key], (key, hold)
    tied = torch.zeros(v.shape[1], dtype=torch.bool)
    tied[sum(groups, [])] = True
    assert torch.equal(case['extent'], tied[None].expand(v.shape[0], -1))


def later_tie_rows():
    """{vertex: columns of dverts that carry no extent term}: every index of a tie group but its lowest."""
    rows = {}
    for key, g in TIE_GROUPS.items():
        for i in sorted(g)[1:]:
            rows.setdefault(i, []).append(2 if key[0] == 'z' else 1)
    return rows


def row(verts, bounds, glob, venc, maps):
    """cat(encoding | pooled | global) in the dtype of the inputs: gcn_factored_ref.plain with weight = identity."""
    ctot = venc + sum(m.shape[1] for m in maps) + (glob.shape[1] if glob is not None else 0)
    return F.plain(verts, bounds, glob, torch.eye(ctot, dtype=verts.dtype), venc, maps)


def reference(case, dtype=torch.float64, wanted=('verts', 'glob', 'maps')):
    """(x, dverts, dglob | None, [dmap]) of the restatement in `dtype`, loss = (x * R).sum()."""
    def leaf(t, on):                                        # a copy: the case's own tensors stay as they are
        return t.to(dtype, copy=True).requires_grad_(on)

    v = leaf(case['verts'], 'verts' in wanted)
    g = leaf(case['glob'], 'glob' in wanted) if case['glob'] is not None else None
    mp = [leaf(m, 'maps' in wanted) for m in case['maps']]
    x = row(v, case['bounds'].to(dtype), g, case['venc'], mp)
    (x * case['R'].to(dtype)).sum().backward()
    return x.detach(), v.grad, g.grad if g is not None else None, [m.grad for m in mp]


def reference_without_extent_term(case):
    """dverts in float64 with the four extents held constant: the direct terms only."""
    v = case['verts'].double().requires_grad_(True)
    frozen = v.detach()
    zmax, zmin = frozen[..., 2].max(1, keepdim=True)[0], frozen[..., 2].min(1, keepdim=True)[0]
    ymax, ymin = frozen[..., 1].max(1, keepdim=True)[0], frozen[..., 1].min(1, keepdim=True)[0]
    b = case['bounds'].double()[:, None, :]
    gx = b[..., 0] + (1 - (v[..., 2] - zmin) / (zmax - zmin)) * (b[..., 1] - b[..., 0])
    gy = b[..., 2] + (1 - (v[..., 1] - ymin) / (ymax - ymin)) * (b[..., 3] - b[..., 2])
    grid = torch.stack([gx, gy], -1)[:, None]
    pooled = [torch.nn.functional.grid_sample(m.double(), grid, align_corners=True) for m in case['maps']]
    parts = [F._encoding(v, case['venc']), torch.cat(pooled, 1)[:, :, 0].permute(0, 2, 1)]
    if case['glob'] is not None:
        parts.append(case['glob'].double()[:, None, :].expand(-1, v.shape[1], -1))
    (torch.cat(parts, 2) * case['R'].double()).sum().backward()
    return v.grad


def split_errors(dv, dv64, case):
    """(elem_rel_err over the other unmasked rows O, over the extent rows E), each against its own largest component."""
    from conftest import elem_rel_err
    E = case['extent']
    O = ~E & ~case['masked']
    return elem_rel_err(dv[O], dv64[O]), elem_rel_err(dv[E], dv64[E])


def split_bar(own):
    """test_gpu_parity._raster_case's bar for small components: 1e-3, or 4 x the fp32 restatement's own error."""
    return max(1e-3, 4 * own)


# ---- aggregation edge cases

def irregular_mesh():
    """(faces, n): 9 vertices; vertex 8 is in no face, face (0, 1, 2) comes twice (once rotated), (3, 3, 4) is degenerate."""
    return torch.tensor([[0, 1, 2], [1, 2, 0], [0, 1, 2], [2, 3, 5], [3, 3, 4], [4, 5, 6], [6, 7, 0], [5, 6, 7]]), 9


def random_mesh(n, faces, seed):
    return torch.randint(0, n, (faces, 3), generator=torch.Generator().manual_seed(seed)), n


# ---- bounds cases

BOUNDS_SHAPES = [(1, 1, 1), (3, 7, 1030), (4, 33, 31), (3, 128, 128)]
BOUNDS_KINDS = ['empty', 'full', 'column0', 'row0', 'last_pixel', 'random']


def _spread(total, C):
    """`total` / 256 over C channels, in multiples of 1 / 256: the channel sum is exact in any order."""
    return torch.tensor([total // C + (1 if c < total % C else 0) for c in range(C)], dtype=torch.float32) / 256


def bounds_images(C, H, W):
    """(imgs [6,C,H,W], lit only [6,C,H,W]): lit pixels sum to 8/256 > 0.03 over the channels; imgs also has dim pixels of
    7/256 scattered over a tenth of the unlit ones, which may move no bound."""
    gen = torch.Generator().manual_seed(C * 1000003 + H * 1009 + W)
    lit = torch.zeros(6, H, W, dtype=torch.bool)
    lit[1] = True
    lit[2, :, 0] = True
    lit[3, 0, :] = True
    lit[4, H - 1, W - 1] = True
    lit[5] = torch.rand(H, W, generator=gen) < 0.01
    dim = (torch.rand(6, H, W, generator=gen) < 0.1) & ~lit
    only = lit[:, None].float() * _spread(8, C)[None, :, None, None]
    return only + dim[:, None].float() * _spread(7, C)[None, :, None, None], only
