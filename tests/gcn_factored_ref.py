"""conv1 of the GCN in factored form for the tests: the cases both test files share, and the two float64
statements of h = [encoding | pooled | global] Theta through tests/gcn_ref.py -- the plain one (the row, then the product)
and the factored one (project the maps and the global features, then pool the projected maps)."""
import torch

import gcn_ref as R

REAL_MAPS = [(64, 32), (128, 16), (256, 8), (512, 4)]
SMALL_MAPS = [(4, 32), (8, 16), (16, 8), (32, 4)]
# name -> (map shapes (C, H = W), G, Cout, venc, N, bounds given directly)
OP_CASES = {
    'small': (SMALL_MAPS, 16, 24, 39, 256, False),
    'real_channels': (REAL_MAPS, 512, 512, 39, 256, False),
    'venc3': (SMALL_MAPS, 16, 24, 3, 256, False),
    'venc0_no_global': (SMALL_MAPS, 0, 24, 0, 256, False),
    'no_maps': ([], 16, 24, 39, 256, False),
    'n200_two_levels': (SMALL_MAPS[:2], 16, 24, 39, 200, False),
    'corners_outside': (SMALL_MAPS, 16, 24, 39, 256, True),
}
WIDE_BOUNDS = [-1.3, 1.2, -0.9, 1.4]


def op_case(name):
    """dict(verts [2,N,3], bounds [2,4], glob [2,G] | None, weight [ctot,Cout], venc, maps, R [2,N,Cout]) in fp32."""
    from test_gcn import composed_sphere_vertices
    map_shapes, G, Cout, venc, N, wide = OP_CASES[name]
    gen = torch.Generator().manual_seed(1000 + sorted(OP_CASES).index(name))
    B = 2
    if wide:
        verts = torch.rand(B, N, 3, generator=gen) - 0.5
        bounds = torch.tensor([WIDE_BOUNDS] * B)
    else:
        verts = composed_sphere_vertices(B, 2, gen)[0][:, :N].contiguous()
        rgbs = torch.zeros(B, 3, 64, 64)
        for b in range(B):
            y0, x0 = int(torch.randint(1, 16, (1,), generator=gen)), int(torch.randint(1, 16, (1,), generator=gen))
            rgbs[b, :, y0:64 - y0, x0:64 - 2 * x0] = 0.5
        bounds = R.bounds(rgbs)
    assert verts.shape == (B, N, 3)
    maps = [torch.randn(B, c, s, s, generator=gen) for c, s in map_shapes]
    glob = torch.randn(B, G, generator=gen) if G else None
    ctot = venc + sum(c for c, _ in map_shapes) + G
    a = (6.0 / (ctot + Cout)) ** 0.5                         # glorot, as GCNConv initialises conv1
    weight = (torch.rand(ctot, Cout, generator=gen) * 2 - 1) * a
    return dict(verts=verts, bounds=bounds, glob=glob, weight=weight, venc=venc, maps=maps,
                R=torch.randn(B, N, Cout, generator=gen))


def _encoding(verts, venc):
    return R.positional_encoding(verts) if venc == 39 else verts[..., :venc]


def plain(verts, bounds, glob, weight, venc, maps):
    """cat(encoding, pooled, global) @ weight in the dtype of the inputs."""
    parts = [_encoding(verts, venc)]
    if maps:
        parts.append(R.pooling(maps, verts, bounds))
    if glob is not None:
        parts.append(glob[:, None, :].expand(-1, verts.shape[1], -1))
    return torch.cat(parts, 2) @ weight


def factored(verts, bounds, glob, weight, venc, maps):
    """The same product from the projected maps: enc Theta_e + sum_l pooled(P_l) + g Theta_g."""
    B, N, Cout = verts.shape[0], verts.shape[1], weight.shape[1]
    h = _encoding(verts, venc) @ weight[:venc]
    r = venc
    for m in maps:
        C, H, W = m.shape[1:]
        P = m.flatten(2).transpose(1, 2) @ weight[r:r + C]                      # [B, H W, Cout]
        h = h + R.pooling([P.transpose(1, 2).reshape(B, Cout, H, W)], verts, bounds)
        r += C
    if glob is not None:
        h = h + (glob @ weight[r:])[:, None, :]
    return h


def outside_fractions(verts, bounds, size):
    """(fraction of the vertices with a bilinear corner outside a size x size map, fraction with all four inside), from the
    float64 grid."""
    v = verts.double()
    zmax, zmin = v[..., 2].max(1, keepdim=True)[0], v[..., 2].min(1, keepdim=True)[0]
    ymax, ymin = v[..., 1].max(1, keepdim=True)[0], v[..., 1].min(1, keepdim=True)[0]
    b = bounds.double()[:, None, :]
    gx = b[..., 0] + (1 - (v[..., 2] - zmin) / (zmax - zmin)) * (b[..., 1] - b[..., 0])
    gy = b[..., 2] + (1 - (v[..., 1] - ymin) / (ymax - ymin)) * (b[..., 3] - b[..., 2])
    ix, iy = (gx + 1) / 2 * (size - 1), (gy + 1) / 2 * (size - 1)
    inside = (ix >= 0) & (ix <= size - 1) & (iy >= 0) & (iy <= size - 1)
    return float((~inside).double().mean()), float(inside.double().mean())


def float64_reference(case):
    """(h, dverts, dweight, dglob | None, [dmap]) of the plain form in float64, loss = (h * R).sum()."""
    v = case['verts'].double().requires_grad_(True)
    w = case['weight'].double().requires_grad_(True)
    g = case['glob'].double().requires_grad_(True) if case['glob'] is not None else None
    mp = [m.double().requires_grad_(True) for m in case['maps']]
    h = plain(v, case['bounds'].double(), g, w, case['venc'], mp)
    (h * case['R'].double()).sum().backward()
    return h.detach(), v.grad, w.grad, g.grad if g is not None else None, [m.grad for m in mp]
