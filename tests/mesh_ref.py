"""The triangle-mesh path (csrc/mesh.hip) for its domain tests: float64 statements of what the raster's
tile cull may drop and of which face the sampler must name, the case builders that put faces, cameras, shapes and indices
where the kernels branch, and the bars.  Plain torch on the CPU.

Reference.  oracle/vpn_oracle.py is dtype-generic: the reference of a test is that oracle on the fp32 inputs cast up to
float64, autograd for the gradients.  `face_terms` restates its per-face coverage (the oracle returns only the union);
test_mesh_domain_cpu.py shows that the restated terms give the oracle's alpha bit for bit.

Cull.  mesh.hip's stage_faces drops a (tile, face) pair when the face's box, inflated by the reach sqrt(16 sigma), misses
the tile's NDC rectangle.  A pixel centre of that tile is then at least the reach away from the face: d2 >= 16 sigma and
a_f <= sigmoid(-16) = 1.1254e-7 < CULL_A.  Dropping n such faces changes alpha = 1 - prod(1 - a) by at most n * CULL_A:
the forward bar of a pixel is ALPHA_BAR + n_culled(its tile) * CULL_A, so a cull that drops more fails where it happened.

Measures.  Norm-wise rel_err with the widening of test_mesh_path.py (`norm_bar`), and conftest.elem_rel_err per sample,
which holds every vertex to its own size (floor 1e-2 of the sample's largest component): the kernel may be ELEM_MARGIN times
as far from float64 as the fp32 oracle on the same case, never needing to be below ELEM_FLOOR (`elem_bar`)."""
import collections
import functools
import math

import numpy as np
import torch

from conftest import elem_rel_err, rel_err
from oracle import vpn_oracle as O

TILE = 16                      # R_TW = R_TH of vpn_raster_common.h
X_CUT = 16.0                   # MR_X_CUT: the box of a face is inflated by sqrt(X_CUT sigma)
CULL_A = 1.2e-7                # what a culled face may cover at a pixel centre: sigmoid(-16) = 1.1254e-7
ALPHA_BAR = 2e-5               # the project's forward bar (tests/test_mesh_path.py)
NORM_BAR = 1e-4                # the project's fp32 bar on a whole gradient
ELEM_MARGIN, ELEM_FLOOR = 4.0, 1e-4      # tests/test_trunknorm.py::hold's margin: __expf and v_rcp where the oracle divides
SAMPLE_ULPS = 4.0              # a draw this close (in ulp32 of the total area) to a prefix sum may name either neighbour:
#                                kernel and statement round their prefix sum to fp32 once each (0.5 ulp each), the target is
#                                one fp32 product (0.5 ulp of a number <= total), the areas' own fp32 error does not grow in
#                                an fp64 sum (<= 1 ulp of the total for well-shaped faces): 2.5 ulp, rounded up to a power of 2
SAMPLE_CAP = 1e-3              # share of a case's draws that may differ from the statement (tests/test_mesh_path.py)
POINT_BAR = 1e-6
SAMPLE_GRAD_BAR = 1e-5
CAMS = ((1.0, 0.0, 0.0), (1.6, -35.0, 250.0), (0.8, 60.0, 95.0))
TH = math.tan(0.5 * O.FOVY_DEG * math.pi / 180)

Case = collections.namedtuple('Case', 'name verts faces cam H W sigma meta')
SampleCase = collections.namedtuple('SampleCase', 'name verts faces u n meta')
Statement = collections.namedtuple('Statement', 'face dist alt alt_dist')


def norm_bar(e_cpu):
    """test_mesh_raster_vs_oracle's bar: 1e-4 against float64; the fp32 oracle's own distance widens it only when it is
    itself beyond 5e-5, and never past 3e-4."""
    return NORM_BAR if e_cpu <= 0.5 * NORM_BAR else min(2 * e_cpu, 3e-4)


def elem_bar(e_cpu):
    return max(ELEM_MARGIN * e_cpu, ELEM_FLOOR)


def grad_errors(got, ref64):
    """(norm-wise error of the whole gradient, [B] element-wise errors per sample)."""
    return rel_err(got, ref64), [elem_rel_err(got[b], ref64[b]) for b in range(ref64.shape[0])]


def clamp_faces(faces, P):
    """What the kernels do to a vertex index: clamped to [0, P - 1]."""
    return faces.long().clamp(0, P - 1)


# ------------------------------------------------------------------------------------------------ per-face terms, cull
def face_terms(verts, faces, cam, H, W, sigma):
    """oracle.mesh_raster's per-face coverage a [B,F,HW] (0 for a face that is not drawn), the mask of drawn faces [B,F]
    and the projected corners [B,F,3,3], in the dtype of `verts`: the oracle's own lines up to the union."""
    dt = verts.dtype
    pr = O.mesh_project(verts, cam)
    px, py = O.pixel_grid(H, W, dt)
    gx = (px / TH)[None, :].expand(H, W).reshape(-1)
    gy = (py / TH)[:, None].expand(H, W).reshape(-1)
    tri = pr[:, faces.long(), :]
    ok = (tri[..., 2] > O.MESH_NEAR).all(-1)
    ax, ay = tri[:, :, 0, 0], tri[:, :, 0, 1]
    bx, by = tri[:, :, 1, 0], tri[:, :, 1, 1]
    cx, cy = tri[:, :, 2, 0], tri[:, :, 2, 1]

    def seg_d2(x0, y0, x1, y1):
        ex, ey = (x1 - x0)[..., None], (y1 - y0)[..., None]
        wx, wy = gx[None, None, :] - x0[..., None], gy[None, None, :] - y0[..., None]
        t = ((wx * ex + wy * ey) / (ex * ex + ey * ey).clamp_min(1e-20)).clamp(0.0, 1.0)
        qx, qy = wx - t * ex, wy - t * ey
        return qx * qx + qy * qy

    def edge(x0, y0, x1, y1):
        return (x1 - x0)[..., None] * (gy[None, None, :] - y0[..., None]) - (y1 - y0)[..., None] * (gx[None, None, :] - x0[..., None])
    d2 = torch.minimum(torch.minimum(seg_d2(ax, ay, bx, by), seg_d2(bx, by, cx, cy)), seg_d2(cx, cy, ax, ay))
    e0, e1, e2 = edge(ax, ay, bx, by), edge(bx, by, cx, cy), edge(cx, cy, ax, ay)
    inside = (((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))) & (((e0 + e1) + e2).abs() > O.MESH_MIN_AREA2)
    a = torch.sigmoid((torch.where(inside, d2, -d2) / sigma).clamp(-80.0, 80.0))
    return torch.where(ok[..., None], a, torch.zeros_like(a)), ok, tri


def union(a):
    """alpha [B,HW] of per-face terms [B,F,HW], as the oracle forms it."""
    return 1.0 - torch.prod(1.0 - a, dim=1)


def tile_grid(H, W):
    return (H + TILE - 1) // TILE, (W + TILE - 1) // TILE


def tile_rects(H, W):
    """mesh_tile's NDC rectangles in float64: x0, x1 [tiles_x], y0, y1 [tiles_y] (y1 is the upper side: row r0)."""
    ty, tx = tile_grid(H, W)
    c0 = torch.arange(tx, dtype=torch.float64) * TILE
    r0 = torch.arange(ty, dtype=torch.float64) * TILE
    ar = W / H
    return (2 * c0 / W - 1) * ar, (2 * (c0 + TILE) / W - 1) * ar, 1 - 2 * (r0 + TILE) / H, 1 - 2 * r0 / H


def tile_of_pixels(H, W):
    """[HW] flat tile index (ty * tiles_x + tx) of every pixel."""
    _, tx = tile_grid(H, W)
    r, c = torch.arange(H)[:, None] // TILE, torch.arange(W)[None, :] // TILE
    return (r * tx + c).reshape(-1)


def cull_table(verts64, faces, cam64, H, W, sigma):
    """stage_faces' rule in float64.  kept [B,tiles_y,tiles_x,F]: every corner past MESH_NEAR and the box inflated by
    sqrt(16 sigma) meets the tile's rectangle (both closed, as the kernel compares).  n_culled [B,tiles_y,tiles_x]: the
    DRAWN faces the tile drops.  a_culled [B,tiles_y,tiles_x]: the largest a_f any of them has at a pixel centre of the tile."""
    assert verts64.dtype == torch.float64
    a, ok, tri = face_terms(verts64, faces, cam64, H, W, sigma)
    reach = math.sqrt(X_CUT * sigma)
    x0, x1 = tri[..., 0].min(-1).values - reach, tri[..., 0].max(-1).values + reach           # [B,F]
    y0, y1 = tri[..., 1].min(-1).values - reach, tri[..., 1].max(-1).values + reach
    tx0, tx1, ty0, ty1 = tile_rects(H, W)
    hx = (x0[:, None, :] <= tx1[None, :, None]) & (x1[:, None, :] >= tx0[None, :, None])    # [B,tiles_x,F]
    hy = (y0[:, None, :] <= ty1[None, :, None]) & (y1[:, None, :] >= ty0[None, :, None])    # [B,tiles_y,F]
    kept = ok[:, None, None, :] & hy[:, :, None, :] & hx[:, None, :, :]
    culled = ok[:, None, None, :] & ~kept
    nty, ntx = tile_grid(H, W)
    tp = tile_of_pixels(H, W)
    a_culled = torch.zeros(verts64.shape[0], nty * ntx, dtype=torch.float64)
    for t in range(nty * ntx):
        sel = a[:, :, tp == t].amax(-1)                                                     # [B,F]
        a_culled[:, t] = torch.where(culled.reshape(-1, nty * ntx, culled.shape[-1])[:, t], sel, torch.zeros_like(sel)).amax(-1)
    return kept, culled.sum(-1), a_culled.reshape(-1, nty, ntx)


def per_pixel(tile_values, H, W):
    """[B,tiles_y,tiles_x] -> [B,H,W]: every pixel gets its tile's value."""
    return tile_values.repeat_interleave(TILE, 1).repeat_interleave(TILE, 2)[:, :H, :W]


# ------------------------------------------------------------------------------------------------ placing geometry
def unproject(ndc_x, ndc_y, z, camrow):
    """World point (float64) that O.mesh_project sends to (ndc_x, ndc_y) at depth z under the camera row."""
    eye, right, up, fwd = (t[0] for t in O.camera_basis(torch.tensor([camrow], dtype=torch.float64), torch.float64))
    ndc_x, ndc_y, z = (torch.as_tensor(t, dtype=torch.float64) for t in (ndc_x, ndc_y, z))
    return eye + (ndc_x * z * TH)[..., None] * right + (ndc_y * z * TH)[..., None] * up + z[..., None] * fwd


def camera_point(xc, yc, zc, camrow):
    """World point (float64) with camera-space coordinates (xc, yc, zc)."""
    eye, right, up, fwd = (t[0] for t in O.camera_basis(torch.tensor([camrow], dtype=torch.float64), torch.float64))
    return eye + xc * right + yc * up + zc * fwd


def _cams(rows):
    return torch.tensor(rows, dtype=torch.float32)


def walk_mesh(gen, P, F, step=0.07, half=0.3):
    """P vertices of a random walk folded into the cube of half-width `half`, F faces of three consecutive vertices
    (a few skip one, so that the areas spread): faces ~ step wide, scattered over the cube, no repeated index when P >= 5."""
    x = torch.cumsum(step * torch.randn(P, 3, generator=gen, dtype=torch.float64), 0)
    x = (torch.remainder(x + half, 4 * half) - 2 * half).abs() - half                       # triangle wave: reflect at the walls
    i = torch.randint(0, P, (F,), generator=gen)
    k = torch.randint(1, 3, (F, 2), generator=gen)
    faces = torch.stack([i, (i + k[:, 0]) % P, (i + k[:, 0] + k[:, 1]) % P], 1) if P >= 5 else torch.stack([i, (i + 1) % P, (i + 2) % P], 1)
    return x.float(), faces


SIDES = ('left', 'right', 'top', 'bottom', 'top_left', 'top_right', 'bottom_left', 'bottom_right')
BORDER_SIGMAS = (1e-2, 1e-3, 1e-4)
BORDER_DELTAS = (1e-4, 1e-2)
BORDER_TILE = (1, 1)           # (ty, tx) of the interior tile of the 4 x 4: x in [-0.5, 0], y in [0, 0.5]


@functools.lru_cache(maxsize=None)
def border_faces(side, sigma):
    """64 x 64 (4 x 4 tiles, 0.5 NDC each), B = 3 under the three cameras; four faces ~0.05 NDC wide whose inflated box ends
    delta INSIDE (kept, faces 0 and 2) or delta OUTSIDE (culled, faces 1 and 3) the named side or corner of BORDER_TILE,
    delta = 1e-4 (faces 0, 1) and 1e-2 (faces 2, 3).  Placed by inverting each camera's projection in float64, at depths
    around the look-at point.  meta: tile, inside (face numbers), outside."""
    H = W = 64
    gen = torch.Generator().manual_seed(4100 + SIDES.index(side) * 10 + BORDER_SIGMAS.index(sigma))
    reach, s = math.sqrt(X_CUT * sigma), 0.05
    tx0, tx1, ty0, ty1 = (float(t[BORDER_TILE[1 if i < 2 else 0]]) for i, t in enumerate(tile_rects(H, W)))
    boxes = []                                                          # (xmin, ymin) of each face's own box
    for j, (delta, sign) in enumerate((d, sg) for d in BORDER_DELTAS for sg in (+1, -1)):      # sign +1: overlap by delta
        along = 0.06 + 0.09 * j                                         # spread along the side, so that no two faces coincide
        if 'left' in side:
            xmin = tx0 + sign * delta - reach - s                       # box's right end = tx0 + sign delta
        elif 'right' in side:
            xmin = tx1 - sign * delta + reach
        else:
            xmin = tx0 + along
        if 'top' in side:
            ymin = ty1 - sign * delta + reach
        elif 'bottom' in side:
            ymin = ty0 + sign * delta - reach - s
        else:
            ymin = ty0 + along
        boxes.append((xmin, ymin))
    verts = torch.zeros(3, 12, 3, dtype=torch.float64)
    for j, (xmin, ymin) in enumerate(boxes):
        # a scalene triangle that touches all four sides of the square (no pixel centre on a bisector, where the nearest
        # edge -- and with it the vertex that gets the gradient -- is a coin flip), mirrored at random
        beta, gamma = (0.2 + 0.6 * torch.rand(2, generator=gen, dtype=torch.float64)).tolist()
        mx, my = (torch.rand(2, generator=gen) < 0.5).tolist()
        pts = [(0.0, 0.0), (1.0, beta), (gamma, 1.0)]
        pts = [(xmin + s * (1 - p if mx else p), ymin + s * (1 - q if my else q)) for p, q in pts]
        for b, camrow in enumerate(CAMS):
            z = camrow[0] * (0.9 + 0.2 * torch.rand(3, generator=gen, dtype=torch.float64))
            verts[b, 3 * j:3 * j + 3] = unproject([p[0] for p in pts], [p[1] for p in pts], z, camrow)
    faces = torch.arange(12).reshape(4, 3)
    return Case('border_%s_%g' % (side, sigma), verts.float(), faces, _cams(CAMS), H, W, sigma,
                dict(tile=BORDER_TILE, inside=(0, 2), outside=(1, 3)))


SHAPES = (  # H, W, F, P, sigma: every H x W, F and P of the list at least once
    (1, 1, 1, 3, 1e-2), (16, 17, 63, 255, 1e-3), (17, 16, 64, 256, 1e-4), (15, 33, 65, 257, 1e-3),
    (56, 40, 128, 255, 1e-4), (40, 56, 129, 257, 1e-3), (1, 1, 129, 256, 1e-3), (16, 17, 1, 3, 1e-4),
    (17, 16, 129, 3, 1e-2), (15, 33, 128, 256, 1e-2), (56, 40, 65, 257, 1e-4), (40, 56, 63, 3, 1e-3))


@functools.lru_cache(maxsize=None)
def shapes():
    """A dozen (H x W, F, P) combinations, B = 3 with three different vertex sets under the three cameras."""
    out = []
    for i, (H, W, F, P, sigma) in enumerate(SHAPES):
        gen = torch.Generator().manual_seed(4200 + i)
        if P == 3:                                                      # one triangle (and its permutations, F times)
            v = torch.stack([0.5 * (torch.rand(3, 3, generator=gen) - 0.5) for _ in range(3)])
            f = torch.stack([torch.randperm(3, generator=gen) for _ in range(F)])
        else:
            vf = [walk_mesh(gen, P, F) for _ in range(3)]
            v, f = torch.stack([x[0] for x in vf]), vf[0][1]
        out.append(Case('shape_%dx%d_F%d_P%d' % (H, W, F, P), v, f, _cams(CAMS), H, W, sigma, {}))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def three_cameras(sigma=1e-4):
    """The largest case: 64 x 64, 129 faces, P = 40, B = 3 under the three cameras."""
    gen = torch.Generator().manual_seed(4300)
    vf = [walk_mesh(gen, 40, 129) for _ in range(3)]
    return Case('three_cameras_%g' % sigma, torch.stack([x[0] for x in vf]), vf[0][1], _cams(CAMS), 64, 64, sigma, {})


@functools.lru_cache(maxsize=None)
def near_plane():
    """Face 0 straddles the near plane (vertex 2 at z_c = 0.5 MESH_NEAR), face 1 is drawn with vertex 5 at 1.5 MESH_NEAR,
    face 2 lies behind the eye, face 3 is drawn and shares vertices 0 and 1 with face 0.  meta: drawn (faces), dead
    (vertices of undrawn faces only), shared."""
    cam = CAMS[0]
    n = O.MESH_NEAR
    v = torch.stack([unproject(-0.30, -0.10, 1.00, cam), unproject(0.25, -0.15, 1.05, cam), camera_point(0.0, 2e-4, 0.5 * n, cam),
                     unproject(-0.50, 0.20, 0.95, cam), unproject(-0.10, 0.30, 1.00, cam), unproject(-0.30, 0.60, 1.5 * n, cam),
                     camera_point(-0.1, 0.0, -0.5, cam), camera_point(0.1, 0.0, -0.5, cam), camera_point(0.0, 0.1, -0.4, cam),
                     unproject(0.05, -0.55, 0.90, cam)])
    f = torch.tensor([[0, 1, 2], [3, 4, 5], [6, 7, 8], [0, 1, 9]])
    return Case('near_plane', v.float()[None], f, _cams(CAMS[:1]), 48, 48, 1e-3,
                dict(drawn=(1, 3), dead=(2, 6, 7, 8), shared=(0, 1)))


@functools.lru_cache(maxsize=None)
def fan(valence=200):
    """`valence` thin faces around one apex vertex (vertex 0): that many atomic adds per tile land on its two addresses."""
    cam = CAMS[1]
    gen = torch.Generator().manual_seed(4400)
    ang = torch.arange(valence, dtype=torch.float64) * (2 * math.pi / valence)
    rim = unproject(0.05 + 0.55 * torch.cos(ang), -0.03 + 0.5 * torch.sin(ang),
                    cam[0] * (0.95 + 0.1 * torch.rand(valence, generator=gen, dtype=torch.float64)), cam)
    v = torch.cat([unproject(0.05, -0.03, cam[0], cam)[None], rim])
    i = torch.arange(valence)
    f = torch.stack([torch.zeros_like(i), 1 + i, 1 + (i + 1) % valence], 1)
    return Case('fan_%d' % valence, v.float()[None], f, _cams([cam]), 32, 32, 1e-3, dict(apex=0))


@functools.lru_cache(maxsize=None)
def stack(copies=40):
    """`copies` coincident copies (corner order rotated) of one face that covers a quarter of the 48 x 48 image: deep inside
    it 1 - alpha = prod (1 - a) falls below 2^-25 and the stored alpha is 1."""
    cam = CAMS[0]
    v = unproject([-0.72, 0.70, -0.69], [-0.71, -0.68, 0.73], [1.0, 1.02, 0.97], cam)      # legs ~ sqrt 2: area 1 of the image's 4
    f = torch.tensor([[(j + k) % 3 for k in range(3)] for j in range(copies)])
    return Case('stack_%d' % copies, v.float()[None], f, _cams([cam]), 48, 48, 1e-3, {})


BAD = (-1, -2 ** 31, None, 'P+5', 2 ** 31 - 1)                          # None: P itself


@functools.lru_cache(maxsize=None)
def bad_indices():
    """B = 2 with different vertices per sample; the faces hold -1, -2^31, P, P + 5 and 2^31 - 1 next to good indices.
    The statement is the oracle on clamp_faces(faces, P)."""
    gen = torch.Generator().manual_seed(4500)
    P = 10
    v = torch.stack([walk_mesh(gen, P, 1, step=0.2)[0] for _ in range(2)])
    f = torch.tensor([[0, 1, 2], [-1, 4, 5], [3, -2 ** 31, 6], [7, 8, P], [P + 5, 2, 5], [1, 2 ** 31 - 1, 4], [-1, P, 3], [6, 7, 8]])
    return Case('bad_indices', v, f, _cams(CAMS[1:]), 32, 32, 1e-3, dict(P=P))


def raster_cases():
    """Every raster case, in a fixed order."""
    return (tuple(border_faces(s, g) for s in SIDES for g in BORDER_SIGMAS) + shapes() + tuple(three_cameras(g) for g in BORDER_SIGMAS) +
            (near_plane(), fan(), stack(), bad_indices()))


def case_by_name(name):
    return next(c for c in raster_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def raster_reference(name, seed=0):
    """For the named case and random upstream weights Wt [B,H,W] (seeded): dict of Wt and, for fp32 and fp64, the oracle's
    alpha and vertex gradient on the clamped faces; n_culled per pixel.  Computed once, shared, never written to."""
    c = case_by_name(name)
    gen = torch.Generator().manual_seed(5000 + seed)
    B, P = c.verts.shape[:2]
    Wt = torch.randn(B, c.H, c.W, generator=gen)
    f = clamp_faces(c.faces, P)
    out = dict(Wt=Wt, faces=f)
    for dt in (torch.float32, torch.float64):
        v = c.verts.to(dt).clone().requires_grad_(True)
        a = O.mesh_raster(v, f, c.cam.to(dt), c.H, c.W, c.sigma)
        (a * Wt.to(dt)).sum().backward()
        out[dt] = (a.detach(), v.grad)
    _, n_culled, _ = cull_table(c.verts.double(), f, c.cam.double(), c.H, c.W, c.sigma)
    out['n_culled'] = per_pixel(n_culled, c.H, c.W)
    return out


def kept_alpha(verts, faces, cam, H, W, sigma, kept):
    """alpha [B,H,W] of the faces each pixel's tile keeps (kept: cull_table's), in the dtype of `verts`."""
    a, _, _ = face_terms(verts, faces, cam, H, W, sigma)
    B, Fn = a.shape[:2]
    mask = kept.reshape(B, -1, Fn)[:, tile_of_pixels(H, W), :].transpose(1, 2)
    return union(torch.where(mask, a, torch.zeros_like(a))).reshape(B, H, W)


TILE_CASES = ('border_top_left_0.01', 'border_right_0.001', 'border_bottom_0.0001', 'three_cameras_0.0001')


@functools.lru_cache(maxsize=None)
def tile_reference(name, seed=1):
    """Upstream weights that live on ONE tile at a time: Wt [B,H,W] and, per tile t (flat index), the fp32 and fp64
    gradients [T,B,P,3] from one forward each.  The statement here is the union of the faces the tile KEEPS (cull_table in
    float64, used as it is for the fp32 figure): against the full union, a tile all of whose faces are culled has a gradient
    ~1e-7 of its neighbours' where the kernel by design returns exactly 0 -- a 100 % element-wise error in a quantity the
    forward bar already allows (test_what_the_cull_drops_is_below_its_bound).  Here such a tile must give exactly 0."""
    c = case_by_name(name)
    gen = torch.Generator().manual_seed(5000 + seed)
    B, P = c.verts.shape[:2]
    Wt = torch.randn(B, c.H, c.W, generator=gen)
    tp = tile_of_pixels(c.H, c.W).reshape(c.H, c.W)
    f = clamp_faces(c.faces, P)
    kept, _, _ = cull_table(c.verts.double(), f, c.cam.double(), c.H, c.W, c.sigma)
    out = dict(Wt=Wt, tiles=int(tp.max()) + 1, tile_of_pixel=tp, kept=kept)
    for dt in (torch.float32, torch.float64):
        v = c.verts.to(dt).clone().requires_grad_(True)
        a = kept_alpha(v, f, c.cam.to(dt), c.H, c.W, c.sigma, kept)
        out[dt] = torch.stack([torch.autograd.grad((a * (Wt * (tp == t)).to(dt)).sum(), v, retain_graph=True)[0] for t in range(out['tiles'])])
    return out


# ------------------------------------------------------------------------------------------------ sampler
def ulp32(x):
    return float(np.spacing(np.float32(x)))


def sample_statement(verts64, faces, u):
    """The face-choice rule in float64 for one mesh: verts64 (P,3), faces (F,3) with valid indices, u (n,3).
    face (n,): the first face whose inclusive cumulative area exceeds u0 * total, the last face when none does.
    dist (n,): distance of u0 * total to the nearest prefix sum, in ulp32(total) (0 when the total is 0).
    alt (n,2): the faces of non-zero area that meet the statement's face at its lower / upper prefix sum (-1: none),
    alt_dist (n,2): the distance of the target to that prefix sum in the same unit."""
    assert verts64.dtype == torch.float64
    f = faces.long()
    a, b, c = verts64[f[:, 0]], verts64[f[:, 1]], verts64[f[:, 2]]
    area = 0.5 * torch.cross(b - a, c - a, dim=1).norm(dim=1)
    cum = torch.cumsum(area, 0)
    total = cum[-1]
    F, n = f.shape[0], u.shape[0]
    target = u[:, 0].double() * total
    face = torch.searchsorted(cum, target, right=True).clamp_max(F - 1)
    if float(total) == 0.0:
        return Statement(face, torch.zeros(n, dtype=torch.float64), torch.full((n, 2), -1), torch.full((n, 2), float('inf'), dtype=torch.float64))
    unit = ulp32(float(total))
    dist = (target[:, None] - cum[None, :]).abs().amin(1) / unit
    nz = torch.nonzero(area > 0)[:, 0]
    cnz = cum[nz]
    j = torch.searchsorted(cnz, target, right=True).clamp_max(nz.numel() - 1)
    assert torch.equal(nz[j], face)                                     # the rule never names a face of no area
    lower = torch.where(j > 0, cnz[(j - 1).clamp_min(0)], torch.zeros_like(target))
    alt = torch.stack([torch.where(j > 0, nz[(j - 1).clamp_min(0)], torch.full_like(j, -1)),
                       torch.where(j < nz.numel() - 1, nz[(j + 1).clamp_max(nz.numel() - 1)], torch.full_like(j, -1))], 1)
    alt_dist = torch.stack([(target - lower).abs(), (target - cnz[j]).abs()], 1) / unit
    return Statement(face, dist, alt, alt_dist)


def face_allowed(st, got):
    """(n,) bool: `got` is the statement's face, or the neighbour across a prefix sum within SAMPLE_ULPS of the target."""
    got = got.long()
    near = (st.alt_dist <= SAMPLE_ULPS) & (st.alt >= 0)
    return (got == st.face) | ((got[:, None] == st.alt) & near).any(1)


def bary_points(verts64, faces, face, u):
    """float64 points and barycentric weights of the square-root map for the given face choice."""
    f = faces.long()[face.long()]
    r = torch.sqrt(u[:, 1].double())
    w = torch.stack([1.0 - r, r * (1.0 - u[:, 2].double()), r * u[:, 2].double()], 1)
    return (w[:, :, None] * verts64[f]).sum(1), w


def bary_scatter(P, faces, face, w, g):
    """float64 gradient (P,3) of sum(points * g) w.r.t. the vertices for the given face choice."""
    f = faces.long()[face.long()]
    out = torch.zeros(P, 3, dtype=torch.float64)
    for k in range(3):
        out.index_add_(0, f[:, k], w[:, k:k + 1] * g.double())
    return out


U_EDGE = (0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24)
SAMPLE_N = 1000
SAMPLE_SEED, SAMPLE_BASE = 77, 5
COLLINEAR = ((0.0, 0.0, 0.0), (0.125, 0.25, 0.5), (0.25, 0.5, 1.0))     # exact in fp32 with exact products: area 0 in any precision


def _explicit_u(gen, n):
    u = torch.rand(n, 3, generator=gen)
    rows = [(a, b, c) for a in U_EDGE for b in (0.0, 1.0 - 2.0 ** -24) for c in (0.0, 1.0 - 2.0 ** -24)]
    u[:len(rows)] = torch.tensor(rows, dtype=torch.float32)
    return u


def _sample_mesh(gen, F, P=96):
    """A walk mesh of unequal areas with faces of no area planted at the head, in the middle (around face 1024 too when
    there is one) and at the tail: alternately a repeated index and three collinear corners (the last three vertices)."""
    v, f = walk_mesh(gen, P, F)
    v = v * (0.5 + torch.rand(P, 1, generator=gen))                      # spreads the areas further
    v = torch.cat([v, torch.tensor(COLLINEAR)])
    planted = []
    if F >= 16:
        planted = sorted({0, 1, F // 2, F // 2 + 1, F - 2, F - 1} | ({1022, 1023, 1024} if F > 1025 else set()))
        for k, i in enumerate(planted):
            f[i] = torch.tensor([P, P + 1, P + 2]) if k % 2 else torch.stack([f[i, 0], f[i, 0], f[i, 2]])
    return v, f, tuple(planted)


@functools.lru_cache(maxsize=None)
def sampler_meshes():
    """F in {1, 1023, 1024, 1025, 2049} (one, two and three chunks of mesh_cdf_kernel), an all-degenerate mesh and a B = 2
    batch with bad indices; explicit u [B,n,3] whose first 16 rows cross the edge values of u0, u1, u2.  meta: planted."""
    out = []
    for i, F in enumerate((1, 1023, 1024, 1025, 2049)):
        gen = torch.Generator().manual_seed(4600 + i)
        v, f, planted = _sample_mesh(gen, F)
        out.append(SampleCase('F%d' % F, v[None], f, _explicit_u(gen, SAMPLE_N)[None], SAMPLE_N, dict(planted=planted)))
    gen = torch.Generator().manual_seed(4610)
    v, f, _ = _sample_mesh(gen, 70)
    f = torch.stack([f[:, 0], f[:, 0], f[:, 2]], 1)
    f[::2] = torch.tensor([96, 97, 98])
    out.append(SampleCase('all_degenerate', v[None], f, _explicit_u(gen, SAMPLE_N)[None], SAMPLE_N, dict(planted=tuple(range(70)))))
    gen = torch.Generator().manual_seed(4611)
    va, f, planted = _sample_mesh(gen, 130)
    vb = _sample_mesh(gen, 130)[0]
    P = va.shape[0]
    f[3, 1], f[40, 0], f[60, 2], f[70, 0], f[100, 1] = -1, -2 ** 31, P, P + 5, 2 ** 31 - 1
    out.append(SampleCase('bad_indices_B2', torch.stack([va, vb]), f, torch.stack([_explicit_u(gen, SAMPLE_N) for _ in range(2)]),
                          SAMPLE_N, dict(planted=planted)))
    return tuple(out)


def sampler_uniforms(case, mode, b):
    """The draws of sample b: the case's explicit u, or the Philox stream the kernel uses for (SAMPLE_SEED, SAMPLE_BASE + b)."""
    return case.u[b] if mode == 'explicit' else O.philox_uniforms_mesh(SAMPLE_SEED, SAMPLE_BASE + b, case.n)


def sample_weights(case, b):
    """Upstream gradient (n,3) of sample b's points, all of one sign: a vertex of the one-face mesh sums 1000 terms, and with
    random signs that sum cancels until the fp32 oracle itself is 1.0e-5 from float64 element-wise (the whole bar); like-signed
    terms keep an fp32 sum good to ~sqrt(n) 2^-24 = 2e-6 in whatever order the atomics land."""
    return 0.5 + torch.rand(case.n, 3, generator=torch.Generator().manual_seed(4700 + b))
