"""tests/mesh_ref.py does what tests/test_mesh_domain.py relies on (no GPU): the restated per-face terms are the oracle's,
every builder puts its faces, corners and indices where it says, what the cull rule drops is below CULL_A, the fp32 oracle
sits within half of every fixed bar on every case, and oracle.mesh_sample agrees with the float64 face-choice statement
except next to a prefix sum."""
import math

import pytest
import torch

import mesh_ref as M
from oracle import vpn_oracle as O

F64 = torch.float64


def _c64(c):
    return c.verts.double(), M.clamp_faces(c.faces, c.verts.shape[1]), c.cam.double()


# ------------------------------------------------------------------------------------------------ per-face terms
@pytest.mark.parametrize('name', ['border_top_left_0.001', 'shape_15x33_F65_P257', 'shape_1x1_F1_P3', 'near_plane', 'stack_40',
                                  'bad_indices'])
def test_face_terms_are_the_oracles(name):
    """1 - prod(1 - a) of the restated terms is oracle.mesh_raster's alpha bit for bit in float64 (and in fp32)."""
    c = M.case_by_name(name)
    v, f, cam = _c64(c)
    for dt in (F64, torch.float32):
        a, ok, _ = M.face_terms(v.to(dt), f, cam.to(dt), c.H, c.W, c.sigma)
        assert torch.equal(M.union(a).reshape(-1, c.H, c.W), O.mesh_raster(v.to(dt), f, cam.to(dt), c.H, c.W, c.sigma))
        assert a.shape == (v.shape[0], f.shape[0], c.H * c.W) and bool((a[~ok] == 0).all())


def test_cull_constant_is_the_coverage_at_the_reach():
    """MR_X_CUT = 16 <-> 'coverage < 1.2e-7': at the reach sqrt(16 sigma) the logit is -16."""
    assert abs(1 / (1 + math.exp(16.0)) - 1.1254e-7) < 1e-11 and 1 / (1 + math.exp(M.X_CUT)) < M.CULL_A
    assert 1 / (1 + math.exp(M.X_CUT - 0.1)) > M.CULL_A                # and no looser: a reach 0.3 % shorter would break it
    assert (M.TILE, M.X_CUT) == (16, 16.0)


# ------------------------------------------------------------------------------------------------ cull
@pytest.mark.parametrize('sigma', M.BORDER_SIGMAS)
@pytest.mark.parametrize('side', M.SIDES)
def test_border_faces_sit_on_their_side(side, sigma):
    """The target tile keeps faces 0 and 2 and drops faces 1 and 3 (all four drawn) in all three samples; every box ends
    delta from the named side(s) of the tile."""
    c = M.border_faces(side, sigma)
    v, f, cam = _c64(c)
    kept, n_culled, a_culled = M.cull_table(v, f, cam, c.H, c.W, c.sigma)
    ty, tx = c.meta['tile']
    assert c.verts.shape == (3, 12, 3) and (c.H, c.W) == (64, 64) and kept.shape == (3, 4, 4, 4)
    assert bool(kept[:, ty, tx, list(c.meta['inside'])].all()) and not bool(kept[:, ty, tx, list(c.meta['outside'])].any())
    assert bool((n_culled[:, ty, tx] == 2).all())                       # dropped by the box, not by the near plane
    _, ok, tri = M.face_terms(v, f, cam, c.H, c.W, c.sigma)
    assert bool(ok.all())
    reach = math.sqrt(M.X_CUT * sigma)
    x0, x1, y0, y1 = (float(t[tx if i < 2 else ty]) for i, t in enumerate(M.tile_rects(c.H, c.W)))
    gaps = []                                                           # signed overlap of the inflated box with the tile, per named side
    if 'left' in side:
        gaps.append(tri[..., 0].amax(-1) + reach - x0)
    if 'right' in side:
        gaps.append(x1 - (tri[..., 0].amin(-1) - reach))
    if 'top' in side:
        gaps.append(y1 - (tri[..., 1].amin(-1) - reach))
    if 'bottom' in side:
        gaps.append(tri[..., 1].amax(-1) + reach - y0)
    want = torch.tensor([1e-4, -1e-4, 1e-2, -1e-2], dtype=F64)
    for g in gaps:                                                      # fp32 vertices: the placement is good to ~1e-6 NDC
        assert float((g - want).abs().max()) < 5e-6, g
    assert float((tri[..., :2].amax(-2) - tri[..., :2].amin(-2) - 0.05).abs().max()) < 1e-5     # ~0.05 NDC wide
    # the three samples hold DIFFERENT vertices (one projection, three cameras)
    assert float((c.verts[0] - c.verts[1]).norm(dim=1).min()) > 0.01 and float((c.verts[1] - c.verts[2]).norm(dim=1).min()) > 0.01


def _cases():
    return [c.name for c in M.raster_cases()]


@pytest.mark.parametrize('name', _cases())
def test_what_the_cull_drops_is_below_its_bound(name):
    """The largest a_f of a culled (tile, face) pair at a pixel centre of the tile is below CULL_A, and the float64 alpha
    of the kept faces alone differs from the full one by no more than n_culled(tile) * CULL_A at any pixel."""
    c = M.case_by_name(name)
    v, f, cam = _c64(c)
    kept, n_culled, a_culled = M.cull_table(v, f, cam, c.H, c.W, c.sigma)
    assert float(a_culled.max()) < M.CULL_A, float(a_culled.max())
    a, _, _ = M.face_terms(v, f, cam, c.H, c.W, c.sigma)
    B, Fn = a.shape[:2]
    tp = M.tile_of_pixels(c.H, c.W)
    mask = kept.reshape(B, -1, Fn)[:, tp, :].transpose(1, 2)            # [B,F,HW]: does the pixel's tile keep the face
    diff = (M.union(a) - M.union(torch.where(mask, a, torch.zeros_like(a)))).abs().reshape(B, c.H, c.W)
    assert bool((diff <= M.per_pixel(n_culled, c.H, c.W) * M.CULL_A + 1e-13).all())        # 1e-13: float64 rounding of two products
    assert torch.equal(M.per_pixel(n_culled, c.H, c.W), M.raster_reference(name)['n_culled'])


def test_culled_pairs_exist_where_the_reach_matters():
    """The cull is exercised, not vacuous: at 64 x 64 every sigma leaves tiles that drop drawn faces AND tiles that keep
    some, and the reach is 4/5, 1/4 and 1/12 of a tile."""
    for sigma, frac in zip(M.BORDER_SIGMAS, (0.8, 0.2530, 0.08)):
        assert abs(math.sqrt(M.X_CUT * sigma) / 0.5 - frac) < 1e-3
        c = M.three_cameras(sigma)
        kept, n_culled, _ = M.cull_table(*_c64(c), c.H, c.W, c.sigma)
        assert int(n_culled.max()) > 0 and int(kept.sum(-1).max()) > 64   # some tile walks two staged passes


# ------------------------------------------------------------------------------------------------ the other builders
def test_shapes_cover_the_lists():
    cs = M.shapes()
    assert len(cs) == 12
    assert {(c.H, c.W) for c in cs} == {(1, 1), (16, 17), (17, 16), (15, 33), (56, 40), (40, 56)}
    assert {c.faces.shape[0] for c in cs} == {1, 63, 64, 65, 128, 129}
    assert {c.verts.shape[1] for c in cs} == {3, 255, 256, 257}
    assert {c.sigma for c in cs} == set(M.BORDER_SIGMAS)
    for c in cs:
        assert c.verts.shape[0] == 3 and c.cam.tolist() == torch.tensor(M.CAMS).tolist() and c.verts.dtype == torch.float32
        assert int(c.faces.min()) >= 0 and int(c.faces.max()) < c.verts.shape[1]
        assert bool(M.face_terms(*_c64(c), c.H, c.W, c.sigma)[1].all())         # every face in front of every camera
    t = M.three_cameras()
    assert (t.H, t.W, t.faces.shape[0], t.verts.shape) == (64, 64, 129, (3, 40, 3))


def test_near_plane_case():
    c = M.near_plane()
    v, f, cam = _c64(c)
    z = O.mesh_project(v, cam)[0, :, 2]
    assert abs(float(z[2]) / O.MESH_NEAR - 0.5) < 1e-3 and abs(float(z[5]) / O.MESH_NEAR - 1.5) < 1e-3
    assert bool((z[6:9] < 0).all())
    _, ok, _ = M.face_terms(v, f, cam, c.H, c.W, c.sigma)
    assert ok[0].tolist() == [False, True, False, True] and c.meta['drawn'] == (1, 3)
    used = set(f[list(c.meta['drawn'])].reshape(-1).tolist())
    assert set(c.meta['dead']) == set(range(v.shape[1])) - used and set(c.meta['shared']) == set(f[0].tolist()) & set(f[3].tolist())
    r = M.raster_reference(c.name)
    assert float(r[F64][1][0, list(c.meta['dead'])].abs().max()) == 0.0
    assert float(r[F64][1][0, list(c.meta['shared'])].abs().min()) > 0.0
    # the undrawn faces add nothing: the drawn ones alone give the same alpha
    assert torch.equal(r[F64][0], O.mesh_raster(v, f[list(c.meta['drawn'])], cam, c.H, c.W, c.sigma))


def test_fan_and_stack_cases():
    c = M.fan()
    assert c.faces.shape[0] == 200 and int((c.faces == c.meta['apex']).sum()) == 200 and c.verts.shape[1] == 201
    a, _, _ = M.face_terms(*_c64(c), c.H, c.W, c.sigma)
    assert float((a > 0.05).sum(1).max()) >= 20                         # many faces matter at the apex's pixels
    c = M.stack()
    r = M.raster_reference(c.name)
    assert c.faces.shape[0] == 40 and bool((c.faces.sort(1).values == torch.arange(3)).all())
    sat = (1.0 - r[F64][0]) < 2.0 ** -25
    assert 0.2 < float(sat.float().mean()) < 0.3                        # about a quarter of the image
    # no pixel sits so close to 2^-25 that fp32 rounding of the product decides on which side it falls
    p = torch.prod(1.0 - M.face_terms(*_c64(c), c.H, c.W, c.sigma)[0], 1)
    assert float(((p / 2.0 ** -25) - 1).abs().min()) > 1e-2


def test_bad_indices_case():
    c = M.bad_indices()
    P = c.meta['P']
    assert c.verts.shape == (2, P, 3) and float((c.verts[0] - c.verts[1]).abs().min()) > 1e-4
    for bad in (-1, -2 ** 31, P, P + 5, 2 ** 31 - 1):
        assert int((c.faces == bad).sum()) >= 1
    assert torch.equal(c.faces.to(torch.int32).long(), c.faces)         # all of them fit the kernel's int32
    f = M.clamp_faces(c.faces, P)
    assert int(f.min()) == 0 and int(f.max()) == P - 1 and int((f != c.faces).sum()) == 7


# ------------------------------------------------------------------------------------------------ reference alone
@pytest.mark.parametrize('name', _cases())
def test_fp32_oracle_is_within_half_of_the_fixed_bars(name):
    """A bar must not be one the reference itself only just meets: the fp32 oracle's alpha is within ALPHA_BAR / 2 of
    float64 and its gradient within NORM_BAR / 2 (so norm_bar never widens on these cases)."""
    r = M.raster_reference(name)
    da = float((r[torch.float32][0] - r[F64][0]).abs().max())
    en, ee = M.grad_errors(r[torch.float32][1], r[F64][1])
    print('%-28s alpha %.2e  grad norm-wise %.2e  per sample element-wise %s' % (name, da, en, ' '.join('%.1e' % e for e in ee)))
    assert da <= 0.5 * M.ALPHA_BAR and en <= 0.5 * M.NORM_BAR
    assert M.norm_bar(en) == M.NORM_BAR


# ------------------------------------------------------------------------------------------------ sampler
def _per_mesh(case):
    P = case.verts.shape[1]
    for b in range(case.verts.shape[0]):
        yield b, case.verts[b], M.clamp_faces(case.faces, P)


def test_sampler_meshes_cover_the_list():
    cs = {c.name: c for c in M.sampler_meshes()}
    assert [cs['F%d' % F].faces.shape[0] for F in (1, 1023, 1024, 1025, 2049)] == [1, 1023, 1024, 1025, 2049]
    for c in cs.values():
        F, P = c.faces.shape[0], c.verts.shape[1]
        assert c.n == 1000 and c.u.shape == (c.verts.shape[0], 1000, 3) and float(c.u.max()) < 1.0
        rows = {tuple(r) for r in c.u[0, :16].tolist()}
        assert rows == {(a, b, d) for a in M.U_EDGE for b in (0.0, 1 - 2.0 ** -24) for d in (0.0, 1 - 2.0 ** -24)}
        for b, v, f in _per_mesh(c):
            tri = v.double()[f]
            area = 0.5 * torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1).norm(dim=1)
            planted = list(c.meta['planted'])
            assert bool((area[planted] == 0).all())
            if c.name == 'all_degenerate':
                assert float(area.max()) == 0.0 and planted == list(range(F))
            elif c.name.startswith('F') and F > 1:
                assert {0, F // 2, F - 1} <= set(planted) and float(area.max() / area[area > 0].min()) > 50     # unequal areas
                assert int((area == 0).sum()) == len(planted)
                kinds = [len(set(f[i].tolist())) for i in planted]
                assert 2 in kinds and 3 in kinds                        # repeated indices and collinear corners
        if F == 2049:
            assert {1023, 1024} <= set(c.meta['planted'])
    bad = cs['bad_indices_B2']
    assert bad.verts.shape[0] == 2 and int((bad.faces < 0).sum()) == 2 and int((bad.faces >= bad.verts.shape[1]).sum()) == 3


@pytest.mark.parametrize('mode', ['explicit', 'philox'])
def test_oracle_sampler_against_the_statement(mode):
    """oracle.mesh_sample names the statement's face except within SAMPLE_ULPS of a prefix sum, where it names the face on
    the other side; faces of no area are never named (the all-degenerate mesh: the last face); u0 = 1 - 2^-24 stays in
    range; the draws that differ stay within the cap (those that merely come that close to a prefix sum cannot: the 16
    planted rows sit on the first and last prefix sum on purpose, and of 1000 uniform draws over 2049 faces about 2 fall
    within 4 ulp by chance -- printed); points and gradient within half their bars."""
    for c in M.sampler_meshes():
        F = c.faces.shape[0]
        for b, v, f in _per_mesh(c):
            u = M.sampler_uniforms(c, mode, b)
            st = M.sample_statement(v.double(), f, u)
            vv = v.clone().requires_grad_(True)
            pts, idx = O.mesh_sample(vv, f, u)
            assert int(idx.min()) >= 0 and int(idx.max()) <= F - 1
            differ = idx != st.face
            chance = st.dist <= M.SAMPLE_ULPS
            if mode == 'explicit':
                chance[:16] = False                                     # the planted rows sit on the first / last prefix sum on purpose
            print('%-16s %-8s b %d: differ %d  within %g ulp by chance %d, within 1 ulp %d' %
                  (c.name, mode, b, int(differ.sum()), M.SAMPLE_ULPS, int(chance.sum()), int((chance & (st.dist <= 1)).sum())))
            assert bool(M.face_allowed(st, idx).all())
            assert bool((st.dist[differ] <= M.SAMPLE_ULPS).all())
            assert int(differ.sum()) <= M.SAMPLE_CAP * c.n
            if c.name == 'all_degenerate':
                assert bool((idx == F - 1).all()) and bool((st.face == F - 1).all())
            else:
                planted = torch.tensor(c.meta['planted'], dtype=torch.long)
                assert not bool(torch.isin(idx, planted).any()) and not bool(torch.isin(st.face, planted).any())
            p64, w64 = M.bary_points(v.double(), f, idx, u)
            assert float((pts.detach().double() - p64).abs().max()) <= 0.5 * M.POINT_BAR
            g = M.sample_weights(c, b)
            (pts * g).sum().backward()
            eg = M.elem_rel_err(vv.grad, M.bary_scatter(v.shape[0], f, idx, w64, g))
            print('    points %.2e  grad %.2e' % (float((pts.detach().double() - p64).abs().max()), eg))
            assert eg <= 0.5 * M.SAMPLE_GRAD_BAR


def test_statement_on_a_hand_made_mesh():
    """Areas 0, 2, 0, 6, 0 (prefix sums 0, 2, 2, 8, 8): the rule skips the faces of no area and the last row stays in range."""
    v = torch.tensor([[0, 0, 0], [2, 0, 0], [0, 2, 0], [6, 0, 0], [1, 0, 0]], dtype=F64)
    f = torch.tensor([[0, 0, 1], [0, 1, 2], [0, 4, 1], [0, 3, 2], [2, 2, 2]])
    u = torch.tensor([[0.0, 0, 0], [0.2, 0, 0], [0.25, 0, 0], [0.25 - 2.0 ** -24, 0, 0], [1 - 2.0 ** -24, 0, 0]])
    st = M.sample_statement(v, f, u)
    assert st.face.tolist() == [1, 1, 3, 1, 3]
    assert st.alt.tolist() == [[-1, 3], [-1, 3], [1, -1], [-1, 3], [1, -1]]
    unit = M.ulp32(8.0)
    assert st.dist.tolist() == [0.0, pytest.approx(0.4 / unit), 0.0, pytest.approx(8 * 2.0 ** -24 / unit), pytest.approx(8 * 2.0 ** -24 / unit)]
    assert M.face_allowed(st, torch.tensor([1, 3, 1, 3, 1])).tolist() == [True, False, True, True, False]
