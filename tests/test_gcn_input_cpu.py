"""CPU checks of the cases of tests/gcn_input_ref.py (the plain GCN input op): every case builds with its
conditions, its float64 reference is finite, the same restatement in fp32 agrees with it (the reference's own fp32 error,
printed: the GPU bars of tests/test_gcn_input.py are set against it), the tie rule of torch.max / torch.min is the one the
kernels follow, and the aggregation and bounds edge cases are what they claim to be."""
import pytest
import torch

import gcn_input_ref as G
import gcn_ref as R
from conftest import rel_err
from test_gcn_cpu import _check_adjacency


@pytest.mark.parametrize('name', sorted(G.CASES))
def test_case_builds_and_the_restatement_agrees_with_itself_in_fp32(name):
    c, spec = G.case(name), G.CASES[name]
    assert c['verts'].shape == (spec['B'], spec['N'], 3) and c['verts'].dtype == torch.float32
    assert [tuple(m.shape[1:]) for m in c['maps']] == spec['maps']
    assert (c['glob'] is None) == (spec['G'] == 0)
    share = float(c['masked'].double().mean())
    assert share <= G.MAX_MASKED and not bool((c['masked'] & c['extent']).any())
    x64, dv64, dg64, dm64 = G.reference64(name)
    x32, dv32, dg32, dm32 = G.reference32(name)
    ctot = spec['venc'] + sum(m[0] for m in spec['maps']) + spec['G']
    assert x64.shape == (spec['B'], spec['N'], ctot) and dv64.shape == c['verts'].shape
    for t in [x64, dv64] + ([dg64] if dg64 is not None else []) + dm64:
        assert bool(torch.isfinite(t).all())
    keep = ~c['masked']
    errs = dict(x=rel_err(x32, x64), dverts=rel_err(dv32[keep], dv64[keep]))
    if dg64 is not None:
        errs['dglob'] = rel_err(dg32, dg64)
    for i, (a, b) in enumerate(zip(dm32, dm64)):
        errs['dmap%d' % i] = rel_err(a, b)
    split = G.split_errors(dv32, dv64, c)
    print(name, 'masked %d of %d' % (int(c['masked'].sum()), c['masked'].numel()), 'fp32 restatement:', errs,
          'split (O, E): %.2e %.2e' % split)
    assert errs.pop('x') <= 1e-5
    for k, e in errs.items():
        assert e <= 1e-4, (k, e)
    assert max(split) < 1.0                          # a wrong floor or a wrong tie would show as an error of order 1


def test_ties_go_to_the_lowest_index_in_the_reference():
    c = G.case('ties')
    G.check_tie_layout(c)
    dv, direct = G.reference64('ties')[1], G.reference_without_extent_term(c)
    for i, cols in G.later_tie_rows().items():
        assert torch.allclose(dv[:, i, cols], direct[:, i, cols], rtol=1e-12, atol=0), i
    for key, g in G.TIE_GROUPS.items():               # ... and the whole sum sits on the first one
        col = 2 if key[0] == 'z' else 1
        gap = (dv[:, min(g), col] - direct[:, min(g), col]).abs()
        assert bool((gap > 1e-3 * dv[..., col].abs().max()).all()), (key, gap)


def test_crowded_cells_and_outside_corners():
    c = G.case('crowded')
    for counts in G.cell_counts(c['verts'], c['bounds'], 32, 32):
        assert int(counts.max()) >= 128 and set((counts % 4).tolist()) == {0, 1, 2, 3}
    c = G.case('corners_outside')
    out, inside = G.F.outside_fractions(c['verts'], c['bounds'], 32)
    assert out >= 0.2 and inside >= 0.2
    c = G.case('empty_image')                          # the extreme vertices sit exactly on ix = W - 1 and ix = 0
    ix, iy = G.grid_coordinates(c['verts'], c['bounds'], G.SMALL_SQUARE)[0]
    assert float(ix.max()) == 31.0 and float(ix.min()) == 0.0 and float(iy.max()) == 31.0 and float(iy.min()) == 0.0
    c = G.case('one_column')
    ix = G.grid_coordinates(c['verts'], c['bounds'], G.SMALL_SQUARE)[0][0]
    assert bool((ix == ix[:, :1]).all())


def test_adjacency_of_irregular_meshes():
    faces, n = G.irregular_mesh()
    _check_adjacency(faces, n)
    from vpn_amd import ops
    rp, col, w = ops.gcn_normalized_adjacency(ops.gcn_edges(faces), n)
    assert int(rp[9] - rp[8]) == 1 and int(col[rp[8]]) == 8 and float(w[rp[8]]) == 1.0     # the isolated vertex: y = h + bias
    assert ops.gcn_edges(faces).tolist() == [[0, 1], [0, 2], [0, 6], [0, 7], [1, 2], [2, 3], [2, 5], [3, 4], [3, 5], [4, 5],
                                             [4, 6], [5, 6], [5, 7], [6, 7]]
    _check_adjacency(torch.zeros(0, 3, dtype=torch.long), 1)
    _check_adjacency(*G.random_mesh(131, 300, 5))


@pytest.mark.parametrize('shape', G.BOUNDS_SHAPES)
def test_bounds_images_are_exact_and_dim_pixels_move_nothing(shape):
    C, H, W = shape
    imgs, only = G.bounds_images(C, H, W)
    assert torch.equal(imgs * 256, (imgs * 256).round())
    s = imgs.sum(1)
    assert set(s.unique().tolist()) <= {0.0, 7 / 256, 8 / 256} and 7 / 256 < 0.03 < 8 / 256
    assert torch.equal(s, imgs.flip(1).sum(1))
    if H * W >= 100:
        assert bool((s == 7 / 256).flatten(1).any(1)[[0, 2, 3, 4, 5]].all())
    b = R.bounds(imgs)
    assert torch.equal(b, R.bounds(only))
    assert b[0].tolist() == [-1.0, 1.0, -1.0, 1.0]                    # empty: "unset" on both sides
    assert b[2, 1] == -1.0 and b[3, 3] == -1.0                       # only column 0 / row 0: the far bound is 0
    last = torch.tensor([W - 1.0, W - 1.0, H - 1.0, H - 1.0]) / torch.tensor([W, W, H, H]) * 2 - 1
    assert torch.equal(b[4], last)                                    # a single pixel: both bounds on it (0 stays "unset")
