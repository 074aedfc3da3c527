"""CPU checks of the middle of the ACD-mix stage: the properties of the specification on its numpy
restatement (tests/acdmix_ref.py), the C ABI entries, and the reference's names in modules/augmentation.py.  No GPU call
is made."""
import ctypes
import functools
import inspect

import numpy as np
import pytest
import torch

import acdmix_ref as AR
import reconstruct_ref as RR

F = np.float32
MARGIN = 1e-3
DIRS = np.concatenate([AR.lattice_dirs(), RR.random_dirs(42, seed=2)])         # the axes among them: a box's outer polytope is the box


def _draws(S, O, G, coin=0, u_num=0.0, scale=1.0, turn=2, shift=0.0, u_hull=None):
    full = lambda v, dt: np.full((S, O), v, dt)
    return dict(coin=full(coin, np.int32), u_num=full(u_num, F), scale=full(scale, F), turn=full(turn, np.int32),
                shift=full(shift, F), u_hull=np.zeros((S, G), F) if u_hull is None else np.asarray(u_hull, F).reshape(S, G))


def _filter(hulls, keep, cands, n_out, dirs=DIRS, margin=MARGIN):
    """hulls: list of [D,3]; cands: list of [n_h,3], the candidates drawn on each hull -> the restatement's outputs."""
    cand = np.concatenate(cands)[None]
    own = np.concatenate([np.full(len(c), h, np.int32) for h, c in enumerate(cands)])[None]
    return AR.union_surface(np.stack(hulls)[None], np.asarray(keep, np.int32)[None], dirs, cand, own, margin, n_out), cand, own


def test_two_disjoint_boxes_keep_every_candidate():
    a, b = ([-0.5, -0.5, -0.5], [-0.1, 0.5, 0.5]), ([0.1, -0.5, -0.5], [0.5, 0.5, 0.5])
    hulls = [AR.box_hull(*a, DIRS), AR.box_hull(*b, DIRS)]
    (sup, outside, points, src, count), cand, _ = _filter(hulls, [1, 1], [AR.box_points(*a, 300, 1), AR.box_points(*b, 300, 2)], 600)
    assert outside.all() and count.tolist() == [600]
    assert np.array_equal(src[0], np.arange(600)) and np.array_equal(points, cand)
    assert sup.shape == (1, 2, 48) and np.array_equal(sup[0, 0], RR.dot(hulls[0][:, None, :], DIRS[None]).max(0))


def test_a_hull_inside_another_contributes_nothing():
    big, small = ([-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]), ([-0.1, -0.2, -0.1], [0.2, 0.1, 0.1])
    hulls = [AR.box_hull(*big, DIRS), AR.box_hull(*small, DIRS)]
    (_, outside, _, src, count), _, own = _filter(hulls, [1, 1], [AR.box_points(*big, 200, 3), AR.box_points(*small, 100, 4)], 256)
    assert outside[0, :200].all() and not outside[0, 200:].any() and count.tolist() == [200]
    assert (own[0, src[0]] == 0).all()


@functools.lru_cache(maxsize=None)
def _overlap(n_out=512):
    """Two ellipsoids, centres one semi-axis apart, nc = 2 n_out candidates."""
    ra, rb = (0.4, 0.3, 0.25), (0.3, 0.35, 0.3)
    ca, cb = (0.0, 0.0, 0.0), (0.4, 0.0, 0.0)
    hulls = [AR.ellipsoid_hull(ca, ra, DIRS), AR.ellipsoid_hull(cb, rb, DIRS)]
    cands = [AR.ellipsoid_points(ca, ra, n_out, 5), AR.ellipsoid_points(cb, rb, n_out, 6)]
    out, cand, own = _filter(hulls, [1, 1], cands, n_out)
    return hulls, cand, own, out


def test_overlapping_pair_in_fp64():
    n_out = 512
    hulls, cand, own, (sup, outside, points, src, count) = _overlap(n_out)
    assert cand.shape[1] == 2 * n_out
    print('overlap: %d of %d candidates survive' % (int(count[0]), cand.shape[1]))
    assert int(count[0]) >= n_out                      # padding cannot hide a filter that rejects too much
    assert int(count[0]) < cand.shape[1]               # ... and the pair does overlap
    for h in range(2):
        other = own[0] != h
        deep = AR.inside_fp64(cand[0], hulls[h], DIRS, MARGIN + 1e-6)
        shallow = AR.inside_fp64(cand[0], hulls[h], DIRS, MARGIN - 1e-6)
        assert not (outside[0].astype(bool) & other & deep).any()          # no survivor is inside the other hull beyond the margin
        assert ((outside[0] == 0) & other <= shallow).all()                # every rejected candidate is inside it
    assert np.array_equal(src[0], np.nonzero(outside[0])[0][:n_out]) and np.array_equal(points[0], cand[0, src[0]])


def _object(zs, D=6):
    """Hulls [1,G,D,3] whose z ranges are given: unit squares in x, y, distinct vertices."""
    hulls = []
    for g, (z0, z1) in enumerate(zs):
        v = np.array([[g + 0.125, 0.25, z0], [g + 0.5, 0.25, z1], [g + 0.5, 0.75, z0], [g + 0.125, 0.75, z1], [g + 0.25, 0.5, z0],
                      [g + 0.375, 0.5, z1]], F)
        hulls.append(v[:D])
    return np.stack(hulls)[None]


def test_cut_hulls_collapse_and_contribute_nothing():
    verts = _object([(-0.5, 0.5), (-0.25, 0.25), (0.5, 0.75)])          # two centre hulls, one not
    d = _draws(1, 1, 3, coin=1, u_num=0.0, u_hull=[0.9, 0.1, 0.0])
    out, keep = AR.hull_augment(verts, [0, 0, 0], **d)
    assert keep.tolist() == [[1, 0, 1]]                                 # hull 1: the smallest key among the centre hulls
    assert (out[0, 1] == verts[0, 1, 0]).all() and np.array_equal(out[0, 0], verts[0, 0]) and np.array_equal(out[0, 2], verts[0, 2])
    cands = [np.tile(out[0, g].mean(0, keepdims=True), (10, 1)).astype(F) for g in range(3)]
    (_, outside, _, src, count), _, own = _filter(list(out[0]), keep[0], cands, 16, dirs=AR.lattice_dirs())
    assert not outside[0, 10:20].any() and (own[0, src[0]] != 1).all() and count.tolist() == [20]
    # the coin says no: exactly the centre hulls stay
    _, keep = AR.hull_augment(verts, [0, 0, 0], **_draws(1, 1, 3, coin=0))
    assert keep.tolist() == [[1, 1, 0]]
    # u_num picks the number: 3 centre hulls, floor(0.99 * 2) + 1 = 2 cut, never all of them
    verts = _object([(-0.5, 0.5), (-0.25, 0.25), (-0.125, 0.5)])
    _, keep = AR.hull_augment(verts, [0, 0, 0], **_draws(1, 1, 3, coin=1, u_num=0.99, u_hull=[0.5, 0.7, 0.6]))
    assert keep.tolist() == [[0, 1, 0]]
    _, keep = AR.hull_augment(verts, [0, 0, 0], **_draws(1, 1, 3, coin=1, u_num=7.0, u_hull=[0.5, 0.7, 0.6]))
    assert keep.sum() == 1


def test_turn_indices_are_exact_signed_swaps():
    verts = _object([(-0.5, 0.5)])
    x, y, z = (verts[0, 0, :, k] for k in range(3))
    want = {0: (-y, x), 1: (y, -x), 2: (x, y), 3: (-x, -y), 4: (-x, -y)}
    for turn, (wx, wy) in want.items():
        out, keep = AR.hull_augment(verts, [0], **_draws(1, 1, 1, turn=turn))
        assert keep.tolist() == [[1]]
        assert np.array_equal(out[0, 0, :, 0], wx) and np.array_equal(out[0, 0, :, 1], wy) and np.array_equal(out[0, 0, :, 2], z)
        # ... which is rotate_points about (0,0,1) by TURNS[turn] degrees (rotate.py:23,36-44), up to its rounding
        a = np.deg2rad(AR.TURNS[turn])
        R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        assert np.abs(np.stack([wx, wy]) - R @ np.stack([x, y]).astype(np.float64)).max() < 1e-12
    # the reference's order: scale, turn, shift along y
    out, _ = AR.hull_augment(verts, [0], **_draws(1, 1, 1, turn=0, scale=1.1, shift=0.07))
    s, t = F(1.1), F(0.07)
    assert np.array_equal(out[0, 0, :, 0], -(y * s)) and np.array_equal(out[0, 0, :, 1], x * s + t) and np.array_equal(out[0, 0, :, 2], z * s)


def test_no_centre_hull_and_a_single_one():
    verts = _object([(0.5, 0.75), (0.25, 0.5), (-0.75, -0.5), (-0.5, 0.5)])
    group = [0, 0, 1, 1]
    for coin in (0, 1):
        _, keep = AR.hull_augment(verts, group, **_draws(1, 2, 4, coin=coin, u_num=0.9))
        # object 0 has no centre hull: kept whole (the deviation); object 1 has one: it alone stays, coin or not
        assert keep.tolist() == [[1, 1, 0, 1]]
    # a hull that belongs to no object is cut
    out, keep = AR.hull_augment(verts, [0, 5, 1, -1], **_draws(1, 2, 4))
    assert keep.tolist() == [[1, 0, 1, 0]] and (out[0, 1] == verts[0, 1, 0]).all() and (out[0, 3] == verts[0, 3, 0]).all()
    # min |z| < 0.05 makes a centre hull too
    _, keep = AR.hull_augment(_object([(0.04, 0.5), (0.05, 0.5), (-0.5, 0.5)]), [0, 0, 0], **_draws(1, 1, 3))
    assert keep.tolist() == [[1, 0, 1]]


def test_equal_keys_go_to_the_lowest_index():
    verts = _object([(-0.5, 0.5)] * 4)
    _, keep = AR.hull_augment(verts, [0] * 4, **_draws(1, 1, 4, coin=1, u_num=0.5, u_hull=[0.5, 0.25, 0.25, 0.25]))
    assert keep.tolist() == [[1, 0, 0, 1]]                              # 1 + floor(0.5 * 3) = 2 of the three equal keys: 1 and 2


def test_padding_rule_and_the_empty_rule():
    big, small = ([-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]), ([-0.1, -0.2, -0.1], [0.2, 0.1, 0.1])
    hulls = [AR.box_hull(*big, DIRS), AR.box_hull(*small, DIRS)]
    cands = [AR.box_points(*big, 5, 3), AR.box_points(*small, 9, 4)]
    (_, outside, points, src, count), cand, _ = _filter(hulls, [1, 1], cands, 12)
    assert count.tolist() == [5] and src[0].tolist() == [0, 1, 2, 3, 4] * 2 + [0, 1]       # slot i repeats survivor i mod count
    assert np.array_equal(points[0], cand[0, src[0]])
    # nothing survives (every hull cut): the candidates themselves, src = i mod nc
    (_, outside, points, src, count), cand, _ = _filter(hulls, [0, 0], cands, 17)
    assert count.tolist() == [0] and not outside.any() and src[0].tolist() == [i % 14 for i in range(17)]
    assert np.array_equal(points[0], cand[0, src[0]])
    # a candidate that names no hull is rejected
    cand_hull = np.array([[0, 1, -1, 2]], np.int32)
    out = AR.union_surface(np.stack(hulls)[None], np.array([[1, 0]], np.int32), DIRS, AR.box_points(*big, 4, 1)[None], cand_hull, MARGIN, 4)
    assert out[1].tolist() == [[1, 0, 0, 0]]


def test_entries_are_bound_and_exported():
    import vpn_amd._lib as lib
    L = lib.lib()
    for name in ('vpn_hull_augment', 'vpn_union_surface'):
        assert name in lib.SIGNATURES and hasattr(ctypes.CDLL(lib.LIB_PATH), name)
    assert L.vpn_abi_version() == 9                                    # entries added, none changed
    one = ctypes.c_void_p(16)                                          # never dereferenced: the size checks come first
    aug = lambda S, G, D, O, p=one: L.vpn_hull_augment(p, one, one, one, one, one, one, one, S, G, D, O, one, one, None)
    uni = lambda S, G, D, nc, n_out, margin=1e-3, p=one: L.vpn_union_surface(p, one, one, one, one, S, G, D, nc, n_out, margin, one, one,
                                                                             one, one, one, None)
    assert aug(1, 2, 6, 1, None) == -1 and uni(1, 2, 6, 8, 8, p=None) == -1
    assert L.vpn_hull_augment(one, one, one, one, one, one, one, one, 1, 2, 6, 1, one, None, None) == -1
    assert L.vpn_union_surface(one, one, one, one, one, 1, 2, 6, 8, 8, 1e-3, one, one, one, one, None, None) == -1
    assert aug(0, 2, 6, 1) == -1 and aug(1, 2, 6, 0) == -1 and uni(1, 2, 6, 0, 8) == -1 and uni(1, 2, 6, 8, 0) == -1
    assert uni(1, 2, 6, 8, 8, margin=float('nan')) == -1
    assert aug(1, 65, 6, 1) == -2 and aug(1, 2, 257, 1) == -2 and aug(65536, 2, 6, 1) == -2 and aug(1, 2, 6, 65) == -2
    assert uni(1, 65, 6, 8, 8) == -2 and uni(1, 2, 257, 8, 8) == -2 and uni(65536, 2, 6, 8, 8) == -2 and uni(1, 2, 6, 16385, 8) == -2


def test_reference_names_and_positional_parameters():
    import vpn_amd
    from vpn_amd.modules import augmentation as A
    sig = inspect.signature

    def positional(fn):
        return [p.name for p in sig(fn).parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]

    assert positional(A.acd) == ['points', 'hull_num'] and sig(A.acd).parameters['hull_num'].default == 8          # acd.py:24
    assert positional(A.augment) == ['hulls']                                                                      # acd.py:114
    assert positional(A.acd_mix_meshes) == ['points1', 'points2'] and positional(A.acd_mix_data) == ['points1', 'points2']
    for kw in ('coin', 'u_num', 'scale', 'turn', 'shift', 'u_hull', 'colors', 'seed', 'margin'):
        assert sig(A.acd_mix_meshes).parameters[kw].kind == inspect.Parameter.KEYWORD_ONLY
        assert sig(A.acd_mix_data).parameters[kw].kind == inspect.Parameter.KEYWORD_ONLY
    p = sig(A.acd_mix_data).parameters
    assert p['views'].default == 20 and p['img_size'].default is None and p['num_points'].default == 2048          # generate.py:150
    assert p['margin'].default == 1e-3 and p['mix_hull_num'].default == 8 and p['cams'].kind == inspect.Parameter.KEYWORD_ONLY
    assert A.ACD_TURNS == AR.TURNS
    for name in ('acd', 'augment', 'acd_mix_meshes', 'acd_mix_data', 'hull_augment', 'union_surface', 'acd_mix_points'):
        assert callable(getattr(vpn_amd, name))
    # the draws follow torch.manual_seed in the stated order, and a draw that is given is not drawn
    torch.manual_seed(3)
    d = A._augment_draws(2, 2, 3, None, None, None, None, None, None)
    torch.manual_seed(3)
    for s in range(2):
        for o in range(2):
            assert int(d['coin'][s, o]) == int(torch.randint(0, 2, (1,)))
            assert float(d['u_num'][s, o]) == torch.rand(1).item()
            assert torch.equal(d['u_hull'][s, 3 * o:3 * o + 3], torch.rand(3))
            assert float(d['scale'][s, o]) == float(torch.tensor(0.8 + torch.rand(1).item() * 0.4))
            assert int(d['turn'][s, o]) == int(torch.randint(0, 5, (1,)))
            assert float(d['shift'][s, o]) == float(torch.tensor((torch.rand(1).item() - 0.5) / 5))
    assert 0.8 <= float(d['scale'].min()) and float(d['scale'].max()) <= 1.2 and float(d['shift'].abs().max()) <= 0.1
    torch.manual_seed(3)
    first = torch.rand(1)
    torch.manual_seed(3)
    e = A._augment_draws(2, 2, 3, d['coin'], d['u_num'], d['scale'], d['turn'], d['shift'], d['u_hull'])
    assert all(e[k] is d[k] for k in d) and torch.equal(torch.rand(1), first)
    with pytest.raises(RuntimeError, match='GPU only'):                # no CPU path
        vpn_amd.union_surface(torch.rand(1, 2, 6, 3), torch.ones(1, 2, dtype=torch.int32), torch.rand(6, 3), torch.rand(1, 8, 3),
                              torch.zeros(1, 8, dtype=torch.int32), 8)
    with pytest.raises(RuntimeError, match='gradients'):               # data only
        vpn_amd.hull_augment(torch.rand(1, 2, 6, 3, requires_grad=True), [0, 0], [[0]], [[0.0]], [[1.0]], [[2]], [[0.0]], [[0.0, 0.0]])
    with pytest.raises(RuntimeError, match='gradients'):
        vpn_amd.acd_mix_data(torch.rand(1, 16, 3, requires_grad=True), torch.rand(1, 16, 3))
    with pytest.raises(ValueError, match='union_surface'):             # shapes are checked before anything is unpacked
        vpn_amd.union_surface(torch.rand(2, 6, 3), torch.ones(1, 2, dtype=torch.int32), torch.rand(6, 3), torch.rand(1, 8, 3),
                              torch.zeros(1, 8, dtype=torch.int32), 8)
