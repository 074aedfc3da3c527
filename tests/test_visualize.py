"""GPU checks of the visualisation stage (csrc/visualize.hip, modules/visualize.py) against tests/visualize_ref.py.

A kernel is compared with the fp32 restatement; which pixels are AMBIGUOUS is taken from the fp64 restatement (tol 1e-5):
winner and runner-up depths within 1e-5 relative, or the hit margin of either (1 - m2, t_far - t_near, the near plane; for
meshes the distance of the pixel centre to an edge, NDC) within 1e-5 of zero.  Everywhere else the winner must be the same:
at ambient = 1 the bytes of the primitive render are the winner's palette entry (the palettes used here are distinct after
quantisation, background included), so the bytes must be EQUAL; where colour is interpolated or shaded the bytes may differ
by one level (an fp32 value next to an integer, truncated) -- a different winner differs by far more.

At most 0.1 % of an image's pixels may be ambiguous (16 at 128^2, 65 at 256^2): a condition on the inputs, asserted per
image before anything is compared (and printed: run with -s).  Largest count per image, from the fp64 restatement on the
CPU (composed16: for the same primitives meshed by the oracle's transform):
    spheres16 1   mixed8 3   prims64 8   eye_and_behind 2   no_hit 0   composed16 13   sphere386 13   two_samples 14
The mesh counts are what the edges give, not accidents: a pixel centre lies within 1e-5 NDC of an edge with probability
(edge length in pixels) x 2e-5 / (pixel pitch 1 / 64); the visible edges of a 768-face sphere that fills a third of a 128^2
image add up to about ten such pixels.  composed16 (4032 faces) is therefore viewed from dist 3: at dist 2 its seed-21
input had 23 in one image, and the input was changed, not the cap.
Semi-axes stay above 0.08: fp32's own error of 1 - m2 grows with |o~| = distance / semi-axis (about 4 |o~| 2^-24 ~ 6e-6 at
|o~| = 25) and has to stay inside the 1e-5 band that is excluded."""
import functools
import os

import pytest
import torch

import visualize_ref as VR
from geom_util import uv_sphere_386

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CAP = 1e-3


def _params(seed, S, K, vmin, vmax, spread):
    g = torch.Generator().manual_seed(seed)
    v = vmin + (vmax - vmin) * torch.rand(S, K, 3, generator=g)
    q = torch.rand(S, K, 4, generator=g)
    t = spread * (torch.rand(S, K, 3, generator=g) * 2 - 1)
    return torch.cat([v, q, t], 2)


def _turn(dist, elevs, n=12, direct=True, S=1, phase=0.0):
    views = ([(dist, 0.0, 0.0)] if direct else []) + [(dist, float(e), phase + 360.0 * a / n) for a in range(n) for e in elevs]
    return torch.tensor(views, dtype=torch.float32)[None].repeat(S, 1, 1)


def _palette(K):
    from vpn_amd.modules.visualize import default_palette
    return default_palette(K)


PRIM_CASES = {
    # name: (params, kinds, cams, H)
    'spheres16': lambda: (_params(11, 1, 16, 0.10, 0.30, 0.35), [0] * 16, _turn(2.0, (0,)), 128),
    'mixed8': lambda: (_params(12, 1, 8, 0.10, 0.30, 0.35), [1] * 4 + [0] * 4, _turn(2.0, (-30, 0, 30)), 128),
    'prims64': lambda: (_params(13, 2, 64, 0.08, 0.16, 0.35), [1] * 16 + [0] * 48, _turn(2.0, (-30, 0, 30), S=2), 256),
    'eye_and_behind': lambda: (torch.tensor([[[3.0, 3.0, 3.0, 0.1, 0.2, 0.3, 0.1, 0.0, 0.0, 0.0],          # encloses the eye
                                              [0.3, 0.3, 0.3, 0.1, 0.2, 0.3, 0.1, 6.0, 0.0, 0.0],          # behind the first cameras
                                              [0.2, 0.3, 0.2, 0.3, 0.1, 0.2, 0.4, 0.0, 0.1, 0.0],
                                              [2.5, 2.5, 2.5, 0.3, 0.1, 0.2, 0.4, 0.0, 0.0, 0.0]]]),       # a box around the eye
                               [0, 0, 1, 1], torch.tensor([[[2.0, 0.0, 0.0], [2.0, 20.0, 40.0], [2.0, -20.0, 200.0]]]), 128),
    'no_hit': lambda: (torch.tensor([[[0.2, 0.2, 0.2, 0.1, 0.2, 0.3, 0.1, 0.0, 3.0, 0.0],
                                      [0.2, 0.1, 0.2, 0.1, 0.2, 0.3, 0.1, 0.0, -3.0, 0.0]]]), [0, 1], _turn(2.0, (0,), n=4), 128),
}


@functools.lru_cache(maxsize=None)
def _prim_case(name):
    params, kinds, cams, H = PRIM_CASES[name]()
    pal = _palette(len(kinds))
    ref = VR.ref_primitives(params, kinds, cams, pal, H, H)
    amb = VR.ref_primitives(params, kinds, cams, pal, H, H, dtype=torch.float64, tol=VR.AMBIG)['ambiguous']
    return params, kinds, cams, pal, H, ref, amb


def _check_cap(name, amb):
    per_image = amb.flatten(2).sum(-1)
    print('%s: ambiguous pixels per image: max %d of %d' % (name, int(per_image.max()), amb.shape[-1] * amb.shape[-2]))
    assert int(per_image.max()) <= CAP * amb.shape[-1] * amb.shape[-2], (name, per_image.tolist())


@pytest.mark.parametrize('ambient', [1.0, 0.35])
@pytest.mark.parametrize('name', list(PRIM_CASES))
def test_primitive_render_equals_the_restatement(name, ambient):
    from vpn_amd import ops
    params, kinds, cams, pal, H, ref, amb = _prim_case(name)
    _check_cap(name, amb)
    bg = (0.0, 0.0, 0.0)
    got = ops.vis_primitives(params.to(DEV), kinds, cams.to(DEV), pal.to(DEV), H, H, ambient=ambient, background=bg).cpu()
    want = VR.shaded_image(ref, ambient)
    assert got.shape == want.shape == (params.shape[0], cams.shape[1], H, H, 3) and got.dtype == torch.uint8
    diff = (got.int() - want.int()).abs().amax(-1)
    clear = ~amb
    print('%s ambient %.2f: hit pixels %d, pixels that differ at all %d, outside the ambiguous set %d, max level difference there %d'
          % (name, ambient, int((ref['winner'] >= 0).sum()), int((diff > 0).sum()), int((diff[clear] > 0).sum()), int(diff[clear].max())))
    if ambient == 1.0:
        q = VR.quantise(torch.cat([pal, torch.tensor([bg])]))
        assert len({tuple(r) for r in q.tolist()}) == len(q)            # bytes identify the winner
        assert int(diff[clear].max()) == 0
    else:
        assert int(diff[clear].max()) <= 1
    if name == 'no_hit':
        assert int(got.max()) == 0 and int((ref['winner'] >= 0).sum()) == 0
    if name == 'eye_and_behind':
        assert set(ref['winner'][0, 0].unique().tolist()) == {-1, 2}     # neither enclosing primitive nor the one behind is drawn
        assert 1 in ref['winner'][0, 2].unique().tolist()                # ... which the camera on the other side does see


def _mesh_cases():
    from vpn_amd.modules.meshing import Meshing
    from vpn_amd.modules.visualize import position_colors
    out = {}
    p16 = _params(23, 1, 16, 0.10, 0.30, 0.35)
    verts, faces = Meshing.mesh_primitives(p16.to(DEV), [1] * 4 + [0] * 12)
    verts = verts.cpu()
    out['composed16'] = (verts, faces.cpu(), position_colors(verts), _turn(3.0, (20,), n=5, phase=7.0), 128)
    v, f = uv_sphere_386(0.5)
    out['sphere386'] = (v[None], f, position_colors(v[None]), _turn(1.6, (0,), n=12, direct=True, phase=7.0), 128)
    g = torch.Generator().manual_seed(5)
    v2 = torch.stack([v * torch.tensor([1.0, 0.7, 1.2]), v + 0.05 * torch.randn(v.shape, generator=g)])
    out['two_samples'] = (v2, f, position_colors(v2), _turn(1.8, (-25, 35), n=2, direct=False, S=2, phase=11.0), 128)
    return out


@functools.lru_cache(maxsize=None)
def _mesh_case(name):
    verts, faces, colors, cams, H = _mesh_cases()[name]
    ref = VR.ref_mesh(verts, faces, colors, cams, H, H)
    amb = VR.ref_mesh(verts, faces, colors, cams, H, H, dtype=torch.float64, tol=VR.AMBIG)['ambiguous']
    return verts, faces, colors, cams, H, ref, amb


@pytest.mark.parametrize('ambient', [1.0, 0.35])
@pytest.mark.parametrize('name', ['composed16', 'sphere386', 'two_samples'])
def test_mesh_render_equals_the_restatement(name, ambient):
    from vpn_amd import ops
    verts, faces, colors, cams, H, ref, amb = _mesh_case(name)
    _check_cap(name, amb)
    got = ops.vis_mesh(verts.to(DEV), faces.to(DEV, torch.int32), colors.to(DEV), cams.to(DEV), H, H, ambient=ambient).cpu()
    want = VR.shaded_image(ref, ambient)
    diff = (got.int() - want.int()).abs().amax(-1)
    clear = ~amb
    print('%s ambient %.2f: hit pixels %d, pixels that differ at all %d, outside the ambiguous set %d, max level difference there %d'
          % (name, ambient, int((ref['winner'] >= 0).sum()), int((diff > 0).sum()), int((diff[clear] > 0).sum()), int(diff[clear].max())))
    assert int((ref['winner'] >= 0).sum()) > 0.05 * ref['winner'].numel()
    assert int(diff[clear].max()) <= 1
    # background and drawn pixels are told apart exactly (position colours of a drawn pixel are not all zero)
    assert torch.equal((got.amax(-1) > 0)[clear], (want.amax(-1) > 0)[clear])


def test_views_written_through_pitch_and_offset_equal_separate_renders():
    from vpn_amd import ops
    params, kinds, cams, pal, H, _ref, _amb = _prim_case('mixed8')
    V = 6
    cams = cams[:, :V].to(DEV).contiguous()
    dense = ops.vis_primitives(params.to(DEV), kinds, cams, pal.to(DEV), H, H, ambient=0.35)
    # two frames of three columns, with a column left free on the left and a guard row band below
    frames = torch.full((2, H + 4, 4 * H, 3), 77, dtype=torch.uint8, device=DEV)
    pitch = 4 * H * 3
    offs = [f * (H + 4) * pitch + (1 + c) * H * 3 for f in range(2) for c in range(3)]
    out = ops.vis_primitives(params.to(DEV), kinds, cams, pal.to(DEV), H, H, ambient=0.35, out=frames, pitch=pitch, view_offset=offs)
    assert out is frames
    want = torch.full_like(frames, 77)
    for i in range(V):
        f, c = divmod(i, 3)
        want[f, :H, (1 + c) * H:(2 + c) * H] = dense[0, i]
    assert torch.equal(frames, want)
    # offsets as device data: a view that would leave the buffer is skipped by the kernel, the others are written
    bad = torch.tensor(offs[:5] + [frames.numel() - 10], dtype=torch.int64, device=DEV)
    frames2 = torch.full_like(frames, 77)
    ops.vis_primitives(params.to(DEV), kinds, cams, pal.to(DEV), H, H, ambient=0.35, out=frames2, pitch=pitch, view_offset=bad)
    want[1, :H, 3 * H:4 * H] = 77
    assert torch.equal(frames2, want)
    # the mesh kernel through the same addressing
    verts, faces, colors, mcams, Hm, _r, _a = _mesh_case('sphere386')
    mc = mcams[:, :V].to(DEV).contiguous()
    args = (verts.to(DEV), faces.to(DEV, torch.int32), colors.to(DEV), mc, Hm, Hm)
    dense = ops.vis_mesh(*args)
    frames.fill_(77)
    ops.vis_mesh(*args, out=frames, pitch=pitch, view_offset=offs)
    want.fill_(77)
    for i in range(V):
        f, c = divmod(i, 3)
        want[f, :H, (1 + c) * H:(2 + c) * H] = dense[0, i]
    assert torch.equal(frames, want)
    with pytest.raises(ValueError):
        ops.vis_mesh(*args, out=frames, pitch=pitch, view_offset=offs[:5] + [frames.numel()])


def _scene():
    """(image, K Meshing-made meshes of one sample, the pack behind them) as test.py:114-123 builds them."""
    from vpn_amd import Meshing, PrimitivePack
    p = _params(31, 1, 6, 0.10, 0.25, 0.3).to(DEV)
    kinds = [1, 1, 0, 0, 0, 0]
    meshes = []
    for k, kind in enumerate(kinds):
        fn = Meshing.cuboid_meshing if kind == 1 else Meshing.sphere_meshing
        meshes.append(fn(p[:, k, 0:3], p[:, k, 3:7], p[:, k, 7:10])[0])
    image = torch.rand(3, 137, 137, generator=torch.Generator().manual_seed(3)).to(DEV)
    return image, meshes, PrimitivePack(p, kinds)


def _sphere_mesh():
    from vpn_amd import TriangleMesh
    v, f = uv_sphere_386(0.5)
    return TriangleMesh(v.to(DEV), f.to(DEV, torch.int32))


def test_no_host_synchronisation_and_graph_replay():
    from vpn_amd import Visualizer
    image, meshes, pack = _scene()
    sphere = _sphere_mesh()
    refined = torch.cat([m.vertices for m in meshes]) * 1.05
    cams = _turn(2.0, (-30, 0, 30))[0].to(DEV)
    calls = {
        'turntable': lambda: Visualizer.turntable(pack, cams, image_size=128),
        'turntable_mesh': lambda: Visualizer.turntable(sphere, cams, image_size=128, ambient=0.35),
        'frames_vp_meshes': lambda: Visualizer.frames_vp_meshes(image, meshes, is_three_elev=True),
        'frames_mesh_gif': lambda: Visualizer.frames_mesh_gif(image, sphere, 1.6),
        'frames_mesh_3pose': lambda: Visualizer.frames_mesh_3pose(image, sphere, 1.6, 10.0, 40.0),
        'frames_refine_vp_meshes': lambda: Visualizer.frames_refine_vp_meshes(image, meshes, refined),
    }
    eager = {k: fn() for k, fn in calls.items()}                        # first calls: the cached view lists are uploaded
    torch.cuda.synchronize()
    assert eager['frames_vp_meshes'].shape == (12, 256, 5 * 256, 3) and eager['frames_refine_vp_meshes'].shape == (12, 256, 5 * 256, 3)
    assert eager['frames_mesh_gif'].shape == (12, 256, 4 * 256, 3) and eager['frames_mesh_3pose'].shape == (1, 256, 4 * 256, 3)
    assert eager['turntable'].shape == (1, 37, 128, 128, 3)
    torch.cuda.set_sync_debug_mode('error')
    try:
        again = {k: fn() for k, fn in calls.items()}
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for k in calls:
        assert torch.equal(again[k], eager[k]), k
    # captured once, replayed twice: the bytes of the eager call
    for k in ('turntable', 'frames_vp_meshes', 'frames_mesh_gif', 'frames_refine_vp_meshes'):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            calls[k]()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = calls[k]()
        for _ in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager[k]), k


def test_vp_dump_takes_meshes_or_a_pack_and_edited_meshes_render_their_triangles(monkeypatch):
    from vpn_amd import Visualizer, ops
    image, meshes, pack = _scene()
    a = Visualizer.frames_vp_meshes(image, meshes)
    b = Visualizer.frames_vp_meshes(image, pack)
    assert a.shape == (12, 256, 3 * 256, 3) and torch.equal(a, b)
    assert torch.equal(a[:, :, 256:512], a[:1, :, 256:512].expand(12, -1, -1, -1))          # the direct pose, once, in every frame
    assert torch.equal(a[0, :, 512:], a[0, :, 256:512])                                      # azim 0 is the direct pose
    # an edit: the primitives are no longer trusted, the triangle kernel draws what the vertices say
    seen = []
    real = ops.vis_mesh
    monkeypatch.setattr(ops, 'vis_mesh', lambda *a_, **k_: (seen.append(1), real(*a_, **k_))[1])
    meshes[2].vertices += 0.0
    c = Visualizer.frames_vp_meshes(image, meshes)
    assert seen == [1]
    # observation, not a bound: the polyhedra are inscribed in their primitives, so the two silhouettes differ along the outlines
    sa, sc = a[:, :, 256:].amax(-1) > 0, c[:, :, 256:].amax(-1) > 0
    print('silhouette pixels: primitives %d, triangles %d, triangles outside the primitives %d' % (int(sa.sum()), int(sc.sum()), int((sc & ~sa).sum())))
    assert int(sc.sum()) > 0.8 * int(sa.sum())


def test_gif_end_to_end(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from vpn_amd import Visualizer
    image, meshes, _pack = _scene()
    path = str(tmp_path / 'vp.gif')
    Visualizer.render_vp_meshes(image, meshes, path, dist=2.0, is_three_elev=True)
    with Image.open(path) as im:
        assert im.n_frames == 12 and im.size == (5 * 256, 256) and im.info['duration'] == 300 and im.info['loop'] == 0
    png = str(tmp_path / 'pose.png')
    Visualizer.render_mesh_3pose(image, _sphere_mesh(), png, 1.6, 0.0, 30.0)
    with Image.open(png) as im:
        assert im.size == (4 * 256, 256)
        want = Visualizer.frames_mesh_3pose(image, _sphere_mesh(), 1.6, 0.0, 30.0)[0].cpu()
        import numpy as np
        assert torch.equal(torch.from_numpy(np.array(im.convert('RGB'))), want)
