"""CPU checks of the visualisation stage: the restatement (tests/visualize_ref.py) tied to what the oracle already pins, the
frame assembly of modules/visualize.py with renders injected on the CPU, the save path, the palette, argument validation and
the agreement of header, binding and built library.  No GPU."""
import ctypes
import math
import os
import re

import pytest
import torch

import visualize_ref as VR
from conftest import ROOT
from oracle import vpn_oracle as O
from test_kernel_budget_cpu import _resources

CAMS = torch.tensor([[[2.0, 0.0, 0.0], [1.5, 25.0, 70.0], [2.5, -35.0, 200.0]]])


@pytest.mark.parametrize('kind', [O.SPHERE, O.CUBOID])
def test_hit_mask_is_the_half_level_of_the_soft_raster(kind):
    """K = 1: coverage is sigmoid((1 - m2) / sigma), and for the cuboid lam < 1 iff the line meets the box, so alpha > 0.5 is
    the hit mask.  Compared outside the pixels whose decision hangs on less than 1e-5."""
    params = torch.tensor([[[0.30, 0.20, 0.25, 0.3, 0.5, 0.2, 0.15, 0.05, -0.04, 0.08]]])
    H = 96
    r32 = VR.ref_primitives(params, [kind], CAMS, torch.ones(1, 3), H, H)
    r64 = VR.ref_primitives(params, [kind], CAMS, torch.ones(1, 3), H, H, dtype=torch.float64, tol=VR.AMBIG)
    clear = ~r64['ambiguous']
    for vi in range(CAMS.shape[1]):
        alpha, _ = O.raster(params, [kind], CAMS[:, vi], H, H, sigma=0.05)
        a64, _ = O.raster(params.double(), [kind], CAMS[:, vi].double(), H, H, sigma=0.05)
        ok = clear[0, vi] & ((a64[0] - 0.5).abs() > 1e-5 / 0.05 / 4)            # |1 - m2| > 1e-5 in the oracle's own terms
        hit = r32['winner'][0, vi] >= 0
        assert int(hit.sum()) > 200
        assert torch.equal(hit[ok], (alpha[0] > 0.5)[ok])
        assert int((~ok).sum()) <= 4


def test_nearer_sphere_wins_and_the_opposite_camera_swaps_them():
    params = torch.tensor([[[0.2, 0.2, 0.2, 0.1, 0.2, 0.3, 0.0, 0.5, 0.0, 0.0],
                            [0.3, 0.3, 0.3, 0.1, 0.2, 0.3, 0.0, -0.5, 0.0, 0.0]]])
    pal = torch.tensor([[0.9, 0.1, 0.1], [0.1, 0.2, 0.9]])
    cams = torch.tensor([[[2.0, 0.0, 0.0], [2.0, 0.0, 180.0]]])
    r = VR.ref_primitives(params, [0, 0], cams, pal, 64, 64)
    c = 32
    assert r['winner'][0, 0, c, c] == 0 and r['winner'][0, 1, c, c] == 1
    assert r['image'][0, 0, c, c].tolist() == VR.quantise(pal[0]).tolist()
    assert r['image'][0, 1, c, c].tolist() == VR.quantise(pal[1]).tolist()
    assert abs(float(r['depth'][0, 0, c, c]) - 1.3) < 1e-2 and abs(float(r['runner'][0, 0, c, c]) - 2.2) < 1e-2
    # equal depths go to the lowest index: the same sphere twice
    twice = params[:, :1].repeat(1, 2, 1)
    assert int(VR.ref_primitives(twice, [0, 0], cams, pal, 64, 64)['winner'].max()) == 0


def _triangle():
    # in the plane x = 0, facing the camera at (2, 0, 0): image x is -z, image y is y
    verts = torch.tensor([[[0.0, -0.5, 0.6], [0.0, -0.5, -0.6], [0.0, 0.6, 0.0]]])
    colors = torch.eye(3)[None]
    return verts, torch.tensor([[0, 1, 2]]), colors, torch.tensor([[[2.0, 0.0, 0.0]]])


def test_one_triangle_centroid_colour_and_area():
    verts, faces, colors, cams = _triangle()
    H = 128
    r = VR.ref_mesh(verts, faces, colors, cams, H, H)
    pr = O.mesh_project(verts, cams[0])[0]
    cx, cy = float(pr[:, 0].mean()), float(pr[:, 1].mean())
    col, row = int((cx + 1) * 0.5 * H), int((1 - cy) * 0.5 * H)
    got = r['image'][0, 0, row, col].int()
    assert int((got - 85).abs().max()) <= 1 + 3, got                    # the pixel centre is up to half a pixel from the centroid
    # exactly at the centroid's own pixel the interpolated colour is the mean +- 1 level once the offset is accounted for
    th = math.tan(0.5 * O.FOVY_DEG * math.pi / 180)
    px, py = O.pixel_grid(H, H)
    p = torch.tensor([px[col] / th, py[row] / th])
    a, b, c = pr[0, :2], pr[1, :2], pr[2, :2]
    area = float((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))
    w = [float((x[0] - p[0]) * (y[1] - p[1]) - (x[1] - p[1]) * (y[0] - p[0])) / area for x, y in ((b, c), (c, a), (a, b))]
    assert int((got - VR.quantise(torch.tensor(w))).abs().max()) <= 1          # all corners at one depth: plain barycentrics
    covered = int((r['winner'] >= 0).sum())
    pix = (2.0 / H) ** 2
    perimeter = float((a - b).norm() + (b - c).norm() + (c - a).norm()) / (2.0 / H)
    assert abs(covered - abs(area) / 2 / pix) <= perimeter, (covered, abs(area) / 2 / pix, perimeter)


def test_face_with_a_vertex_behind_the_near_plane_is_not_drawn():
    verts, faces, colors, cams = _triangle()
    verts = verts.clone()
    verts[0, 2] = torch.tensor([2.0 - 0.5 * O.MESH_NEAR, 0.0, 0.0])     # depth 0.5 MESH_NEAR
    r = VR.ref_mesh(verts, faces, colors, cams, 64, 64)
    assert int(r['winner'].max()) == -1 and int(r['image'].max()) == 0
    # ... while the triangle behind it still is, and the nearer of two wins
    far = torch.tensor([[0.0, -0.5, 0.6], [0.0, -0.5, -0.6], [0.0, 0.6, 0.0]]) - torch.tensor([0.4, 0.0, 0.0])
    v2 = torch.cat([_triangle()[0][0], far])[None]
    r2 = VR.ref_mesh(v2, torch.tensor([[3, 4, 5], [0, 1, 2]]), torch.rand(1, 6, 3), cams, 64, 64)
    assert r2['winner'][0, 0, 32, 32] == 1 and abs(float(r2['runner'][0, 0, 32, 32]) - 2.4) < 1e-5


def _fake_render(log):
    """Draws view (dist, elev, azim) as the constant colour (azim / 30, elev / 30 + 1, 10 dist) into its block."""
    def render(job, frames, size):
        log.append(job)
        for d, e, a, f, c in job.views:
            frames[f, :, c * size:(c + 1) * size] = torch.tensor([int(a) // 30, int(e) // 30 + 1, int(d * 10)], dtype=torch.uint8)
    return render


def _cpu_scene(K=3):
    from vpn_amd import PrimitivePack
    g = torch.Generator().manual_seed(0)
    p = torch.cat([torch.rand(1, K, 3, generator=g) * 0.2 + 0.1, torch.rand(1, K, 4, generator=g), torch.rand(1, K, 3, generator=g) * 0.4 - 0.2], 2)
    image = torch.rand(3, 64, 96, generator=g)
    return image, PrimitivePack(p, [1] + [0] * (K - 1))


@pytest.mark.parametrize('three', [False, True])
def test_frame_assembly_of_the_vp_dump(three):
    from vpn_amd import Visualizer
    from vpn_amd.modules.visualize import _image_block
    image, pack = _cpu_scene()
    log = []
    fr = Visualizer.frames_vp_meshes(image, pack, dist=2.0, is_three_elev=three, render=_fake_render(log))
    E = 3 if three else 1
    assert fr.shape == (12, 256, (2 + E) * 256, 3) and fr.dtype == torch.uint8
    assert len(log) == 1 and len(log[0].views) == 1 + 12 * E            # one render call; the direct pose is rendered once
    block = _image_block(image, 256)
    for f in range(12):
        assert torch.equal(fr[f, :, :256], block)                       # the image in column 0
        assert fr[f, 0, 256].tolist() == [0, 1, 20] and torch.equal(fr[f, :, 256:512], fr[0, :, 256:512])     # direct pose
        for e, elev in enumerate((-30, 0, 30) if three else (0,)):      # view order: azim, then elev
            assert fr[f, 100, (2 + e) * 256 + 7].tolist() == [f, elev // 30 + 1, 20]
    # the resize is bilinear interpolation of the float image, quantised like every other pixel
    want = torch.nn.functional.interpolate(image[None], size=(256, 256), mode='bilinear', align_corners=False)[0]
    assert torch.equal(block, (want.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0))


def test_frame_assembly_of_the_mesh_and_refine_dumps():
    from vpn_amd import TriangleMesh, Visualizer, config
    from geom_util import uv_sphere_386
    image, _ = _cpu_scene()
    v, f = uv_sphere_386(0.5)
    mesh = TriangleMesh(v, f)
    log = []
    fr = Visualizer.frames_mesh_gif(image, mesh, 1.5, render=_fake_render(log))
    assert fr.shape == (12, 256, 4 * 256, 3) and len(log) == 1 and log[0].ambient == 1.0
    for fi in range(12):
        assert [fr[fi, 5, c * 256].tolist() for c in (1, 2, 3)] == [[fi, 0, 15], [fi, 1, 15], [fi, 2, 15]]     # elev -30, 0, 30
    cols = log[0].scene[3]
    assert cols.shape == (1, 386, 3) and float(cols.min()) == 0.0 and float(cols.max()) == 1.0                 # mesh.py:12-14
    fr = Visualizer.frames_mesh_3pose(image, mesh, 1.5, 30.0, 330.0, render=_fake_render(log))
    assert fr.shape == (1, 256, 4 * 256, 3)
    assert [fr[0, 5, c * 256].tolist() for c in (1, 2, 3)] == [[11, 2, 15], [0, 2, 15], [1, 2, 15]]            # (azim + 30 i) % 360
    # refine: [image, deformed direct, primitives, deformed, deformed in grey] at dist 1, elev 0
    meshes = [TriangleMesh(v * 0.3 + 0.2 * k, f) for k in range(3)]
    refined = torch.cat([m.vertices for m in meshes]) * 1.1
    log.clear()
    fr = Visualizer.frames_refine_vp_meshes(image, meshes, refined, render=_fake_render(log))
    assert fr.shape == (12, 256, 5 * 256, 3) and len(log) == 3
    assert all(j.ambient == config.VIS_REFINE_AMBIENT == 0.35 for j in log)
    assert [len(j.views) for j in log] == [13, 12, 12]
    for fi in range(12):
        assert fr[fi, 9, 256].tolist() == [0, 1, 10]
        assert [fr[fi, 9, c * 256].tolist() for c in (2, 3, 4)] == [[fi, 1, 10]] * 3
    deformed, prims, grey = log
    assert torch.equal(deformed.scene[1][0], refined) and deformed.scene[2].shape == (3 * 768, 3)
    assert int(deformed.scene[2][768:].min()) == 386                    # faces offset by the vertices before them
    assert torch.equal(grey.scene[3], torch.full((1, 3 * 386, 3), 0.5))
    pal = deformed.scene[3][0]
    assert torch.equal(pal[:386], pal[:1].expand(386, 3)) and not torch.equal(pal[0], pal[386])    # a vertex takes its primitive's colour
    with pytest.raises(ValueError):
        Visualizer.frames_refine_vp_meshes(image, meshes, refined[:-1], render=_fake_render(log))


def test_saved_files_reopen(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    from vpn_amd import Visualizer
    from vpn_amd.modules import visualize as M
    image, pack = _cpu_scene()
    fr = Visualizer.frames_vp_meshes(image, pack, render=_fake_render([]))
    path = str(tmp_path / 'a.gif')
    M.save_gif(fr, path)
    with Image.open(path) as im:
        assert im.n_frames == 12 and im.size == (3 * 256, 256) and im.info['duration'] == 300 and im.info['loop'] == 0
    from vpn_amd import TriangleMesh
    from geom_util import uv_sphere_386
    fr = Visualizer.frames_mesh_3pose(image, TriangleMesh(*uv_sphere_386(0.5)), 1.5, 0.0, 0.0, render=_fake_render([]))
    png = str(tmp_path / 'b.png')
    M.save_image(fr[0], png)
    with Image.open(png) as im:
        assert im.size == (4 * 256, 256)


def test_surface_matches_the_reference():
    import inspect
    import vpn_amd
    V = vpn_amd.Visualizer
    assert V is vpn_amd.modules.Visualizer is vpn_amd.modules.visualize.Visualizer
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(V.render_vp_meshes) == [('image', E), ('vp_meshes', E), ('save_name', E), ('dist', 2.0), ('is_three_elev', False)]
    assert sig(V.render_refine_vp_meshes) == [('image', E), ('vp_meshes', E), ('predict_vertices', E), ('save_name', E)]
    assert sig(V.render_mesh_gif) == [('image', E), ('mesh', E), ('save_name', E), ('dist', E)]
    assert sig(V.render_mesh_3pose) == [('image', E), ('mesh', E), ('save_name', E), ('dist', E), ('elev', E), ('azim', E)]
    assert sig(V.turntable) == [('obj', E), ('cams', E), ('image_size', 256), ('palette', None), ('ambient', 1.0), ('background', (0.0, 0.0, 0.0))]
    src = open(os.path.join(ROOT, 'volumetric-primitives-net_amd', 'modules', 'visualize.py')).read()
    assert re.findall(r'^(?:from|import) .*PIL.*$', src, flags=re.M) == []        # PIL is imported inside the save functions only
    assert src.count('from PIL import Image') == 2


@pytest.mark.parametrize('K', [1, 16, 20, 64])
def test_default_palette_has_K_distinct_rows(K):
    from vpn_amd.modules.visualize import default_palette
    pal = default_palette(K)
    assert pal.shape == (K, 3) and pal.dtype == torch.float32 and float(pal.min()) >= 0.0 and float(pal.max()) <= 1.0
    q = VR.quantise(torch.cat([pal, torch.zeros(1, 3)]))
    assert len({tuple(r) for r in q.tolist()}) == K + 1                 # distinct as bytes too, and none is the background


def test_arguments_are_validated_before_any_launch():
    from vpn_amd import Visualizer, ops
    image, pack = _cpu_scene(K=5)
    with pytest.raises(ValueError, match='palette has 4 colours for K = 5'):
        ops.vis_primitives(pack.params, [0] * 5, CAMS, torch.rand(4, 3), 64, 64)
    with pytest.raises(ValueError, match='palette has 4 colours for K = 5'):
        Visualizer.frames_vp_meshes(image, pack, palette=torch.rand(4, 3), render=_fake_render([]))
    with pytest.raises(ValueError, match='kinds'):
        ops.vis_primitives(pack.params, [0] * 4, CAMS, torch.rand(5, 3), 64, 64)
    with pytest.raises(ValueError, match='GPU only'):
        ops.vis_primitives(pack.params, [0] * 5, CAMS, torch.rand(5, 3), 64, 64)
    with pytest.raises(ValueError, match='float32'):
        ops.vis_primitives(pack.params.double(), [0] * 5, CAMS, torch.rand(5, 3), 64, 64)
    with pytest.raises(ValueError, match='colors'):
        ops.vis_mesh(torch.rand(1, 9, 3), torch.zeros(4, 3, dtype=torch.int32), torch.rand(1, 8, 3), CAMS, 64, 64)
    with pytest.raises(ValueError, match='int32'):
        ops.vis_mesh(torch.rand(1, 9, 3), torch.zeros(4, 3, dtype=torch.int64), torch.rand(1, 9, 3), CAMS, 64, 64)
    with pytest.raises(ValueError, match='GPU only'):
        ops.vis_mesh(torch.rand(1, 9, 3), torch.zeros(4, 3, dtype=torch.int32), torch.rand(1, 9, 3), CAMS, 64, 64)


def test_header_binding_and_library_agree_on_the_new_entries():
    import vpn_amd._lib as lib
    L = lib.lib()
    hdr = open(os.path.join(ROOT, 'include', 'vpn_hip.h')).read()
    assert L.vpn_abi_version() == lib.ABI_VERSION == int(re.search(r'#define VPN_ABI_VERSION (\d+)', hdr).group(1))
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('vpn_vis_primitives', 'vpn_vis_mesh', 'vpn_vis_mesh_workspace'):
        assert name in lib.SIGNATURES and hasattr(L, name)
        decl = re.search(r'\b%s\s*\(([^)]*)\)' % name, code).group(1)
        assert len(decl.split(',')) == len(lib.SIGNATURES[name][1]), name          # as many parameters as the binding passes
    assert L.vpn_vis_mesh_workspace(2, 37, 386) == 2 * 37 * 386 * 16 and L.vpn_vis_mesh_workspace(0, 1, 1) == 0
    f = ctypes.c_void_p(256)             # never dereferenced: every call below is refused before a launch
    prim = lambda **k: L.vpn_vis_primitives(k.get('params', f), f, f, k.get('pal', f), k.get('S', 1), k.get('K', 4), k.get('V', 3), 64,
                                            k.get('W', 64), k.get('amb', 1.0), 0.0, 0.0, 0.0, k.get('out', f), k.get('bytes', 3 * 64 * 64 * 3),
                                            k.get('pitch', 64 * 3), None, None)
    assert prim(params=None) == -1 and prim(pal=None) == -1 and prim(out=None) == -1 and prim(K=0) == -1 and prim(V=0) == -1
    assert prim(pitch=64 * 3 - 1) == -1 and prim(bytes=3 * 64 * 64 * 3 - 1) == -1 and prim(amb=1.5) == -1
    assert prim(K=513) == -2
    mesh = lambda **k: L.vpn_vis_mesh(f, f, k.get('colors', f), f, 1, k.get('P', 9), k.get('F', 4), 3, 64, 64, 1.0, 0.0, 0.0, 0.0,
                                      k.get('ws', f), f, k.get('bytes', 3 * 64 * 64 * 3), 64 * 3, None, None)
    assert mesh(colors=None) == -1 and mesh(ws=None) == -1 and mesh(ws=ctypes.c_void_p(260)) == -1 and mesh(P=0) == -1 and mesh(F=0) == -1
    assert mesh(bytes=100) == -1


def test_render_kernels_use_no_scratch():
    for kernel in ('vis_primitives_kernel', 'vis_project_kernel', 'vis_mesh_kernel'):
        r = _resources('visualize.hip', kernel)
        assert r['ScratchSize'] == 0, (kernel, r)
    assert _resources('visualize.hip', 'vis_mesh_kernel')['LDS'] <= 16 * 1024          # 256 staged faces of 48 bytes
