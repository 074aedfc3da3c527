"""CPU checks of the Phong renderer: the restatement (tests/phong_ref.py) against closed forms and against
visualize_ref's mesh rule, the atlas builder, the OBJ writer, argument validation, the agreement of header, binding and
built library, and the analysis of the inputs that tests/test_phong.py runs on the GPU.  No GPU."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

import phong_ref as PR
import visualize_ref as VR
from conftest import ROOT
from oracle import vpn_oracle as O
from test_kernel_budget_cpu import _resources

CAP = 1e-3


def test_hit_mask_is_the_mesh_rule_of_the_visualiser():
    verts, faces, uv, tex, cams, H, W = PR.cases()['b']
    r = PR.ref_phong(verts, faces, uv, tex, cams, H, W)
    m = VR.ref_mesh(verts, faces, torch.rand(verts.shape, generator=torch.Generator().manual_seed(0)), cams, H, W)
    assert int((m['winner'] >= 0).sum()) > 2000
    assert torch.equal(r['winner'], m['winner']) and torch.equal(r['depth'], m['depth'])
    # a pixel that sees no face is black; one that sees a face is not (ambient 0.7 of a texel with a positive channel)
    assert torch.equal(r['rgb'].amax(-1) > 0, m['winner'] >= 0)


def _facing_triangle():
    # in the plane x = 0, facing the camera at (2, 0, 0) (normal +x towards the eye); constant uv -> texel (ty 1, tx 2) of 2 x 3
    verts = torch.tensor([[[0.0, -0.5, 0.6], [0.0, -0.5, -0.6], [0.0, 0.6, 0.0]]])
    uv = torch.full((1, 3, 2), 0.75)
    tex = torch.rand(1, 3, 2, 3, generator=torch.Generator().manual_seed(1))
    return verts, torch.tensor([[0, 1, 2]]), uv, tex, torch.tensor([[[2.0, 0.0, 0.0]]])


def test_one_triangle_facing_the_camera_equals_the_closed_form():
    verts, faces, uv, tex, cams = _facing_triangle()
    H = 128
    texel = tex[0, :, 1, 2]
    amb, dif, spe = (torch.tensor(x) for x in PR.MATERIAL)
    r = PR.ref_phong(verts, faces, uv, tex, cams, H, H, light=(0.0, 0.0, -1.0))
    c = H // 2                                                          # the pixel whose centre is half a pixel from the optical axis
    assert int(r['winner'][0, 0, c, c]) == 0 and int(r['texel'][0, 0, c, c]) == 1 * 3 + 2
    # n = l = +x exactly, so cosT = 1 and r = n; cosA = cos(pixel ray, axis) = 1 / sqrt(1 + px^2 + py^2) >= 1 - (px^2 + py^2) / 2
    px, py = O.pixel_grid(H, H)
    slack = float(px[c] ** 2 + py[c] ** 2) / 2 * float(spe.max()) + 1e-6
    want = (texel * (amb + dif) + spe).clamp(0.0, 1.0)
    assert float(r['cosT'][0, 0, c, c]) == 1.0
    assert float((r['rgb'][0, 0, c, c] - want).abs().max()) <= slack, (r['rgb'][0, 0, c, c], want, slack)
    # ambient only: the texel, exactly, on every pixel that sees the face
    r1 = PR.ref_phong(verts, faces, uv, tex, cams, H, H, light=(0.0, 0.0, -1.0), material=[[1, 1, 1], [0, 0, 0], [0, 0, 0]])
    hit = r1['winner'][0, 0] >= 0
    assert int(hit.sum()) > 1000 and torch.equal(r1['rgb'][0, 0][hit], texel.expand(int(hit.sum()), 3))
    assert float(r1['rgb'][0, 0][~hit].abs().max()) == 0.0
    # no specular term for material[2] = 0: ambient + diffuse of the restatement's own cosT
    r0 = PR.ref_phong(verts, faces, uv, tex, cams, H, H, light=(0.3, 0.5, -1.0), material=[PR.MATERIAL[0], PR.MATERIAL[1], [0, 0, 0]])
    want0 = (texel * (amb + dif * r0['cosT'][0, 0][hit][:, None])).clamp(0.0, 1.0)
    assert torch.equal(r0['rgb'][0, 0][hit], want0)
    assert 0.5 < float(r0['cosT'][0, 0][hit].min()) < 1.0
    # ... and with it the image is brighter by specular * cosA^shininess
    rs = PR.ref_phong(verts, faces, uv, tex, cams, H, H, light=(0.3, 0.5, -1.0), shininess=3.0)
    want_s = (want0 + spe * (rs['cosA'][0, 0][hit] ** 3.0)[:, None]).clamp(0.0, 1.0)
    assert float((rs['rgb'][0, 0][hit] - want_s).abs().max()) <= 1e-6


def test_light_is_given_in_the_camera_basis_and_the_normal_faces_the_eye():
    verts, faces, uv, tex, _ = _facing_triangle()
    # the same triangle seen from the other side and in the other winding: n is turned towards the eye, the picture is lit alike
    front = PR.ref_phong(verts, faces, uv, tex, torch.tensor([[[2.0, 0.0, 0.0]]]), 64, 64)
    back = PR.ref_phong(verts, faces, uv, tex, torch.tensor([[[2.0, 0.0, 180.0]]]), 64, 64)
    flipped = PR.ref_phong(verts, faces[:, [0, 2, 1]], uv, tex, torch.tensor([[[2.0, 0.0, 0.0]]]), 64, 64)
    assert torch.equal(front['rgb'], flipped['rgb'])
    hit = front['winner'][0, 0] >= 0
    assert abs(float(front['cosT'][0, 0][hit].mean()) - float(back['cosT'][0, 0][back['winner'][0, 0] >= 0].mean())) < 1e-3
    # the reference's light (0, 10, -10): above and behind the camera, 45 degrees off the axis
    assert abs(float(front['cosT'][0, 0, 32, 32]) - math.cos(math.pi / 4)) < 1e-6


def _literal_atlas(meshes):
    """convex_decomposition.py:32-53, restated literally."""
    n, k, uv, tex = len(meshes), 0, [], []
    for i, m in enumerate(meshes):
        uv.append(torch.full((m.vertices.size(0), 2), i / n + 0.01))
        c = torch.rand(3)
        tex.append(torch.cat([torch.full((1, 1, 1), c[j].item()) for j in range(3)], 0))
        k += m.vertices.size(0)
    return torch.cat(uv)[None], torch.cat(tex, 2)[None]


def _three_parts():
    from vpn_amd.modules.meshing import TriangleMesh, uv_sphere
    v, f = uv_sphere()
    return [TriangleMesh(v * 0.3 + torch.tensor([0.0, 0.0, -0.7 + 0.7 * i]), f) for i in range(3)]


def test_atlas_renders_every_part_in_its_own_colour():
    from vpn_amd.modules.meshing import merge_meshes
    parts = _three_parts()
    colors = torch.tensor([[0.9, 0.1, 0.2], [0.2, 0.8, 0.3], [0.1, 0.3, 0.95]])
    mesh, uv, tex = merge_meshes(parts, colors=colors)
    P, F = parts[0].vertices.size(0), parts[0].faces.size(0)
    assert mesh.vertices.shape == (3 * P, 3) and mesh.faces.shape == (3 * F, 3) and uv.shape == (1, 3 * P, 2) and tex.shape == (1, 3, 1, 3)
    assert torch.equal(mesh.faces[F:2 * F], parts[1].faces + P) and int(mesh.faces[2 * F:].min()) == 2 * P
    assert torch.equal(tex[0, :, 0, :].t(), colors)
    cams = torch.tensor([[[3.0, 15.0, 10.0], [3.0, -20.0, 60.0]]])
    r = PR.ref_phong(mesh.vertices[None], mesh.faces, uv, tex, cams, 64, 64, material=[[1, 1, 1], [0, 0, 0], [0, 0, 0]])
    hit = r['winner'] >= 0
    part = r['winner'][hit] // F
    assert set(part.unique().tolist()) == {0, 1, 2}
    assert torch.equal(r['rgb'][hit], colors[part])                     # nothing blended: the colour of the part the face belongs to
    assert torch.equal(r['texel'][hit], part)
    # uv and texture are the reference's, and the default draws come in its order
    torch.manual_seed(11)
    want_uv, want_tex = _literal_atlas(parts)
    torch.manual_seed(11)
    _, got_uv, got_tex = merge_meshes(parts)
    assert torch.equal(got_uv, want_uv) and torch.equal(got_tex, want_tex)
    with pytest.raises(ValueError, match='colors'):
        merge_meshes(parts, colors=colors[:2])


def test_save_mesh_round_trips_through_load_obj(tmp_path):
    from vpn_amd import TriangleMesh, load_obj
    from vpn_amd.modules.meshing import uv_sphere
    v, f = uv_sphere()
    v = v * 0.37 + torch.tensor([0.1, -0.2, 1e-3])
    path = str(tmp_path / 'm.obj')
    TriangleMesh(v, f.int()).save_mesh(path)
    v2, f2 = load_obj(path)
    assert torch.equal(v2, v) and torch.equal(f2, f)
    lines = open(path).read().splitlines()
    assert lines[0].startswith('v ') and lines[-1].startswith('f ') and len(lines) == v.size(0) + f.size(0)
    assert min(int(t) for ln in lines if ln.startswith('f ') for t in ln.split()[1:]) == 1          # 1-based


def test_arguments_are_validated_before_any_launch():
    from vpn_amd import ops
    kw = dict(light=PR.LIGHT, material=PR.MATERIAL, shininess=1.0)
    verts, faces = torch.rand(1, 9, 3), torch.zeros(4, 3, dtype=torch.int32)
    uv, tex, cams = torch.rand(1, 9, 2), torch.rand(1, 3, 2, 2), torch.tensor([[[3.0, 0.0, 0.0]]])
    with pytest.raises(ValueError, match='uv'):
        ops.phong_mesh(verts, faces, torch.rand(1, 8, 2), tex, cams, 64, 64, **kw)
    with pytest.raises(ValueError, match='texture'):
        ops.phong_mesh(verts, faces, uv, torch.rand(1, 4, 2, 2), cams, 64, 64, **kw)
    with pytest.raises(ValueError, match='float32'):
        ops.phong_mesh(verts.double(), faces, uv, tex, cams, 64, 64, **kw)
    with pytest.raises(ValueError, match='int32'):
        ops.phong_mesh(verts, faces.long(), uv, tex, cams, 64, 64, **kw)
    with pytest.raises(ValueError, match='cams'):
        ops.phong_mesh(verts, faces, uv, tex, cams[0], 64, 64, **kw)
    with pytest.raises(ValueError, match='GPU only'):
        ops.phong_mesh(verts, faces, uv, tex, cams, 64, 64, **kw)


def test_surface_matches_the_reference():
    import vpn_amd
    R = vpn_amd.PhongRenderer
    assert R is vpn_amd.modules.PhongRenderer is vpn_amd.modules.render.PhongRenderer
    assert vpn_amd.modules.render.VertexRenderer is vpn_amd.VertexRenderer              # both classes behind modules.render
    assert vpn_amd.merge_meshes is vpn_amd.modules.merge_meshes is vpn_amd.modules.meshing.merge_meshes
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(R.render) == [('mesh', E), ('dist', E), ('elev', E), ('azim', E), ('uv', None), ('texture', None), ('img_size', 128)]
    assert sig(R.views) == [('mesh', E), ('cams', E), ('uv', E), ('texture', E), ('img_size', 128)]
    assert [list(r) for r in R.material] == [[0.7] * 3, [0.9] * 3, [0.3] * 3] and list(R.light) == [0, 10, -10] and R.shininess == 1
    assert (R.material, R.light, R.shininess) == (PR.MATERIAL, PR.LIGHT, PR.SHININESS)
    assert R.check_camera_parameters(torch.tensor(3.5), 10, torch.tensor([20.0])) == (3.5, 10, 20.0)
    mesh = vpn_amd.TriangleMesh(torch.rand(5, 3), torch.zeros(2, 3, dtype=torch.int64))
    R.check_mesh_parameters(mesh, None, None)
    R.check_mesh_parameters(mesh, torch.rand(1, 5, 2), torch.rand(1, 3, 1, 4))
    with pytest.raises(AssertionError):
        R.check_mesh_parameters(mesh, torch.rand(1, 4, 2), torch.rand(1, 3, 1, 4))
    torch.manual_seed(5)
    uv, tex = R.get_random_color(7)
    torch.manual_seed(5)
    assert torch.equal(uv, torch.rand((1, 7, 2))) and torch.equal(tex, torch.rand((1, 3, 1, 1)) * 255)


def test_header_binding_and_library_agree_on_the_new_entries():
    import vpn_amd._lib as lib
    L = lib.lib()
    hdr = open(os.path.join(ROOT, 'include', 'vpn_hip.h')).read()
    assert L.vpn_abi_version() == lib.ABI_VERSION == int(re.search(r'#define VPN_ABI_VERSION (\d+)', hdr).group(1)) == 9
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in ('vpn_phong_mesh', 'vpn_phong_mesh_workspace'):
        assert name in lib.SIGNATURES and hasattr(L, name)
        decl = re.search(r'\b%s\s*\(([^)]*)\)' % name, code).group(1)
        assert len(decl.split(',')) == len(lib.SIGNATURES[name][1]), name          # as many parameters as the binding passes
    assert L.vpn_phong_mesh_workspace(2, 20, 386) == 2 * 20 * 386 * 16 and L.vpn_phong_mesh_workspace(1, 0, 1) == 0
    f = ctypes.c_void_p(256)             # never dereferenced: every call below is refused before a launch
    call = lambda **k: L.vpn_phong_mesh(k.get('verts', f), f, k.get('uv', f), k.get('tex', f), f, k.get('light', f), k.get('mat', f),
                                        k.get('shin', 1.0), 1, k.get('P', 9), k.get('F', 4), k.get('V', 3), k.get('TH', 1), k.get('TW', 2),
                                        64, k.get('W', 64), k.get('ws', f), k.get('out', f), None)
    for bad in (dict(verts=None), dict(uv=None), dict(tex=None), dict(light=None), dict(mat=None), dict(ws=None), dict(out=None),
                dict(ws=ctypes.c_void_p(260)), dict(P=0), dict(F=0), dict(V=0), dict(TH=0), dict(TW=0), dict(W=0), dict(shin=-1.0),
                dict(shin=float('nan'))):
        assert call(**bad) == -1, bad
    assert call(W=16385) == -2 and call(TW=16385) == -2 and call(V=65536) == -2


def test_phong_kernels_use_no_scratch_and_the_walk_keeps_its_lds():
    for kernel in ('phong_project_kernel', 'phong_mesh_kernel'):
        r = _resources('phong.hip', kernel)
        assert r['ScratchSize'] == 0 and r.get('AGPRs', 0) == 0, (kernel, r)
    r = _resources('phong.hip', 'phong_mesh_kernel')
    assert r['LDS'] <= 16 * 1024 and r['VGPRs'] <= 96, r                # 256 staged faces of 48 bytes; five waves per SIMD or more


def test_gpu_inputs_ambiguity_and_fp32_error():
    """The inputs of tests/test_phong.py, analysed where no GPU is needed: at most 0.1 % of an image is ambiguous by the rule
    of DESIGN.md 4.10 (fp64 restatement, tol 1e-5), fp32 and fp64 restatements see the same face and the same texel
    everywhere else, and the largest rgb difference between them there is what phong_ref.RGB_FP32_ERROR records."""
    cases = PR.cases()
    worst = 0.0
    for name, (verts, faces, uv, tex, cams, H, W) in cases.items():
        r32 = PR.ref_phong(verts, faces, uv, tex, cams, H, W)
        amb = PR.ambiguous(name, cases)
        per_image = amb.flatten(2).sum(-1)
        r64 = PR.ref_phong(verts, faces, uv, tex, cams, H, W, dtype=torch.float64)
        clear = ~amb
        err = float((r32['rgb'].double() - r64['rgb']).abs().amax(-1)[clear].max())
        print('%s: ambiguous pixels per image %s (cap %.2f), pixels that see a face %d, max |fp32 - fp64| of rgb outside them %.3e'
              % (name, per_image.flatten().tolist(), CAP * H * W, int((r32['winner'] >= 0).sum()), err))
        assert int(per_image.max()) <= CAP * H * W, (name, per_image.tolist())
        F = cases['b'][1].shape[0] if name == 'c' else faces.shape[0]
        assert torch.equal(PR.surface(r32['winner'], F)[clear], PR.surface(r64['winner'], F)[clear])
        assert torch.equal(r32['texel'][clear & (r32['winner'] >= 0)], r64['texel'][clear & (r32['winner'] >= 0)])
        worst = max(worst, err)
    print('largest over the inputs %.3e, recorded %.3e, bound of the GPU test %.3e' % (worst, PR.RGB_FP32_ERROR, 4 * PR.RGB_FP32_ERROR))
    assert worst <= PR.RGB_FP32_ERROR
    # the inputs reach what they are there for
    vb, fb, uvb, tb, cb, H, W = cases['b']
    assert fb.shape[0] == 504 > 256 and vb.shape[0] == 2 and cb.shape[1] == 3 and tb.shape[-1] == 2
    rb = PR.ref_phong(vb, fb, uvb, tb, cb, H, W)
    assert set(rb['texel'][rb['winner'] >= 0].unique().tolist()) == {0, 1} and int(rb['winner'].max()) >= 256
    rc = PR.ref_phong(*cases['c'])
    clear = ~PR.ambiguous('b', cases)                                   # both copies shade alike: c is the picture of b
    assert torch.equal(rc['rgb'][clear], rb['rgb'][clear]) and torch.equal(PR.surface(rc['winner'], 504)[clear], rb['winner'][clear])
    assert int((rc['winner'] >= 504).sum()) > 0                         # ... though the second copy is the nearer one by rounding on some pixels
    rd = PR.ref_phong(*cases['d'])
    assert set(rd['winner'].unique().tolist()) == {-1, 2}               # neither the face behind the eye nor the one through the near plane
    pr = O.mesh_project(cases['d'][0], cases['d'][4][0])[0]
    assert float(pr[:3, 2].max()) < 0 and 0 < float(pr[3, 2]) <= O.MESH_NEAR < float(pr[4, 2])
    re_ = PR.ref_phong(*cases['e'])
    assert int(re_['winner'].max()) == -1 and float(re_['rgb'].abs().max()) == 0.0
    ra = PR.ref_phong(*cases['a'])
    assert ra['texel'][ra['winner'] >= 0].unique().numel() >= 8         # the lookup is exercised in both directions
