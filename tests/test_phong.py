"""GPU checks of the Phong renderer (csrc/phong.hip, ops.phong_mesh, PhongRenderer) against tests/phong_ref.py.

The kernel is compared with the fp32 restatement on the inputs a .. e of phong_ref.cases(); which pixels are AMBIGUOUS is
taken from the fp64 restatement by the rule of DESIGN.md 4.10 (winner and runner-up depths within 1e-5 relative, or a pixel
centre within 1e-5 NDC of an edge of either) and those are left out: at most 0.1 % of an image, asserted.  Per image
(tests/test_phong_cpu.py prints them): a 0, b 3 3 0 2 3 3, c as b (phong_ref.ambiguous says why), d 0, e 0.

The kernel writes colours, not face ids: a pixel whose winner differs shows another face's normal (and possibly another
texel), which moves rgb by far more than rounding does.  The rgb bound is not a guess: the largest |fp32 - fp64| of the
restatement over the non-ambiguous pixels of these inputs is 2.236e-07 (phong_ref.RGB_FP32_ERROR = 2.24e-7; powf and the
normalisations dominate), and the kernel must stay within 4 times that, 8.96e-07, of the fp32 restatement -- the factor
covers the device's sinf, cosf and powf against the host's."""
import functools
import importlib.util
import json
import os

import pytest
import torch

import phong_ref as PR
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CAP = 1e-3
RGB_TOL = 4 * PR.RGB_FP32_ERROR         # 4 x 2.24e-7 = 8.96e-7


@functools.lru_cache(maxsize=None)
def _cases():
    return PR.cases()


@functools.lru_cache(maxsize=None)
def _case(name):
    verts, faces, uv, tex, cams, H, W = _cases()[name]
    return verts, faces, uv, tex, cams, H, W, PR.ref_phong(verts, faces, uv, tex, cams, H, W), PR.ambiguous(name, _cases())


def _render(name, **kw):
    from vpn_amd import ops
    verts, faces, uv, tex, cams, H, W, _ref, _amb = _case(name)
    kw = dict(dict(light=PR.LIGHT, material=PR.MATERIAL, shininess=PR.SHININESS), **kw)
    return ops.phong_mesh(verts.to(DEV), faces.to(DEV, torch.int32), uv.to(DEV), tex.to(DEV), cams.to(DEV), H, W, **kw)


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd', 'e'])
def test_render_equals_the_restatement(name):
    verts, faces, uv, tex, cams, H, W, ref, amb = _case(name)
    per_image = amb.flatten(2).sum(-1)
    print('%s: ambiguous pixels per image %s of %d' % (name, per_image.flatten().tolist(), H * W))
    assert int(per_image.max()) <= CAP * H * W, (name, per_image.tolist())
    got = _render(name).cpu()
    assert got.shape == (verts.shape[0], cams.shape[1], H, W, 3) and got.dtype == torch.float32
    clear = ~amb
    diff = (got - ref['rgb']).abs().amax(-1)
    hit = ref['winner'] >= 0
    print('%s: pixels that see a face %d, pixels that differ at all %d, outside the ambiguous set %d, max |kernel - fp32 restatement| there %.3e (bound %.3e)'
          % (name, int(hit.sum()), int((diff > 0).sum()), int((diff[clear] > 0).sum()), float(diff[clear].max()), RGB_TOL))
    # which pixels see a face at all, exactly (a drawn pixel is never black: ambient 0.7 of a texel with a positive channel)
    assert torch.equal((got.amax(-1) > 0)[clear], hit[clear])
    assert float(diff[clear].max()) <= RGB_TOL                          # 4 x the measured fp32 error of the restatement: 8.96e-07
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    if name == 'e':
        assert int(hit.sum()) == 0 and float(got.abs().max()) == 0.0
    if name == 'c':                                                     # the doubled mesh is the picture of the single one
        assert float((got - _render('b').cpu()).abs().amax(-1)[clear].max()) <= RGB_TOL


def test_ambient_only_material_returns_the_texels_exactly():
    verts, faces, uv, tex, cams, H, W, ref, amb = _case('b')
    got = _render('b', material=[[1, 1, 1], [0, 0, 0], [0, 0, 0]]).cpu()
    clear = ~amb & (ref['winner'] >= 0)
    want = torch.stack([tex[s][:, 0, :].t()[ref['texel'][s]] for s in range(tex.shape[0])])
    assert torch.equal(got[clear], want[clear])


def _mesh_b():
    from vpn_amd import TriangleMesh
    verts, faces, uv, tex, cams, H, W, _ref, _amb = _case('b')
    return TriangleMesh(verts[0].to(DEV), faces.to(DEV)), uv[:1].to(DEV), tex[:1].to(DEV), cams[0]


def test_renderer_outputs_alpha_views_and_no_host_synchronisation():
    from vpn_amd import PhongRenderer, VertexRenderer
    mesh, uv, tex, cams = _mesh_b()
    S = 64
    singles = [PhongRenderer.render(mesh, *cams[i].tolist(), uv, tex, img_size=S) for i in range(cams.shape[0])]
    rgb, alpha, norms = singles[0]
    assert rgb.shape == (1, S, S, 3) and alpha.shape == (1, S, S, 1) and norms.shape == (1, mesh.faces.shape[0], 3)
    assert float((norms.norm(dim=-1) - 1).abs().max()) < 1e-5
    # rgb is the kernel's picture of scene 0 of input b
    assert torch.equal(rgb[0], _render('b')[0, 0])
    # alpha is the operator SilhouetteLoss renders, bit for bit
    d, e, a = cams[0].tolist()
    want_alpha, _ = VertexRenderer.triangle_alpha(mesh, d, e, a, S, S)
    assert torch.equal(alpha[0, ..., 0], want_alpha[0])
    cams_dev = cams.to(DEV)
    vr, va = PhongRenderer.views(mesh, cams_dev, uv, tex, img_size=S)
    assert vr.shape == (3, S, S, 3) and va.shape == (3, S, S, 1)
    assert torch.equal(vr, torch.cat([s[0] for s in singles])) and torch.equal(va, torch.cat([s[1] for s in singles]))
    from vpn_amd import ops
    verts, faces, uvb, texb, camsb, H, W, _ref, _amb = _case('b')
    args = (verts.to(DEV), faces.to(DEV, torch.int32), uvb.to(DEV), texb.to(DEV), camsb.to(DEV), H, W)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        again = ops.phong_mesh(*args, light=PR.LIGHT, material=PR.MATERIAL, shininess=PR.SHININESS)
        vr2, va2 = PhongRenderer.views(mesh, cams_dev, uv, tex, img_size=S)
        r1 = PhongRenderer.render(mesh, d, e, a, uv, tex, img_size=S)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(again, _render('b')) and torch.equal(vr2, vr) and torch.equal(va2, va)
    assert torch.equal(r1[0], rgb) and torch.equal(r1[1], alpha)
    # without uv and texture: one random colour (phong_renderer.py:28-30), times 255 as the reference has it, so clamped
    torch.manual_seed(3)
    rr, _, _ = PhongRenderer.render(mesh, d, e, a, img_size=S)
    assert rr.shape == (1, S, S, 3) and torch.equal(rr.amax(-1) > 0, rgb.amax(-1) > 0)


def test_graph_capture_and_replay_reproduce_the_eager_bytes():
    from vpn_amd import ops
    verts, faces, uv, tex, cams, H, W, _ref, _amb = _case('b')
    args = (verts.to(DEV), faces.to(DEV, torch.int32), uv.to(DEV), tex.to(DEV), cams.to(DEV), H, W)
    kw = dict(light=PR.LIGHT, material=PR.MATERIAL, shininess=PR.SHININESS)
    eager = ops.phong_mesh(*args, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.phong_mesh(*args, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.phong_mesh(*args, **kw)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    buf = torch.full_like(eager, 7.0)
    assert ops.phong_mesh(*args, out=buf, **kw) is buf and torch.equal(buf, eager)


def test_example_writes_views_that_the_parsers_read_back(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    import numpy as np
    from vpn_amd import load_obj, obj_to_view_points
    from vpn_amd.modules.dataset import split_rgba
    spec = importlib.util.spec_from_file_location('generate_views', os.path.join(ROOT, 'examples', 'generate_views.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    torch.manual_seed(0)
    mesh, uv, tex = ex.default_mesh(DEV)
    n = ex.generate(mesh, uv, tex, str(tmp_path), n_views=20, img_size=64)
    assert n == 20 and len(os.listdir(tmp_path)) == 60
    for i in (0, 19):
        meta = json.load(open(tmp_path / ('meta_%.6d.json' % i)))
        assert 3.0 <= meta['dist'] <= 5.0 and -45.0 <= meta['elev'] <= 45.0 and 0.0 <= meta['azim'] <= 360.0
        with Image.open(tmp_path / ('img_%.6d.png' % i)) as im:
            assert im.mode == 'RGBA' and im.size == (64, 64)
            img = torch.from_numpy(np.array(im)).permute(2, 0, 1).float() / 255
        rgb, sil = split_rgba(img)
        assert rgb.shape == (3, 64, 64) and 0.01 < float(sil.mean()) < 0.5
        # a pixel centre inside a face has coverage >= 0.5 of that face, so of the union (the converse does not hold: next to
        # a vertex fan the soft union of many near faces is high outside the outline too)
        drawn = rgb.amax(0) > 0
        assert int(drawn.sum()) > 20 and float(sil[0][drawn].min()) >= 127 / 255
        v, f = load_obj(str(tmp_path / ('mesh_%.6d.obj' % i)))
        assert torch.equal(f, mesh.faces.cpu().long())
        want = obj_to_view_points(mesh.vertices[None], torch.tensor([meta['dist']], device=DEV), torch.tensor([meta['elev']], device=DEV),
                                  torch.tensor([meta['azim']], device=DEV))[0].cpu()
        assert torch.equal(v, want)
