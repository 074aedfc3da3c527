"""The Phong renderer's specification restated in pure PyTorch on the CPU, in fp32 or fp64 (tests only).

Which face a pixel sees is visualize_ref.ref_mesh itself (the mesh rule of DESIGN.md 4.10: projection, inside rule, nearest
face, lowest face on equal depths, and the fp64 ambiguity mask at tol = 1e-5), called with (u, v, 0) as the vertex
"colours": its `base` is then the texture coordinate interpolated by the colour rule, in the colour rule's summation order.
What is added here is the shading of the winning face: nearest-texel lookup, unit face normal turned towards the eye, the
light given in the camera basis, ambient + diffuse + specular, clamped.  Every operation is written out in the order the
kernel uses."""
import torch

import visualize_ref as VR
from oracle import vpn_oracle as O

MATERIAL = ((0.7, 0.7, 0.7), (0.9, 0.9, 0.9), (0.3, 0.3, 0.3))      # phong_renderer.py:7
LIGHT = (0.0, 10.0, -10.0)                                           # phong_renderer.py:8
SHININESS = 1.0                                                      # phong_renderer.py:9


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def ref_phong(verts, faces, uv, texture, cams, H, W, light=LIGHT, material=MATERIAL, shininess=SHININESS, dtype=torch.float32,
              tol=0.0):
    """verts [S,P,3], faces [F,3], uv [S,P,2], texture [S,3,TH,TW], cams [S,V,3] -> dict of [S,V,H,W(,3)] tensors:
    winner (-1: no face), depth, ambiguous, uv (interpolated), texel (ty * TW + tx), cosT, cosA and rgb."""
    dt = dtype
    S, V = verts.shape[0], cams.shape[1]
    TH, TW = texture.shape[2], texture.shape[3]
    r = VR.ref_mesh(verts, faces, torch.cat([uv, torch.zeros_like(uv[..., :1])], -1), cams, H, W, dtype=dt, tol=tol)
    verts, texture, cams = verts.to(dt), texture.to(dt), cams.to(dt)
    faces = faces.long()
    light = torch.as_tensor(light, dtype=torch.float32).to(dt)
    material = torch.as_tensor(material, dtype=torch.float32).to(dt)
    px, py = O.pixel_grid(H, W, dt)
    out = {k: [] for k in ('texel', 'cosT', 'cosA', 'rgb')}
    for s in range(S):
        for vi in range(V):
            _eye, right, up, fwd = (x[0] for x in O.camera_basis(cams[s, vi:vi + 1], dt))
            win = r['winner'][s, vi]
            hit = win >= 0
            u, v = r['base'][s, vi, ..., 0], r['base'][s, vi, ..., 1]
            tx = torch.floor(u * TW).clamp(0, TW - 1).nan_to_num(0.0).long()
            ty = torch.floor(v * TH).clamp(0, TH - 1).nan_to_num(0.0).long()
            tex = texture[s][:, ty, tx].permute(1, 2, 0)                 # [H,W,3]
            ray = (fwd[None, None, :] + px[None, :, None] * right[None, None, :]) + py[:, None, None] * up[None, None, :]
            d = ray / torch.sqrt(_dot(ray, ray))[..., None]
            fw = faces[win.clamp_min(0)]
            pa, pb, pc = verts[s][fw[..., 0]], verts[s][fw[..., 1]], verts[s][fw[..., 2]]
            e, g = pb - pa, pc - pa                                      # the cross product written out: every product rounded by itself
            n = torch.stack([e[..., 1] * g[..., 2] - e[..., 2] * g[..., 1], e[..., 2] * g[..., 0] - e[..., 0] * g[..., 2],
                             e[..., 0] * g[..., 1] - e[..., 1] * g[..., 0]], -1)
            n = n / torch.sqrt(_dot(n, n)).clamp_min(1e-20)[..., None]
            n = torch.where((_dot(n, d) > 0)[..., None], -n, n)
            l = (light[0] * right + light[1] * up) + light[2] * fwd
            l = l / torch.sqrt(_dot(l, l)).clamp_min(1e-20)
            cosT = _dot(n, l.expand_as(n)).clamp(0.0, 1.0)
            refl = (2.0 * cosT)[..., None] * n - l
            cosA = (-_dot(refl, d)).clamp(0.0, 1.0)
            spec = torch.pow(cosA, torch.tensor(shininess, dtype=dt))
            rgb = (tex * (material[0] + material[1] * cosT[..., None]) + material[2] * spec[..., None]).clamp(0.0, 1.0)
            rgb = torch.where(hit[..., None], rgb, torch.zeros_like(rgb))
            for key, val in zip(('texel', 'cosT', 'cosA', 'rgb'), (ty * TW + tx, cosT, cosA, rgb)):
                out[key].append(val)
    res = {k: torch.stack(vals).reshape((S, V) + vals[0].shape) for k, vals in out.items()}
    res.update(winner=r['winner'], depth=r['depth'], ambiguous=r['ambiguous'], uv=r['base'][..., :2])
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_phong.py (GPU) -- built and analysed on the CPU by tests/test_phong_cpu.py as well

def _two_spheres():
    """Two uv_sphere() parts merged by merge_meshes (504 faces): S = 2 scenes with different vertices and textures."""
    from vpn_amd.modules.meshing import TriangleMesh, merge_meshes, uv_sphere
    v, f = uv_sphere()
    parts = [TriangleMesh(v * 0.45 + torch.tensor([0.0, 0.1, 0.35]), f), TriangleMesh(v * 0.35 + torch.tensor([0.1, -0.05, -0.4]), f)]
    mesh, uv, tex0 = merge_meshes(parts, colors=[[0.9, 0.2, 0.1], [0.1, 0.4, 0.8]])
    g = torch.Generator().manual_seed(7)
    verts = torch.stack([mesh.vertices, mesh.vertices * torch.tensor([1.1, 0.8, 1.0]) + 0.02 * torch.randn(mesh.vertices.shape, generator=g)])
    tex = torch.cat([tex0, torch.tensor([[0.3, 0.9, 0.5], [0.8, 0.7, 0.2]]).t().reshape(1, 3, 1, 2)])
    cams = torch.tensor([[3.0, 20.0, 37.0], [3.4, -25.0, 141.0], [4.0, 40.0, 263.0]])[None].repeat(2, 1, 1)
    return verts, mesh.faces, uv.repeat(2, 1, 1), tex, cams


def cases():
    """name -> (verts [S,P,3], faces [F,3], uv [S,P,2], texture [S,3,TH,TW], cams [S,V,3], H, W)."""
    out = {}
    # a: one triangle with a texture gradient over a 3 x 4 texture, 40 x 48: partial tiles in both directions
    tri = torch.tensor([[[0.0, -0.7, 0.9], [0.1, -0.6, -0.8], [-0.1, 0.8, 0.1]]])
    uv = torch.tensor([[[0.05, 0.1], [0.95, 0.2], [0.4, 0.9]]])
    tex = torch.rand(1, 3, 3, 4, generator=torch.Generator().manual_seed(3))
    out['a'] = (tri, torch.tensor([[0, 1, 2]]), uv, tex, torch.tensor([[[3.0, 10.0, 15.0]]]), 40, 48)
    # b: more than one 256-face pass, a 2-texel atlas
    verts, faces, uvb, texb, cams = _two_spheres()
    out['b'] = (verts, faces, uvb, texb, cams, 64, 64)
    # c: every face doubled in the opposite winding (ball_pivot.py:24-27): every pixel is a tie, the lowest face wins
    out['c'] = (verts, torch.cat([faces, faces[:, [0, 2, 1]]]), uvb, texb, cams, 64, 64)
    # d: face 0 behind the eye, face 1 crossing MESH_NEAR (a corner at depth 0.5 MESH_NEAR), face 2 drawn
    eye_x = 3.0
    vd = torch.tensor([[[eye_x + 1.0, -0.5, 0.6], [eye_x + 1.0, -0.5, -0.6], [eye_x + 1.0, 0.6, 0.0],
                        [eye_x - 0.5 * O.MESH_NEAR, 0.0, 0.0], [0.5, -0.4, 0.5], [0.5, 0.5, -0.5],
                        [0.0, -0.6, 0.7], [0.0, -0.6, -0.7], [0.0, 0.7, 0.0]]])
    uvd = torch.tensor([[[0.1, 0.5]] * 3 + [[0.5, 0.5]] * 3 + [[0.9, 0.5]] * 3])
    texd = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.2, 0.3, 1.0]]).t().reshape(1, 3, 1, 3)
    out['d'] = (vd, torch.tensor([[0, 1, 2], [3, 4, 5], [6, 7, 8]]), uvd, texd, torch.tensor([[[eye_x, 0.0, 0.0]]]), 64, 64)
    # e: the mesh of (a) far above the view: nothing is hit
    out['e'] = (tri + torch.tensor([0.0, 5.0, 0.0]), torch.tensor([[0, 1, 2]]), uv, tex, torch.tensor([[[3.0, 10.0, 15.0]]]), 40, 48)
    return out


def surface(winner, F):
    """Face ids with the two copies of a doubled face (f and f + F, input c) counted as one surface; -1 stays."""
    return torch.where(winner >= 0, winner % F, winner)


def ambiguous(name, all_cases=None):
    """The ambiguity mask of an input: the rule of DESIGN.md 4.10 on the fp64 restatement at tol = 1e-5.  Input c doubles
    every face of b in the opposite winding: the two copies of a face are ONE surface at one depth, so by the letter of the
    rule every pixel of c would be a depth tie.  Which copy wins is indeed open (their depths differ by rounding only), but
    both copies shade alike, so nothing visible hangs on it: c takes the mask of b, the same surfaces counted once."""
    verts, faces, uv, tex, cams, H, W = (all_cases or cases())['b' if name == 'c' else name]
    return VR.ref_mesh(verts, faces, torch.zeros_like(verts), cams, H, W, dtype=torch.float64, tol=VR.AMBIG)['ambiguous']


# Measured on the CPU by test_phong_cpu.test_gpu_inputs_ambiguity_and_fp32_error (run with -s), recorded in DESIGN.md 4.11:
# the largest |fp32 - fp64| of rgb over the non-ambiguous pixels of the inputs above.  The GPU test allows 4 times this.
RGB_FP32_ERROR = 2.24e-7        # measured 2.236e-07 (input b), rounded up in the third digit
