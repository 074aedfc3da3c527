"""modules/render of the reference (vertex_renderer.py, phong_renderer.py) on the HIP rasters."""
import torch

from .. import config, ops
from ..ops import MeshRasterFunction, RasterFunction, faces_i32
from ..primitives import PrimitivePack, mesh_batches


def _as_batch(x, B, device):
    if isinstance(x, torch.Tensor):
        x = x.to(device=device, dtype=torch.float32).reshape(-1)
        return x.expand(B) if x.numel() == 1 else x
    return torch.full((B,), float(x), dtype=torch.float32, device=device)


class VertexRenderer:
    """Same entry point as the reference (vertex_renderer.py:10-26).  Differences, all forced
    by the reference rendering through kaolin (absent): `mesh` is a PrimitivePack or a mesh that
    carries one (what Meshing.*_meshing / compose_meshes return, so train.py:122-149,176 runs as written), a whole
    batch renders in one call, the camera travels with the call instead of mutating a
    module-global renderer (vertex_renderer.py:7,18), the image size is an argument instead of
    the hard-wired 128x128 (vertex_renderer.py:7), and the third output is the soft-min depth
    map instead of kaolin's face normals."""
    image_size = (config.IMG_SIZE, config.IMG_SIZE)
    sigma = config.RASTER_SIGMA
    gamma = config.RASTER_GAMMA
    z_far = config.RASTER_Z_FAR

    def __init__(self):
        pass

    @classmethod
    def render(cls, mesh, dist, elev, azim, colors=None, image_size=None):
        try:
            mesh = PrimitivePack.of(mesh)    # a pack, a Meshing-made mesh (train.py:122-149), or a list of them
        except TypeError:
            # a mesh without (valid) primitives: its triangles are rendered (vertex_renderer.py:20-24 as written)
            return cls.render_triangles(mesh, dist, elev, azim, colors, image_size)
        B = len(mesh)
        dev = mesh.params.device
        cam = torch.stack([_as_batch(dist, B, dev), _as_batch(elev, B, dev), _as_batch(azim, B, dev)], 1)
        H, W = image_size or cls.image_size
        alpha, depth = RasterFunction.apply(mesh.params, mesh.kinds, cam, H, W, cls.sigma, cls.gamma, cls.z_far)
        render_alphas = alpha[..., None]                       # (B,H,W,1)  vertex_renderer.py:24
        if colors is None:
            render_rgbs = render_alphas.expand(B, H, W, 3)     # colours default to ones (vertex_renderer.py:22)
        else:
            render_rgbs = render_alphas * colors.reshape(-1, 1, 1, 3)
        return render_rgbs, render_alphas, depth[..., None]

    mesh_sigma = config.MESH_RASTER_SIGMA

    @classmethod
    def triangle_alpha(cls, meshes, dist, elev, azim, H, W):
        """alpha (B,H,W) of triangle meshes (one mesh or a list, one per sample) and their batches."""
        batches = mesh_batches(meshes)
        B = sum(len(g) for g, _, _ in batches)
        dev = batches[0][1].device
        cam = torch.stack([_as_batch(dist, B, dev), _as_batch(elev, B, dev), _as_batch(azim, B, dev)], 1)
        out = [None] * B
        for idx, verts, faces in batches:
            # one topology (train_sphere.py: B copies of 386.obj): the whole camera tensor; otherwise rows picked as views
            # (an index tensor made from a host list would be a synchronising copy)
            cam_g = cam if idx == list(range(B)) else torch.stack([cam[i] for i in idx])
            a = MeshRasterFunction.apply(verts, faces_i32(faces, dev), cam_g.contiguous(), H, W, cls.mesh_sigma)
            for j, i in enumerate(idx):
                out[i] = a[j]
        return torch.stack(out), batches

    @classmethod
    def render_triangles(cls, mesh, dist, elev, azim, colors=None, image_size=None):
        """vertex_renderer.py:14-26 for a mesh given by vertices and faces: (rgb (B,H,W,3), alpha (B,H,W,1), unit face
        normals (B,F,3) as DIBRenderer returns them -- a list of per-mesh tensors if the topologies differ)."""
        H, W = image_size or cls.image_size
        alpha, batches = cls.triangle_alpha(mesh, dist, elev, azim, H, W)
        B = alpha.shape[0]
        render_alphas = alpha[..., None]
        if colors is None:
            render_rgbs = render_alphas.expand(B, H, W, 3)
        else:
            render_rgbs = render_alphas * colors.reshape(-1, 1, 1, 3)
        normals = [None] * B
        for idx, verts, faces in batches:
            tri = verts[:, faces.long(), :]
            nrm = torch.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1)
            nrm = nrm / nrm.norm(dim=-1, keepdim=True).clamp_min(1e-20)
            for j, i in enumerate(idx):
                normals[i] = nrm[j]
        face_norms = torch.stack(normals) if len(batches) == 1 else normals
        return render_rgbs, render_alphas, face_norms


class PhongRenderer:
    """phong_renderer.py:12-66 on csrc/phong.hip: a textured, lit render of a triangle mesh.  Same entry
    point, constants and helpers as the reference.  Differences, all forced by the reference rendering through kaolin
    (absent): pixel values follow the specification of DESIGN.md 4.11 (parity unpinned); alpha is the soft silhouette of
    VertexRenderer.triangle_alpha -- the operator SilhouetteLoss renders during training -- not DIB-R's; the texture
    lookup is nearest texel; `views` renders all cameras of a mesh in one launch and nothing is copied to the host."""
    material = ((0.7, 0.7, 0.7), (0.9, 0.9, 0.9), (0.3, 0.3, 0.3))          # phong_renderer.py:7  rows ambient, diffuse, specular
    light = (0.0, 10.0, -10.0)                                               # phong_renderer.py:8  in the camera basis (right, up, fwd)
    shininess = 1.0                                                          # phong_renderer.py:9

    def __init__(self):
        pass

    @classmethod
    def render(cls, mesh, dist, elev, azim, uv=None, texture=None, img_size=128):
        """-> rgb (1,S,S,3), alpha (1,S,S,1), unit world-space face normals (1,F,3)."""
        cls.check_mesh_parameters(mesh, uv, texture)
        dist, elev, azim = cls.check_camera_parameters(dist, elev, azim)
        if uv is None and texture is None:
            uv, texture = cls.get_random_color(mesh.vertices.size(0))
        rgb, alpha = cls.views(mesh, ((dist, elev, azim),), uv, texture, img_size)
        tri = mesh.vertices.detach()[mesh.faces.long(), :]
        nrm = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1)
        face_norms = (nrm / nrm.norm(dim=-1, keepdim=True).clamp_min(1e-20))[None]
        return rgb, alpha, face_norms

    @classmethod
    def views(cls, mesh, cams, uv, texture, img_size=128):
        """All cameras of one mesh in one launch (the loop of generate.py:150-161): cams [V,3] = (dist, elev deg, azim deg),
        a float32 device tensor or a host sequence (uploaded once and cached) -> rgb [V,S,S,3], alpha [V,S,S,1]."""
        cls.check_mesh_parameters(mesh, uv, texture)
        verts = mesh.vertices.detach().float().contiguous()
        dev = verts.device
        if not isinstance(cams, torch.Tensor) or not cams.is_cuda and dev.type == 'cuda':
            host = torch.as_tensor(cams, dtype=torch.float32)
            cams = ops.const_tensor(tuple(host.reshape(-1).tolist()), torch.float32, dev).reshape(host.shape)
        if cams.dim() != 2 or cams.size(1) != 3:
            raise ValueError('cams must be [V,3] = (dist, elev, azim), got %s' % (tuple(cams.shape),))
        cams = cams.contiguous()
        V, S = cams.size(0), int(img_size)
        rgb = ops.phong_mesh(verts[None], faces_i32(mesh.faces, dev), uv.to(dev), texture.to(dev), cams[None], S, S,
                             light=cls.light, material=cls.material, shininess=cls.shininess)[0]
        alpha, _ = VertexRenderer.triangle_alpha([mesh] * V, cams[:, 0], cams[:, 1], cams[:, 2], S, S)
        return rgb, alpha[..., None]

    @staticmethod
    def check_camera_parameters(dist, elev, azim):
        if isinstance(dist, torch.Tensor):                       # phong_renderer.py:41-48: a device scalar is read back
            dist = dist.item()
        if isinstance(elev, torch.Tensor):
            elev = elev.item()
        if isinstance(azim, torch.Tensor):
            azim = azim.item()
        return dist, elev, azim

    @staticmethod
    def check_mesh_parameters(mesh, uv, texture):
        assert hasattr(mesh, 'vertices') and hasattr(mesh, 'faces')          # phong_renderer.py:52 (kaolin's class is absent)
        if uv is None and texture is None:
            return

        assert uv.ndimension() == 3  # (B, N, 2)
        assert texture.ndimension() == 4  # (B, 3, TH, TW)
        assert uv.size(1) == mesh.vertices.size(0) and uv.size(2) == 2
        assert texture.size(1) == 3

    @staticmethod
    def get_random_color(vertex_num):
        """phong_renderer.py:62-66, drawn on the host in the reference's order (`views` moves the pair to the mesh)."""
        uv = torch.rand((1, vertex_num, 2))
        texture = torch.rand((1, 3, 1, 1)) * 255

        return uv, texture
