"""modules/visualize of the reference (visualizer.py, vp_mesh.py, mesh.py, render.py) on csrc/visualize.hip: the visual
dumps every script of the reference writes.

    Visualizer.render_vp_meshes(image, vp_meshes, 'out.gif', dist=2.0, is_three_elev=False)     # train.py:293, test.py:124
    Visualizer.render_mesh_gif(image, mesh, 'out.gif', dist)                                    # train_sphere.py:149
    Visualizer.render_mesh_3pose(image, mesh, 'out.png', dist, elev, azim)                      # test_sphere.py:121
    Visualizer.render_refine_vp_meshes(image, vp_meshes, predict_vertices, 'out.gif')           # train_gcn.py:157

The reference renders one view per DIBRenderer call (13 to 37 per dump) and copies every one to the host
(visualize/render.py:18-21).  Here the views of a dump are rendered by one launch per kind of object straight into the frame
strip on the device (`frames_*`), and the save path is ONE device-to-host copy followed by PIL.

Tensor level, for tests, TensorBoard and batched dumps: `Visualizer.turntable` renders [S,V,H,W,3] uint8 of any set of
cameras; `Visualizer.frames_*` return the assembled uint8 [frames, H, cols * W, 3] of the method of the same name without
writing anything.  Neither synchronises with the host, and both can be captured into a HIP graph once a first call has
uploaded their (cached) view lists.

Deviations from the reference, all forced by kaolin's DIBRenderer / the trimesh texture atlas being absent:
  * pixel values follow this project's specification: hard z-buffered edges, no anti-aliasing;
  * a Meshing-made mesh renders from its primitives (exact ellipsoids and boxes, not their 128-vertex polyhedra); once its
    vertices were edited it renders its triangles with per-primitive vertex colours -- the rule of VertexRenderer.render;
  * the input image is resized with F.interpolate(mode='bilinear'), not PIL's BILINEAR filter (which also low-pass filters
    when it shrinks): the two differ by a few levels at edges;
  * the default palette is this project's (evenly spread hues for any K); the reference's 20-entry COLORS table
    (vp_mesh.py:7-11), which it indexes out of range for K > 20, can be passed as `palette`;
  * render_refine_vp_meshes: the reference shades through PhongRenderer with a texture atlas; here a vertex takes the
    colour of the primitive it came from and the shading is a headlight term on the face normal with
    ambient = config.VIS_REFINE_AMBIENT."""
import colorsys

import torch
import torch.nn.functional as F

from .. import config
from .. import ops
from ..primitives import PrimitivePack, mesh_batches

IMAGE_SIZE = 256                     # visualize/render.py:9
AZIMS = tuple(range(0, 360, 30))     # vp_mesh.py:25, mesh.py:20


def default_palette(K, device=None):
    """K colours of evenly spread hues [K,3] fp32 (two saturations and two values alternate, so that neighbours in index
    differ in more than hue).  On `device` when given (one cached tensor per (K, device)), else on the host."""
    rows = []
    for k in range(int(K)):
        r, g, b = colorsys.hsv_to_rgb(k / float(K), 0.9 if k % 2 == 0 else 0.55, 0.99 if k % 4 < 2 else 0.7)
        rows.append((round(r, 6), round(g, 6), round(b, 6)))
    if device is None:
        return torch.tensor(rows, dtype=torch.float32).reshape(-1, 3)
    return ops.const_tensor(tuple(rows), torch.float32, device)


def _vp_pack(vp_meshes):
    """The [1,K,10] pack behind the K single-primitive meshes of ONE sample (test.py:114-123), or behind a pack; None if a
    mesh has lost its primitives (edited vertices)."""
    if isinstance(vp_meshes, PrimitivePack):
        if len(vp_meshes) != 1:
            raise ValueError('a dump shows one sample: pass pack[b]')
        return vp_meshes
    packs = [getattr(m, 'primitives', None) for m in vp_meshes]
    if not packs:
        raise ValueError('empty list of primitive meshes')
    if any(not isinstance(p, PrimitivePack) for p in packs):
        return None
    kinds = [k for p in packs for k in ops.kinds_host(p.kinds)]
    return PrimitivePack(torch.cat([p.params[:1] for p in packs], 1), kinds)


def _vp_triangles(vp_meshes, palette):
    """(verts [1,P,3], faces [F,3] int32, colors [1,P,3]) of the K meshes composed as vp_mesh.py:35-70 does: vertex colour =
    the colour of the primitive (vp_mesh.py:35-45)."""
    verts, faces, cols, n = [], [], [], 0
    for i, m in enumerate(vp_meshes):
        verts.append(m.vertices)
        faces.append(m.faces + n)
        cols.append(palette[i].expand(m.vertices.size(0), 3))
        n += m.vertices.size(0)
    return torch.cat(verts)[None].float(), torch.cat(faces).to(torch.int32), torch.cat(cols)[None].contiguous()


def position_colors(verts):
    """(v - min) / (max - min) per axis over the vertices of each mesh (mesh.py:12-14), on the device of `verts`."""
    lo, hi = verts.min(dim=1, keepdim=True)[0], verts.max(dim=1, keepdim=True)[0]
    return (verts - lo) / (hi - lo)


def _image_block(image, size):
    """image [C,h,w] (or [h,w]) in [0,1] -> uint8 [size,size,3] as ToPILImage + resize give it, up to the filter."""
    img = image.detach().float()
    if img.dim() == 2:
        img = img[None]
    img = img[:3] if img.size(0) >= 3 else img[:1].expand(3, -1, -1)
    img = F.interpolate(img[None], size=(size, size), mode='bilinear', align_corners=False)[0]
    return (img.clamp(0.0, 1.0) * 255.0).to(torch.uint8).permute(1, 2, 0)


class _Job:
    """One render launch of a dump: what to draw, how, and where each view goes: views = [(dist, elev, azim, frame, col)]."""

    def __init__(self, scene, views, ambient=1.0):
        self.scene, self.views, self.ambient = scene, views, ambient


def hip_render(job, frames, size, background=(0.0, 0.0, 0.0)):
    """Render the views of `job` into their blocks of frames [n, size, cols * size, 3] on the device."""
    n, H, row, _ = frames.shape
    pitch = row * 3
    dev = frames.device
    offs = tuple(f * H * pitch + c * size * 3 for _, _, _, f, c in job.views)
    cams = ops.const_tensor(tuple((float(d), float(e), float(a)) for d, e, a, _, _ in job.views), torch.float32, dev)[None]
    kind = job.scene[0]
    if kind == 'primitives':
        _, params, kinds, palette = job.scene
        ops.vis_primitives(params, kinds, cams, palette, size, size, ambient=job.ambient, background=background, out=frames,
                           pitch=pitch, view_offset=offs)
    else:
        _, verts, faces, colors = job.scene
        ops.vis_mesh(verts, faces, colors, cams, size, size, ambient=job.ambient, background=background, out=frames, pitch=pitch,
                     view_offset=offs)


def assemble(image, n_frames, cols, jobs, once=(), size=IMAGE_SIZE, render=None):
    """The frame strip of a dump: uint8 [n_frames, size, cols * size, 3] on the device of `image`.  Column 0 of every frame
    is the input image; every job is one render call; `once` lists the columns whose block was rendered into frame 0 only
    (the direct pose) and is copied to the other frames on the device.  render: the function that draws a job (tests inject
    one that runs on the CPU); default: the HIP kernels."""
    render = render or hip_render
    frames = torch.empty((n_frames, size, cols * size, 3), dtype=torch.uint8, device=image.device)
    frames[:, :, :size] = _image_block(image, size)
    for job in jobs:
        render(job, frames, size)
    for c in once:
        frames[1:, :, c * size:(c + 1) * size] = frames[0, :, c * size:(c + 1) * size]
    return frames


def _mesh_scene(mesh):
    verts = mesh.vertices.detach().float()
    verts = (verts[None] if verts.dim() == 2 else verts).contiguous()
    return verts, ops.faces_i32(mesh.faces, verts.device)


def save_gif(frames, save_name):
    """ONE device-to-host copy of the frame tensor, then PIL as vp_mesh.py:32 uses it."""
    from PIL import Image
    host = frames.cpu().numpy()
    imgs = [Image.fromarray(f, 'RGB') for f in host]
    imgs[0].save(save_name, format='GIF', append_images=imgs[1:], save_all=True, duration=300, loop=0)


def save_image(frame, save_name):
    from PIL import Image
    Image.fromarray(frame.cpu().numpy(), 'RGB').save(save_name)             # mesh.py:49-50


class Visualizer:
    """The four static methods of visualizer.py:7-25 with the reference's names, argument orders and defaults, the
    `frames_*` function behind each, and `turntable`."""
    image_size = IMAGE_SIZE

    # ---- tensor level
    @staticmethod
    @torch.no_grad()
    def turntable(obj, cams, image_size=IMAGE_SIZE, palette=None, ambient=1.0, background=(0.0, 0.0, 0.0)):
        """uint8 [S,V,H,W,3]: every sample of `obj` from every camera, in one render call.
        obj: a PrimitivePack, a Meshing-made mesh or a list of them, one per sample (rendered from their primitives, coloured
        by `palette` [>= K,3], default default_palette(K)); or triangle meshes of one topology without primitives (vertex
        colours: `palette` as [S,P,3] / [P,3], default position colours, mesh.py:12-14).
        cams: [S,V,3] or [V,3] (the same views for every sample) = (dist, elev deg, azim deg): a float32 device tensor, or a
        host sequence (uploaded once and cached).  image_size: an int or (H, W)."""
        H, W = (image_size, image_size) if isinstance(image_size, int) else image_size
        try:
            pack = PrimitivePack.of(obj)
        except TypeError:
            pack = None
        if pack is not None:
            params = pack.params.detach().float().contiguous()
            S, K, dev = params.size(0), params.size(1), params.device
            pal = default_palette(K, dev) if palette is None else palette
            return ops.vis_primitives(params, pack.kinds, Visualizer._cams(cams, S, dev), pal, H, W, ambient=ambient,
                                      background=background)
        batches = mesh_batches(obj)
        if len(batches) != 1:
            raise ValueError('turntable renders meshes of one topology in one call; got %d topologies' % len(batches))
        _, verts, faces = batches[0]
        verts = verts.detach().float().contiguous()
        S, dev = verts.size(0), verts.device
        colors = position_colors(verts) if palette is None else (palette[None].expand_as(verts) if palette.dim() == 2 else palette)
        return ops.vis_mesh(verts, ops.faces_i32(faces, dev), colors.contiguous(), Visualizer._cams(cams, S, dev), H, W,
                            ambient=ambient, background=background)

    @staticmethod
    def _cams(cams, S, dev):
        if not isinstance(cams, torch.Tensor) or not cams.is_cuda and dev.type == 'cuda':
            host = torch.as_tensor(cams, dtype=torch.float32)                # a host sequence or tensor: uploaded once, cached
            cams = ops.const_tensor(tuple(host.reshape(-1).tolist()), torch.float32, dev).reshape(host.shape)
        if cams.dim() == 2:
            cams = cams[None].expand(S, -1, -1)
        return cams.contiguous()

    @staticmethod
    @torch.no_grad()
    def frames_vp_meshes(image, vp_meshes, dist=2.0, is_three_elev=False, palette=None, render=None):
        """vp_mesh.py:14-32: 12 frames [image, direct pose (dist, 0, 0), one view per elev] -> uint8 [12, 256, (2 + E) 256, 3]."""
        elevs = (-30, 0, 30) if is_three_elev else (0,)                      # vp_mesh.py:21
        views = [(dist, 0, 0, 0, 1)]                                         # the direct pose, once (vp_mesh.py:24)
        for f, azim in enumerate(AZIMS):
            views += [(dist, elev, azim, f, 2 + e) for e, elev in enumerate(elevs)]
        scene = Visualizer._vp_scene(vp_meshes, palette)
        return assemble(image.to(scene[1].device), len(AZIMS), 2 + len(elevs), [_Job(scene, views)], once=(1,), render=render)

    @staticmethod
    def _vp_scene(vp_meshes, palette):
        pack = _vp_pack(vp_meshes)
        dev = pack.params.device if pack is not None else vp_meshes[0].vertices.device
        K = pack.params.size(1) if pack is not None else len(vp_meshes)
        pal = default_palette(K, dev) if palette is None else palette
        if pal.shape[0] < K:
            raise ValueError('the palette has %d colours for K = %d primitives' % (pal.shape[0], K))
        if pack is not None:
            return ('primitives', pack.params.detach().float().contiguous(), pack.kinds, pal)
        return ('mesh',) + _vp_triangles(vp_meshes, pal)                     # edited vertices: the triangles are what there is

    @staticmethod
    @torch.no_grad()
    def frames_mesh_gif(image, mesh, dist, render=None):
        """mesh.py:7-27: 12 frames [image, elev -30, 0, 30] with position colours -> uint8 [12, 256, 4 * 256, 3]."""
        verts, faces = _mesh_scene(mesh)
        views = [(dist, elev, azim, f, 1 + e) for f, azim in enumerate(AZIMS) for e, elev in enumerate(range(-30, 60, 30))]
        return assemble(image.to(verts.device), len(AZIMS), 4, [_Job(('mesh', verts, faces, position_colors(verts)), views)], render=render)

    @staticmethod
    @torch.no_grad()
    def frames_mesh_3pose(image, mesh, dist, elev, azim, render=None):
        """mesh.py:30-50: one frame [image, azim, azim + 30, azim + 60] -> uint8 [1, 256, 4 * 256, 3]."""
        verts, faces = _mesh_scene(mesh)
        views = [(dist, elev, (azim + i * 30) % 360, 0, 1 + i) for i in range(3)]
        return assemble(image.to(verts.device), 1, 4, [_Job(('mesh', verts, faces, position_colors(verts)), views)], render=render)

    @staticmethod
    @torch.no_grad()
    def frames_refine_vp_meshes(image, vp_meshes, predict_vertices, palette=None, render=None):
        """vp_mesh.py:73-92: 12 frames [image, deformed mesh direct pose, primitives, deformed mesh, deformed mesh in one
        grey] at dist 1, elev 0 -> uint8 [12, 256, 5 * 256, 3].  predict_vertices [P,3] or [1,P,3]: the refined vertices of
        the composed mesh, in the vertex order of vp_meshes."""
        if isinstance(vp_meshes, PrimitivePack):
            raise ValueError('the refine dump needs the K primitive meshes (their faces carry the deformed vertices)')
        amb = config.VIS_REFINE_AMBIENT
        scene = Visualizer._vp_scene(vp_meshes, palette)
        K, dev = len(vp_meshes), scene[1].device
        pal = default_palette(K, dev) if palette is None else palette
        _, faces, colors = _vp_triangles(vp_meshes, pal)
        verts = predict_vertices.detach().float().reshape(1, -1, 3).contiguous()
        if verts.size(1) != colors.size(1):
            raise ValueError('%d refined vertices for a composed mesh of %d' % (verts.size(1), colors.size(1)))
        turn = lambda col: [(1.0, 0, azim, f, col) for f, azim in enumerate(AZIMS)]
        jobs = [_Job(('mesh', verts, faces, colors), [(1.0, 0, 0, 0, 1)] + turn(3), amb),        # direct pose once + turntable
                _Job(scene, turn(2), amb),
                _Job(('mesh', verts, faces, torch.full_like(colors, 0.5)), turn(4), amb)]        # vp_mesh.py:79: texture 0.5
        return assemble(image.to(dev), len(AZIMS), 5, jobs, once=(1,), render=render)

    # ---- the reference's surface (visualizer.py:7-25)
    @staticmethod
    def render_vp_meshes(image: torch.Tensor, vp_meshes: list, save_name: str, dist: float = 2.0, is_three_elev: bool = False):
        save_gif(Visualizer.frames_vp_meshes(image, vp_meshes, dist=dist, is_three_elev=is_three_elev), save_name)

    @staticmethod
    def render_refine_vp_meshes(image: torch.Tensor, vp_meshes: list, predict_vertices: torch.Tensor, save_name: str):
        save_gif(Visualizer.frames_refine_vp_meshes(image, vp_meshes, predict_vertices), save_name)

    @staticmethod
    def render_mesh_gif(image: torch.Tensor, mesh, save_name: str, dist: float):
        save_gif(Visualizer.frames_mesh_gif(image, mesh, dist), save_name)

    @staticmethod
    def render_mesh_3pose(image: torch.Tensor, mesh, save_name: str, dist: float, elev: float, azim: float):
        save_image(Visualizer.frames_mesh_3pose(image, mesh, dist, elev, azim)[0], save_name)
