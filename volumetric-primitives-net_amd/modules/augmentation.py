"""modules/augmentation of the reference on the HIP kernels of csrc/augment.hip: the two augmentations train.py:234-237
runs on the device in front of the network, CutMix (cutmix.py) and the point mix-up of point_mixup.py:24-40.  Same
function names and positional parameters; every draw the reference makes inside is a keyword argument here, and where
it is not given it is taken from torch's CPU generator in the reference's order, so the same torch.manual_seed gives
the same cut, the same partners and the same mix-up ratio.

The augmented tensors are data: nothing is differentiable, no output requires grad, inputs that require grad are
rejected.  No call synchronises with the host (no .item() on a device tensor, no boolean-mask indexing, no device-to-host
copy), so the stage can be captured into a HIP graph when its draws are given.

The one deliberate deviation: a sample whose eligible list is EMPTY (its own points all below the cut, its partner's all
above) makes the reference raise (torch.randint(0, 0, ...), cutmix.py:49).  Raising needs a synchronisation; here the
sample keeps its own points and `count[b] == 0` (return_src=True) tells the caller.

The rest of point_mixup_data (point_mixup.py:12-21,43-86) -- cloud -> mesh -> image -> re-sampled cloud -- runs on the
device too, with a second deliberate deviation: the reference reconstructs a surface by ball pivoting
(open3d) and decomposes it into convex hulls with V-HACD (an external binary) per sample on the host; neither exists
here and neither could run inside a training loop.  points_to_meshes_and_colors REPLACES both by ops.hull_meshes: the
cloud is clustered and every cluster becomes the polytope of its support points along the directions of one template,
an inner approximation of the cluster's convex hull with all vertices on it.  All meshes of a batch share one face list,
so the render and the re-sampling are one launch each for the batch.  Parity with the reference's meshes is unpinned;
the atlas rule (uv = i / n + 0.01, one torch.rand(3) per hull) is convex_decomposition.py:32-58's.

Out of scope (host-side mesh processing through trimesh / an external binary): acd.py."""
import torch

from .. import config, ops
from .meshing import TriangleMesh

CUT_MIN, CUT_MAX = 0.3, 0.7              # cutmix.py:9
POINT_CUT_SCALE = 0.30769                # cutmix.py:12


def _philox_seed(seed):
    if seed is None:
        return int(torch.randint(0, 2 ** 62, (1,)).item())       # CPU generator: follows torch.manual_seed
    return int(seed)


def _check_cutmix(rgbs, silhouettes, view_center_points):
    assert rgbs.ndimension() == silhouettes.ndimension() == 4      # (B, C, H, W)   cutmix.py:53-55
    assert view_center_points.ndimension() == 3                    # (B, N, 3)


def cut_mix_data(rgbs: torch.Tensor, silhouettes: torch.Tensor, view_center_points: torch.Tensor, *, cut_ratio=None,
                 indices=None, seed=None, sample_base=0):
    """cutmix.py:5-21.  cut_ratio: the image cut ratio in [0, 1] (default: 0.3 + torch.rand(1) * 0.4); indices: the
    partner of each sample (default: torch.randperm(B), drawn after the ratio as there); seed / sample_base: the Philox
    key of the point draws (default seed: one torch.randint on the CPU generator, after the other two draws).
    Returns (rgbs, silhouettes, view_center_points) like the reference."""
    _check_cutmix(rgbs, silhouettes, view_center_points)
    B, _, _, W = rgbs.size()
    if cut_ratio is None:
        cut_ratio = CUT_MIN + torch.rand(1).item() * (CUT_MAX - CUT_MIN)
    cut_ratio = float(cut_ratio)
    img_cut_index = int(W * cut_ratio)
    point_cut_ratio = (0.5 - cut_ratio) * 2 * POINT_CUT_SCALE
    if indices is None:
        indices = torch.randperm(B)
    indices = ops.partner_indices(indices, B, rgbs.device)
    rgbs, silhouettes = ops.cutmix_images(rgbs, silhouettes, indices, img_cut_index)
    points = cut_mix_batch_points(view_center_points, indices, point_cut_ratio, seed=seed, sample_base=sample_base)
    return rgbs, silhouettes, points


def cut_mix_batch_points(view_center_points, indices, cut_ratio, *, seed=None, sample_base=0, return_src=False):
    """cutmix.py:24-36 for the whole batch in one launch.  cut_ratio: the z threshold, one float or a [B] tensor.
    return_src=True: (points, src [B,N] int32, count [B] int32) -- src[b,i] is the candidate out[b,i] copies (0..N-1 the
    sample's own points, N..2N-1 its partner's), count[b] the length of the eligible list (0: see the module text)."""
    assert view_center_points.ndimension() == 3
    B = view_center_points.size(0)
    indices = ops.partner_indices(indices, B, view_center_points.device)
    if isinstance(cut_ratio, torch.Tensor) and not cut_ratio.is_cuda:
        cut_ratio = cut_ratio.to(torch.float32).reshape(-1)
        cut_ratio = float(cut_ratio) if cut_ratio.numel() == 1 else cut_ratio.pin_memory().to(view_center_points.device,
                                                                                            non_blocking=True)
    out, src, count = ops.cutmix_points(view_center_points, indices, cut_ratio, _philox_seed(seed), sample_base)
    return (out, src, count) if return_src else out


def adjust_point_num(points: torch.Tensor, N: int, *, seed=None, sample_base=0, return_src=False):
    """cutmix.py:39-50: (N', 3) -> (N, 3): the points themselves, N of them without replacement, or N draws with
    replacement.  N' == 0 raises as the reference does (the shape is known on the host)."""
    assert points.ndimension() == 2      # (N', 3)
    if points.size(0) == 0:
        raise RuntimeError('adjust_point_num: no points to draw from (torch.randint: from >= to, cutmix.py:49)')
    out, src, _ = ops.cutmix_points(points[None], None, float('-inf'), _philox_seed(seed), sample_base, n_out=N)
    return (out[0], src[0]) if return_src else out[0]


def mixup_points(points: torch.Tensor, *, ratio=None, indices=None, eps=0.005, iters=100, return_assignment=False):
    """point_mixup.py:24-40: mixed[b] = (1 - r) * points[b] + r * points[p][assignment[b]], the B auctions of the
    reference's loop as one batched launch.  ratio default torch.rand(1), indices default torch.randperm(B), in that order.
    return_assignment=True: (mixed, dist [B,n], assignment [B,n] int32) of the auction points[b] -> points[p]."""
    assert points.ndimension() == 3      # (B, N, 3)   point_mixup.py:75-77
    assert points.size(-1) == 3
    B = points.size(0)
    if ratio is None:
        ratio = torch.rand(1).item()
    if indices is None:
        indices = torch.randperm(B)
    indices = ops.partner_indices(indices, B, points.device)
    mixed, dist, assignment = ops.mixup_points(points, indices, ratio, eps, iters)
    return (mixed, dist, assignment) if return_assignment else mixed


# ---- the rest of point_mixup_data: cloud -> mesh -> image -> re-sampled cloud (csrc/reconstruct.hip)

LLOYD_ITERS = 8
MIXUP_CAMERA = (1.0, 0.0, 0.0)           # point_mixup.py:62: dist 1, elev 0, azim 0
MIXUP_RESAMPLE = 2048                    # point_mixup.py:19
_ATLAS_UV = {}


def check_parameters(view_center_points: torch.Tensor):
    assert view_center_points.ndimension() == 3  # (B, N, 3)   point_mixup.py:73-75
    assert view_center_points.size(-1) == 3


def _atlas_uv(B, H, D, dev):
    """uv [B,H*D,2]: every vertex of hull i at i / H + 0.01 (convex_decomposition.py:39).  ONE [1,H*D,2] constant per
    (H, D, device), uploaded once and expanded over the batch: every row of every call is the same memory, read-only."""
    key = (H, D, str(dev))
    uv = _ATLAS_UV.get(key)
    if uv is None:
        if len(_ATLAS_UV) > 64:
            _ATLAS_UV.clear()
        row = torch.tensor([i / H + 0.01 for i in range(H)], dtype=torch.float64).to(torch.float32)      # torch.full's rounding
        host = row.repeat_interleave(D)[None, :, None].expand(1, H * D, 2).contiguous()
        uv = host.pin_memory().to(dev, non_blocking=True) if torch.device(dev).type == 'cuda' else host
        _ATLAS_UV[key] = uv
    return uv.expand(B, H * D, 2)


def _atlas_texture(B, H, colors, dev):
    """texture [B,3,1,H], texel i of mesh b = colors[b,i] ([B,H,3], host or device); default: one torch.rand(3) per hull,
    mesh after mesh, the draws of merge_meshes in the reference's order."""
    if colors is None:
        colors = torch.stack([torch.rand(3) for _ in range(B * H)]).reshape(B, H, 3)
    colors = torch.as_tensor(colors, dtype=torch.float32)
    if tuple(colors.shape) != (B, H, 3):
        raise ValueError('colors must be [%d,%d,3], one row per hull per mesh, got %s' % (B, H, tuple(colors.shape)))
    ops._augment_is_data(colors)
    if not colors.is_cuda and torch.device(dev).type == 'cuda':
        colors = colors.contiguous().pin_memory().to(dev, non_blocking=True)
    return colors.permute(0, 2, 1)[:, :, None, :].contiguous()


def points_to_mesh_batch(points: torch.Tensor, *, hull_num=None, iters=LLOYD_ITERS, colors=None, template=None,
                         return_parts=False):
    """The tensor-level twin of points_to_meshes_and_colors: points [B,N,3] -> (verts [B,P,3], faces [F,3] int32 shared by
    the batch, uv [B,P,2], texture [B,3,1,H]) with P = H * D; two launches (ops.hull_meshes), no host synchronisation.
    return_parts=True appends (labels [B,N] int32, support [B,P] int32).  faces and uv are cached constants shared by
    all calls (uv an expanded view of one [1,P,2] tensor): read-only for the caller."""
    check_parameters(points)
    H = int(config.DECOMPOSE_CONVEX_NUM if hull_num is None else hull_num)
    verts, faces, labels, support = ops.hull_meshes(points, H, iters, template)
    B, P, _ = verts.shape
    out = (verts, faces, _atlas_uv(B, H, P // H, verts.device), _atlas_texture(B, H, colors, verts.device))
    return out + (labels, support) if return_parts else out


def points_to_meshes_and_colors(points: torch.Tensor, *, hull_num=None, iters=LLOYD_ITERS, colors=None, template=None):
    """point_mixup.py:43-55: (meshes, uvs, textures), one entry per sample: a TriangleMesh of hull_num (default
    config.DECOMPOSE_CONVEX_NUM) merged hulls, its uv [1,P,2] and its texture [1,3,1,hull_num].  The meshes are views of
    one batch and share their face tensor; the faces and the uvs are cached constants shared by all calls, read-only for
    the caller.  See the module text for what replaces ball pivoting and V-HACD."""
    verts, faces, uv, texture = points_to_mesh_batch(points, hull_num=hull_num, iters=iters, colors=colors, template=template)
    B = verts.size(0)
    return ([TriangleMesh.from_tensors(verts[b], faces) for b in range(B)], [uv[b:b + 1] for b in range(B)],
            [texture[b:b + 1] for b in range(B)])


def _render_batch(verts, faces, uv, texture, img_size):
    """(rgbs [B,3,S,S], silhouettes [B,1,S,S]) of B meshes of one topology at MIXUP_CAMERA: one ops.phong_mesh launch pair
    and one soft-alpha batch, PhongRenderer.render's two pictures."""
    from .render import PhongRenderer, VertexRenderer
    B, S, dev = verts.size(0), int(img_size), verts.device
    cams = ops.const_tensor(MIXUP_CAMERA * B, torch.float32, dev).reshape(B, 3)
    rgb = ops.phong_mesh(verts, faces, uv, texture, cams[:, None, :], S, S, light=PhongRenderer.light,
                         material=PhongRenderer.material, shininess=PhongRenderer.shininess)[:, 0]
    alpha = ops.MeshRasterFunction.apply(verts.detach(), faces, cams, S, S, VertexRenderer.mesh_sigma)
    return rgb.permute(0, 3, 1, 2).contiguous(), alpha[:, None]


def meshes_to_imgs(meshes: list, uvs: list, textures: list, *, img_size=None):
    """point_mixup.py:58-70: PhongRenderer.render(mesh, 1, 0, 0, uv, texture) of every mesh -> (rgbs [B,3,S,S], silhouettes
    [B,1,S,S]), S = img_size (default config.IMG_SIZE).  Meshes of one topology (what points_to_meshes_and_colors returns)
    render as one batch; a list of mixed topologies falls back to the reference's per-mesh loop."""
    from ..primitives import mesh_batches
    from .render import PhongRenderer
    assert len(meshes) == len(uvs) == len(textures) and len(meshes) > 0
    S = int(config.IMG_SIZE if img_size is None else img_size)
    batches = mesh_batches(meshes)
    if len(batches) == 1 and len({tuple(t.shape) for t in textures}) == 1:
        _, verts, faces = batches[0]
        dev = verts.device
        return _render_batch(verts.detach().float(), ops.faces_i32(faces, dev), torch.cat([u.to(dev) for u in uvs]),
                             torch.cat([t.to(dev) for t in textures]), S)
    rgbs, silhouettes = [], []
    for i in range(len(meshes)):
        rgb, silhouette, _ = PhongRenderer.render(meshes[i], *MIXUP_CAMERA, uvs[i], textures[i], img_size=S)
        rgbs.append(rgb.permute(0, 3, 1, 2))
        silhouettes.append(silhouette.permute(0, 3, 1, 2))
    return torch.cat(rgbs), torch.cat(silhouettes)


def _mixup_batch(view_center_points, ratio, indices, colors, hull_num, iters, img_size, eps, emd_iters):
    check_parameters(view_center_points)
    mixed = mixup_points(view_center_points, ratio=ratio, indices=indices, eps=eps, iters=emd_iters)
    verts, faces, uv, texture, labels, support = points_to_mesh_batch(mixed, hull_num=hull_num, iters=iters, colors=colors,
                                                                      return_parts=True)
    S = int(config.IMG_SIZE if img_size is None else img_size)
    rgbs, silhouettes = _render_batch(verts, faces, uv, texture, S)
    return rgbs, silhouettes, dict(mixed=mixed, verts=verts, faces=faces, uv=uv, texture=texture, labels=labels, support=support)


def point_mixup_data(view_center_points: torch.Tensor, *, ratio=None, indices=None, colors=None, seed=None, sample_base=0,
                     hull_num=None, iters=LLOYD_ITERS, img_size=None, num_points=MIXUP_RESAMPLE, eps=0.005, emd_iters=100,
                     return_parts=False):
    """point_mixup.py:12-21: mix the clouds of the batch, rebuild a mesh from every mixed cloud, render it and sample it
    again -> (rgbs [B,3,S,S], silhouettes [B,1,S,S], new_points [B,num_points,3]).  Draws, in the reference's order when
    not given: ratio (torch.rand(1)), indices (torch.randperm(B)), colors ([B,hull_num,3]: torch.rand(3) per hull), seed
    (the Philox key of the surface samples; sample_base + b names mesh b: one torch.randint).  Eight launches plus the
    auction's, all on the current stream, no host synchronisation: with the draws given the call can be captured into a
    HIP graph.  return_parts=True appends a dict: mixed, verts, faces, uv, texture, labels, support, face_idx, bary."""
    rgbs, silhouettes, parts = _mixup_batch(view_center_points, ratio, indices, colors, hull_num, iters, img_size, eps, emd_iters)
    new_points, face_idx, bary = ops.sample_meshes(parts['verts'], parts['faces'], num_points, _philox_seed(seed), sample_base)
    if return_parts:
        parts.update(face_idx=face_idx, bary=bary)
        return rgbs, silhouettes, new_points, parts
    return rgbs, silhouettes, new_points


def generate_point_mixup_data(view_center_points: torch.Tensor, *, ratio=None, indices=None, colors=None, hull_num=None,
                              iters=LLOYD_ITERS, img_size=None, eps=0.005, emd_iters=100):
    """point_mixup.py:78-86, the data-set form (generate.py:42-66): (rgbs, silhouettes, meshes), the meshes a list of
    TriangleMesh (save_mesh writes the OBJ)."""
    rgbs, silhouettes, parts = _mixup_batch(view_center_points, ratio, indices, colors, hull_num, iters, img_size, eps, emd_iters)
    verts, faces = parts['verts'], parts['faces']
    return rgbs, silhouettes, [TriangleMesh.from_tensors(verts[b], faces) for b in range(verts.size(0))]
