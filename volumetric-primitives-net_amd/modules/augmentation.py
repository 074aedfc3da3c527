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

The ACD-mix data of generate.py:108-173 (acd.py) runs on the device as well, with a third deliberate deviation (DESIGN.md
4.13): the hulls of the two objects are ops.hull_meshes' (as above), and trimesh.boolean.union is REPLACED by a sampled
union surface: candidates drawn on all augmented hulls survive unless they lie inside another kept hull, and the surviving
cloud is hulled again.  The reference's draws through Python's `random` (acd.py:59,70-72) are drawn from torch's CPU
generator instead, always (the reference skips random.randint when the coin says no), in the order stated at acd_mix_data."""
import collections

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


# ---- ACD-mix data: generate.py:108-173 with acd.py on the device (csrc/acdmix.hip)

ACD_HULL_NUM = 8                         # acd.py:24, generate.py:148
ACD_VIEWS = 20                           # generate.py:150
ACD_POINTS = 2048                        # acd_mix.py:73
ACD_UNION_POINTS = 2048                  # the size of the union-surface cloud that is hulled again
ACD_MARGIN = 1e-3                        # how deep inside another hull a candidate must lie to be dropped
ACD_TURNS = (90.0, -90.0, 0.0, 180.0, -180.0)      # acd.py:59

MeshBatch = collections.namedtuple('MeshBatch', ['vertices', 'faces'])      # [S,P,3] and the [F,3] int32 all samples share


def acd(points: torch.Tensor, hull_num: int = ACD_HULL_NUM, *, iters=LLOYD_ITERS, template=None):
    """acd.py:24-28 on a batch of clouds: points [B,N,3] -> hulls [B,hull_num,D,3], every hull the support polytope of one
    cluster along the template's D directions (ops.hull_meshes; what replaces V-HACD, see the module text)."""
    check_parameters(points)
    verts, _faces, _labels, _support = ops.hull_meshes(points, int(hull_num), iters, template)
    B = verts.size(0)
    return verts.reshape(B, int(hull_num), -1, 3)


def _augment_draws(S, O, H, coin, u_num, scale, turn, shift, u_hull):
    """The draws of acd.augment for O objects of H hulls per sample, sample after sample, object after object, each in the
    reference's order (acd.py:114-119): the coin and the number of the cut-out (:70-71), the keys of its choice (:72), the
    scale (:38), the turn (:59), the shift (:47).  A draw that is given is not drawn."""
    need = dict(coin=coin is None, u_num=u_num is None, u_hull=u_hull is None, scale=scale is None, turn=turn is None, shift=shift is None)
    d = dict(coin=torch.zeros(S, O, dtype=torch.int32), u_num=torch.zeros(S, O), u_hull=torch.zeros(S, O * H), scale=torch.zeros(S, O),
             turn=torch.zeros(S, O, dtype=torch.int32), shift=torch.zeros(S, O))
    for s in range(S):
        for o in range(O):
            if need['coin']:
                d['coin'][s, o] = int(torch.randint(0, 2, (1,)).item())
            if need['u_num']:
                d['u_num'][s, o] = torch.rand(1).item()
            if need['u_hull']:
                d['u_hull'][s, o * H:(o + 1) * H] = torch.rand(H)
            if need['scale']:
                d['scale'][s, o] = 0.8 + torch.rand(1).item() * 0.4                     # s ~ [0.8, 1.2]
            if need['turn']:
                d['turn'][s, o] = int(torch.randint(0, len(ACD_TURNS), (1,)).item())
            if need['shift']:
                d['shift'][s, o] = (torch.rand(1).item() - 0.5) / 5                     # t ~ [-0.1, 0.1]
    given = dict(coin=coin, u_num=u_num, scale=scale, turn=turn, shift=shift, u_hull=u_hull)
    return {k: (d[k] if need[k] else given[k]) for k in d}


def augment(hulls: torch.Tensor, *, coin=None, u_num=None, scale=None, turn=None, shift=None, u_hull=None):
    """acd.py:114-119 for the hulls of ONE object per sample: hulls [S,H,D,3] -> (augmented hulls [S,H,D,3], keep [S,H]
    int32).  A hull the cut-out removes stays in the tensor, collapsed onto its first vertex (keep == 0): the topology is
    fixed.  Draws ([S,1] each, u_hull [S,H]; see _augment_draws) come from torch's CPU generator when not given."""
    assert hulls.ndimension() == 4 and hulls.size(-1) == 3          # (S, H, D, 3)
    S, H = hulls.size(0), hulls.size(1)
    d = _augment_draws(S, 1, H, coin, u_num, scale, turn, shift, u_hull)
    group = ops.const_tensor((0,) * H, torch.int32, hulls.device)
    return ops.hull_augment(hulls, group, d['coin'], d['u_num'], d['scale'], d['turn'], d['shift'], d['u_hull'])


def _normalised(points):
    return points / points.amax(dim=(1, 2), keepdim=True)          # generate.py:128-129: vertices /= vertices.max()


def _acd_mix_cloud(points1, points2, draws, hull_num, iters, union_points, n_cand, margin, seed, sample_base, template, normalize):
    check_parameters(points1)
    check_parameters(points2)
    assert points1.size(0) == points2.size(0)
    ops._augment_is_data(points1, points2)
    p1, p2 = points1.detach().float(), points2.detach().float()
    if normalize:
        p1, p2 = _normalised(p1), _normalised(p2)
    h1 = acd(p1, hull_num, iters=iters, template=template)
    h2 = acd(p2, hull_num, iters=iters, template=template)
    return ops.acd_mix_points(h1, h2, draws['coin'], draws['u_num'], draws['scale'], draws['turn'], draws['shift'], draws['u_hull'],
                              union_points, seed, sample_base, n_cand=n_cand, margin=margin, template=template)


def acd_mix_meshes(points1: torch.Tensor, points2: torch.Tensor, *, coin=None, u_num=None, scale=None, turn=None, shift=None,
                   u_hull=None, colors=None, seed=None, sample_base=0, hull_num=ACD_HULL_NUM, mix_hull_num=ACD_HULL_NUM,
                   iters=LLOYD_ITERS, union_points=ACD_UNION_POINTS, n_cand=None, margin=ACD_MARGIN, template=None,
                   normalize=True, return_parts=False):
    """generate.py:125-148 for S pairs of objects given as clouds [S,N,3]: normalise, decompose each into hull_num hulls
    (acd), augment per object, merge, decompose the merge into mix_hull_num hulls with a texture atlas -> (MeshBatch(vertices
    [S,P,3], faces [F,3] int32), uv [S,P,2], texture [S,3,1,mix_hull_num]), through points_to_mesh_batch.  Draws when not
    given, from torch's CPU generator: the augment draws ([S,2] each, u_hull [S,2 hull_num]; _augment_draws), then one
    colour per hull mesh after mesh (colors [S,mix_hull_num,3]), then seed, the Philox key of the candidates (one
    torch.randint; sample_base + s names sample s).  return_parts=True appends ops.acd_mix_points' dict plus cloud and count."""
    S = points1.size(0)
    d = _augment_draws(S, 2, int(hull_num), coin, u_num, scale, turn, shift, u_hull)
    if colors is None:
        colors = torch.stack([torch.rand(3) for _ in range(S * int(mix_hull_num))]).reshape(S, int(mix_hull_num), 3)
    cloud, count, parts = _acd_mix_cloud(points1, points2, d, hull_num, iters, union_points, n_cand, margin, _philox_seed(seed),
                                         sample_base, template, normalize)
    verts, faces, uv, texture = points_to_mesh_batch(cloud, hull_num=mix_hull_num, iters=iters, colors=colors, template=template)
    out = (MeshBatch(verts, faces), uv, texture)
    if return_parts:
        parts.update(cloud=cloud, count=count)
        return out + (parts,)
    return out


def _acd_cameras(S, V, cams, dev):
    """cams [S,V,3] = (dist, elev, azim) on the device; drawn as generate.py:153-155 does, view after view, when not given."""
    if cams is None:
        rows = []
        for _ in range(S * V):
            dist = 3.0 + torch.rand(1).item() * 2
            elev = (torch.rand(1).item() - 0.5) * 90
            azim = torch.rand(1).item() * 360
            rows.append((dist, elev, azim))
        cams = torch.tensor(rows, dtype=torch.float32).reshape(S, V, 3)
    return ops._draw_tensor('cams', cams, (S, V, 3), torch.float32, dev)


def acd_mix_data(points1: torch.Tensor, points2: torch.Tensor, *, views=ACD_VIEWS, img_size=None, num_points=ACD_POINTS,
                 coin=None, u_num=None, scale=None, turn=None, shift=None, u_hull=None, colors=None, cams=None, seed=None,
                 gt_seed=None, sample_base=0, hull_num=ACD_HULL_NUM, mix_hull_num=ACD_HULL_NUM, iters=LLOYD_ITERS,
                 union_points=ACD_UNION_POINTS, n_cand=None, margin=ACD_MARGIN, template=None, normalize=True, return_parts=False):
    """generate.py:119-173 with ACDMixDataset.load_points (acd_mix.py:71-73) for S pairs of objects given as clouds
    [S,N,3] -> (rgba [S,V,4,I,I] (the Phong render and the soft silhouette, the img_*.png of :157-167), the mesh vertices
    in each view's frame [S,V,P,3] (mesh_*.obj, :164-168), gt_points [S,V,num_points,3] sampled on those meshes, dists,
    elevs, azims [S,V] (meta_*.json)), I = img_size (default config.IMG_SIZE), V = views.  The faces are
    parts['faces'] (return_parts=True appends acd_mix_meshes' dict plus faces, uv, texture, verts, cams, face_idx, bary).
    Draws when not given, from torch's CPU generator, in the reference's order as far as it has one: the augment draws of
    all samples (_augment_draws), one colour per hull mesh after mesh, the cameras (dist 3 .. 5, elev -45 .. 45, azim 0 ..
    360, :153-155) view after view; then the two Philox keys the reference has no counterpart of: seed (the candidates of the
    union surface) and gt_seed (the ground-truth points; mesh sample_base + s V + v).  All views of all scenes are one
    ops.phong_mesh launch pair, one silhouette batch, one obj_to_view_points and one sample_meshes; no host
    synchronisation: with the draws given the call can be captured into a HIP graph."""
    from .render import PhongRenderer, VertexRenderer
    from .transform import obj_to_view_points
    S, V = points1.size(0), int(views)
    d = _augment_draws(S, 2, int(hull_num), coin, u_num, scale, turn, shift, u_hull)
    if colors is None:
        colors = torch.stack([torch.rand(3) for _ in range(S * int(mix_hull_num))]).reshape(S, int(mix_hull_num), 3)
    cams = _acd_cameras(S, V, cams, points1.device)
    seed, gt_seed = _philox_seed(seed), _philox_seed(gt_seed)
    (verts, faces), uv, texture, parts = acd_mix_meshes(points1, points2, colors=colors, seed=seed, sample_base=sample_base,
                                                        hull_num=hull_num, mix_hull_num=mix_hull_num, iters=iters,
                                                        union_points=union_points, n_cand=n_cand, margin=margin, template=template,
                                                        normalize=normalize, return_parts=True, **d)
    I = int(config.IMG_SIZE if img_size is None else img_size)
    P = verts.size(1)
    rgb = ops.phong_mesh(verts, faces, uv, texture, cams, I, I, light=PhongRenderer.light, material=PhongRenderer.material,
                         shininess=PhongRenderer.shininess)                                     # [S,V,I,I,3]
    flat_cams = cams.reshape(S * V, 3)
    per_view = verts[:, None].expand(S, V, P, 3).reshape(S * V, P, 3)
    alpha = ops.MeshRasterFunction.apply(per_view, faces, flat_cams, I, I, VertexRenderer.mesh_sigma)          # [S*V,I,I]
    dists, elevs, azims = (flat_cams[:, k].contiguous() for k in range(3))
    centred = obj_to_view_points(per_view, dists, elevs, azims)                                 # generate.py:164-165
    gt_points, face_idx, bary = ops.sample_meshes(centred, faces, num_points, gt_seed, int(sample_base) * V)
    rgba = torch.cat([rgb.permute(0, 1, 4, 2, 3), alpha.reshape(S, V, 1, I, I)], 2)
    out = (rgba, centred.reshape(S, V, P, 3), gt_points.reshape(S, V, int(num_points), 3), dists.reshape(S, V), elevs.reshape(S, V),
           azims.reshape(S, V))
    if return_parts:
        parts.update(faces=faces, uv=uv, texture=texture, verts=verts, cams=cams, face_idx=face_idx.reshape(S, V, -1),
                     bary=bary.reshape(S, V, -1, 3))
        return out + (parts,)
    return out
