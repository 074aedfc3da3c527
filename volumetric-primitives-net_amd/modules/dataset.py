"""The on-disk formats either side of the hot path (row f4; modules/dataset/dataset.py of the reference): which
models belong to which split, the camera of every rendering, and how an RGBA rendering becomes the network input
and the GT silhouette.  The text parsers and split_rgba are host-side; prepare_images is the loader's image transform
(Resize, ColorJitter, ToTensor, the rotation of AUGMENT_3D['rotate'], the split, Normalize) for a whole batch on the
device, bit-exact to PIL (csrc/input.hip); MeshBatch / sample_gt_points / gt_points are the loader's point
half (_load_sample_points, dataset.py:42-46,161-165, and genre.py:66-74): a ragged batch of parsed meshes becomes the
canonical and view-centred GT point sets in three launches (csrc/gtpoints.hip).  The dataset class itself
(file discovery, OBJ parsing, PNG decoding) is out of scope; the device-side augmentations are in
modules/augmentation.py."""
import torch

from .. import _lib, config, ops

DIST_SCALE = 1.754                       # dataset.py:147: the stored camera distance is scaled by this factor
IMAGENET_MEAN = (0.485, 0.456, 0.406)    # dataset.py:126
IMAGENET_STD = (0.229, 0.224, 0.225)
JITTER_MIN, JITTER_MAX = 0.6, 1.4        # dataset.py:17: ColorJitter(brightness=0.4, saturation=0.4, contrast=0.4)


def parse_split_csv(text: str) -> dict:
    """ShapeNet's split.csv (`id,synsetId,subSynsetId,modelId,split`, dataset.py:98-106) ->
    {'train': [(synsetId, modelId), ...], 'test': [...]}; `val` rows are added to `train` after the train rows,
    the header and malformed rows are skipped."""
    rows = {'train': [], 'val': [], 'test': []}
    for line in text.splitlines():
        f = line.strip().split(',')
        if len(f) >= 5 and f[-1] in rows:
            rows[f[-1]].append((f[1], f[3]))
    return {'train': rows['train'] + rows['val'], 'test': rows['test']}


def parse_rendering_metadata(text: str):
    """rendering_metadata.txt of the ShapeNet renderings (one `azim elev 0 dist 25` line per view,
    dataset.py:141-151) -> (azims, elevs, dists) as lists of floats, dists already multiplied by 1.754.
    (The reference's pattern has no sign: it would read `-10` as `10`; signs are kept here.)"""
    azims, elevs, dists = [], [], []
    for line in text.splitlines():
        t = line.split()
        if len(t) >= 5 and t[2] == '0' and t[4] == '25':
            azims.append(float(t[0]))
            elevs.append(float(t[1]))
            dists.append(float(t[3]) * DIST_SCALE)
    return azims, elevs, dists


def split_rgba(img: torch.Tensor, normalize: bool = False):
    """An RGBA rendering as a (4,H,W) tensor in [0,1] (what ToTensor gives, dataset.py:116-117) ->
    rgb (3,H,W) and silhouette (1,H,W) = the alpha channel (dataset.py:123); optional ImageNet normalisation of
    the rgb part (dataset.py:125-126).  Batched (B,4,H,W) input works the same way."""
    assert img.size(-3) == 4
    rgb, sil = img[..., :3, :, :], img[..., 3:4, :, :]
    if normalize:
        mean = torch.tensor(IMAGENET_MEAN, dtype=rgb.dtype, device=rgb.device).view(3, 1, 1)
        std = torch.tensor(IMAGENET_STD, dtype=rgb.dtype, device=rgb.device).view(3, 1, 1)
        rgb = (rgb - mean) / std
    return rgb, sil


def resized_size(Hs: int, Ws: int, size: int):
    """(H, W) of transforms.Resize(size) on an Hs x Ws image: the shorter side becomes `size`, the longer
    int(size * long / short); no crop."""
    Hs, Ws, size = int(Hs), int(Ws), int(size)
    if Hs <= 0 or Ws <= 0 or size <= 0:
        raise ValueError('sizes must be positive, got %d x %d -> %d' % (Hs, Ws, size))
    if Ws <= Hs:
        return int(size * Hs / Ws), size
    return size, int(size * Ws / Hs)


def prepare_images(rgba_u8: torch.Tensor, *, size=None, jitter=True, rotate=False, normalize=False, factors=None,
                   order=None, angles=None, seed=None, sample_base=0, seed_dev=None):
    """dataset.py:15-19,115-139 for a batch of decoded renderings: rgba_u8 [B,Hs,Ws,4] uint8 on the device (the layout of
    np.asarray(Image.open(p))) -> (rgb [B,3,H,W], silhouette [B,1,H,W], angles [B]) fp32, (H, W) = resized_size(Hs, Ws,
    size) (size default config.IMG_SIZE), every pixel equal to what PIL / torchvision's PIL backend give, bit for bit.
      jitter:    ColorJitter(0.4, 0.4, 0.4) without hue.  factors [B,3] = (brightness, contrast, saturation), each uniform
                 in [0.6, 1.4]; order [B,3] int32 = the permutation of (0, 1, 2) in which they are applied.
      rotate:    the image rotation of AUGMENT_3D['rotate'] (dataset.py:131-139); angles [B] in degrees, uniform in [0, 360).
                 The returned angles are those the images were rotated by (zeros when rotate=False): feed them to
                 rotate_points_forward_x_axis for the points.
      normalize: ImageNet mean / std on rgb (dataset.py:125-126).
    A draw that is not given is drawn in the kernel from Philox4x32-10 keyed on (seed + *seed_dev, sample_base + b), so a
    shard of a batch draws what the whole batch would; seed default: one draw from torch's CPU generator (follows
    torch.manual_seed, like Sampling); seed_dev: a device int64 step counter read by the kernel (HIP-graph replays then
    draw anew).  Three launches, no host synchronisation, no backward."""
    assert rgba_u8.ndimension() == 4 and rgba_u8.size(-1) == 4      # (B, Hs, Ws, 4)
    H, W = resized_size(rgba_u8.size(1), rgba_u8.size(2), config.IMG_SIZE if size is None else size)
    needs_draw = (jitter and (factors is None or order is None)) or (rotate and angles is None)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) if needs_draw else 0
    return ops.prepare_images(rgba_u8, H, W, jitter=jitter, rotate=rotate, normalize=normalize, factors=factors, order=order,
                              angles=angles, seed=seed, seed_dev=seed_dev, sample_base=sample_base)


# ---- the point half of __getitem__ (dataset.py:42-46,161-165; genre.py:66-74; csrc/gtpoints.hip)

CHUNK = _lib.CONSTANTS['VPN_RAGGED_CHUNK']        # faces per chunk: one workgroup of ragged_chunk_kernel
GT_POINT_NUM = 2048                               # dataset.py:165, genre.py:74
INDEX_LIMIT = 0x7fffffff // 3                     # the kernels index 3 * (a vertex or face number) in int32


def chunk_table(face_counts, chunk=None):
    """The chunk table of meshes with the given face counts: ([C,3] rows (mesh, first face in the packed list, face count),
    chunk_offset [S+1]).  Every mesh is tiled in order by chunks of at most `chunk` (default CHUNK) faces; a chunk never
    straddles two meshes."""
    chunk = CHUNK if chunk is None else int(chunk)
    rows, offset, first = [], [0], 0
    for s, count in enumerate(face_counts):
        for start in range(0, count, chunk):
            rows.append((s, first + start, min(chunk, count - start)))
        first += count
        offset.append(len(rows))
    return rows, offset


class MeshBatch:
    """S triangle meshes of different sizes, packed for vpn_ragged_sample: verts [sumP,3] fp32, faces [sumF,3] int32 with
    MESH-LOCAL vertex indices, vert_offset / face_offset / chunk_offset [S+1] int32 and chunks [C,3] int32 = (mesh, first face
    in the packed list, face count <= CHUNK).  Each exists twice: `host` (a dict of CPU tensors, pinned when a device is
    given) and, when a device is given, as attributes on that device.  Offsets and chunks are computed on the host from the
    face counts the loader knows from parsing, so no grid size ever needs a device read-back."""

    FIELDS = ('verts', 'faces', 'vert_offset', 'face_offset', 'chunk_offset', 'chunks')

    def __init__(self, host, device=None):
        self.host = host
        self.device = None if device is None else torch.device(device)
        self.num_meshes = host['vert_offset'].numel() - 1
        self.vert_counts = (host['vert_offset'][1:] - host['vert_offset'][:-1]).tolist()
        self.face_counts = (host['face_offset'][1:] - host['face_offset'][:-1]).tolist()
        for name in self.FIELDS:
            # one non-blocking copy per array out of its pinned staging buffer
            setattr(self, name, None if device is None else host[name].to(self.device, non_blocking=True))

    def __len__(self):
        return self.num_meshes

    @classmethod
    def pack(cls, meshes, device=None):
        """meshes: TriangleMesh objects or (verts [P,3], faces [F,3]) pairs (tensors or anything torch.as_tensor takes).
        device None: the host half only (no GPU needed).  A mesh without vertices or faces is a ValueError that names its
        index; face indices are not checked here (they are clamped on the device)."""
        pairs = []
        for i, m in enumerate(meshes):
            v, f = (m.vertices, m.faces) if hasattr(m, 'vertices') else m
            v = torch.as_tensor(v).detach().to('cpu', torch.float32)
            f = torch.as_tensor(f).detach().to('cpu')
            if v.dim() != 2 or v.size(-1) != 3 or v.size(0) == 0:
                raise ValueError('mesh %d has no vertices (got shape %s, expected [P,3] with P >= 1)' % (i, tuple(v.shape)))
            if f.dim() != 2 or f.size(-1) != 3 or f.size(0) == 0:
                raise ValueError('mesh %d has no faces (got shape %s, expected [F,3] with F >= 1)' % (i, tuple(f.shape)))
            if f.dtype.is_floating_point:
                raise ValueError('mesh %d: faces must be integers' % i)
            pairs.append((v, f))
        if not pairs:
            raise ValueError('MeshBatch.pack needs at least one mesh')
        vert_offset, face_offset = [0], [0]
        for v, f in pairs:
            vert_offset.append(vert_offset[-1] + v.size(0))
            face_offset.append(face_offset[-1] + f.size(0))
        if vert_offset[-1] > INDEX_LIMIT or face_offset[-1] > INDEX_LIMIT:
            raise ValueError('%d vertices / %d faces in one batch: at most %d each' % (vert_offset[-1], face_offset[-1], INDEX_LIMIT))
        rows, chunk_offset = chunk_table([f.size(0) for _, f in pairs])
        pin = device is not None and torch.device(device).type == 'cuda'
        host = {'verts': torch.empty((vert_offset[-1], 3), dtype=torch.float32, pin_memory=pin),
                'faces': torch.empty((face_offset[-1], 3), dtype=torch.int32, pin_memory=pin)}
        for s, (v, f) in enumerate(pairs):
            host['verts'][vert_offset[s]:vert_offset[s + 1]] = v
            # out-of-range indices stay out of range in int32 (and are clamped by the kernels), whatever they were in int64
            host['faces'][face_offset[s]:face_offset[s + 1]] = f.clamp(-1, 0x7fffffff).to(torch.int32)
        for name, values in (('vert_offset', vert_offset), ('face_offset', face_offset), ('chunk_offset', chunk_offset),
                             ('chunks', rows)):
            t = torch.tensor(values, dtype=torch.int32)
            host[name] = t.pin_memory() if pin else t
        return cls(host, device)

    @classmethod
    def from_objs(cls, paths, device=None):
        """TriangleMesh.from_obj for every path (dataset.py:163) through load_obj, packed."""
        from .meshing import load_obj
        return cls.pack([load_obj(p) for p in paths], device)


_PI32 = 3.1415927410125732              # the fp32 pi of rotate.py:4 (VPN_PI)


def _rotation(axis, turns):
    """rotate.py:28-46,59-72 on [S] tensors: axis [S,3] (not normalised), angle in turns -> [S,3,3], in float64."""
    h = ((torch.remainder(turns, 1) * 2) * _PI32) / 2
    r = torch.cat([axis * torch.sin(h)[:, None], torch.cos(h)[:, None]], 1)
    r = r / torch.sqrt((r * r).sum(1))[:, None]
    x, y, z, w = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    return torch.stack([torch.stack([x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw)], 1),
                        torch.stack([2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw)], 1),
                        torch.stack([2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2], 1)], 1)


def view_center_xforms(dists, elevs, azims, dist_invariant=False):
    """The map of transform_to_view_center (dataset.py:168-184) per mesh as [S,3,4] fp32 rows (R | 0): rotate by elev / 360
    turns about -z, by azim / 360 turns about the rotated y axis, divide by dist; dist_invariant (IS_DIST_INVARIANT,
    dataset.py:45-46, multiplies the points by dist again): the rotation alone.  Torch ops on [S] tensors, on the device of
    `dists` when it is a tensor (host numbers stay on the host); built in float64 and rounded once."""
    dev = dists.device if isinstance(dists, torch.Tensor) else torch.device('cpu')
    dists, elevs, azims = (torch.as_tensor(x, dtype=torch.float64, device=dev).detach().reshape(-1) for x in (dists, elevs, azims))
    S = dists.numel()
    if elevs.numel() != S or azims.numel() != S:
        raise ValueError('dists, elevs and azims must have one entry per mesh')
    axes = ops.const_tensor(((0.0, 0.0, -1.0), (0.0, 1.0, 0.0)), torch.float64, dev)
    r1 = _rotation(axes[0:1].expand(S, 3), elevs / 360)
    r2 = _rotation(r1[:, :, 1], azims / 360)                        # the rotated y axis: R1 (0, 1, 0)^T
    m = torch.bmm(r2, r1)
    if not dist_invariant:
        m = m / dists[:, None, None]
    return torch.cat([m, torch.zeros_like(m[:, :, :1])], 2).float()


def genre_xforms(batch):
    """The normalisation of GenReDataset._load_points (genre.py:69-73) per mesh of a MeshBatch as [S,3,4] fp32: subtract the
    vertex mean, divide by 128, swap y and z, negate x, divide by 1.7.  The per-mesh mean is a segment reduction of the packed
    vertices (differences of a float64 running sum at the mesh boundaries: deterministic, no read-back)."""
    on_device = batch.verts is not None
    verts = batch.verts if on_device else batch.host['verts']
    offset = (batch.vert_offset if on_device else batch.host['vert_offset']).long()
    run = torch.cat([torch.zeros((1, 3), dtype=torch.float64, device=verts.device), torch.cumsum(verts.double(), 0)])
    mean = (run[offset[1:]] - run[offset[:-1]]) / (offset[1:] - offset[:-1]).double()[:, None]
    k = 1.0 / (128.0 * 1.7)
    m = torch.zeros((len(batch), 3, 4), dtype=torch.float64, device=verts.device)
    m[:, 0, 0], m[:, 0, 3] = -k, k * mean[:, 0]            # x' = -(x - mean_x) / 128 / 1.7
    m[:, 1, 2], m[:, 1, 3] = k, -k * mean[:, 2]            # y' = (z - mean_z) / 128 / 1.7
    m[:, 2, 1], m[:, 2, 3] = k, -k * mean[:, 1]            # z' = (y - mean_y) / 128 / 1.7
    return m.float()


def _gt_seed(seed, u):
    if seed is None:
        return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()) if u is None else 0
    return int(seed)


def sample_gt_points(batch, n=GT_POINT_NUM, *, sets=1, xforms=None, seed=None, mesh_base=0, u=None, return_faces=False,
                     seed_dev=None, xform_mask=None):
    """mesh.sample(n) (dataset.py:165) for every mesh of a MeshBatch, `sets` times over ONE cumulative-area table per mesh:
    points [S,sets,n,3]; return_faces adds face [S,sets,n] int32 (mesh-local) and bary [S,sets,n,3].
      xforms [S,sets,3,4]: an affine map applied to each sampled point of (mesh, set) (xform_mask: bit t = apply it in set t;
                default all sets): sampling the mapped mesh instead chooses the same faces whenever the map scales all areas
                alike (rotations, reflections, uniform scales, translations).
      u [S,sets,n,3]: explicit uniforms; otherwise Philox4x32-10 keyed on (seed + *seed_dev, mesh_base + s, set): set 0 of
                mesh s draws what vpn_mesh_sample_fwd draws for mesh index mesh_base + s, and a shard of a batch draws what
                the whole batch would.  seed default: one draw from torch's CPU generator (follows torch.manual_seed, like
                prepare_images and Sampling); seed_dev: a device int64 step counter read by the kernel (HIP-graph replays then
                draw anew).
    Three launches whatever S is, no host synchronisation, no autograd node (ground truth is data)."""
    if not isinstance(batch, MeshBatch):
        raise TypeError('batch must be a MeshBatch (MeshBatch.pack / MeshBatch.from_objs)')
    if batch.verts is None:
        raise RuntimeError('vpn_amd operators run on the GPU only: pack the MeshBatch with a device; there is no CPU path')
    if xforms is not None and not isinstance(xforms, torch.Tensor):
        xforms = torch.as_tensor(xforms, dtype=torch.float32)
    return ops.ragged_sample(batch.verts, batch.faces, batch.vert_offset, batch.face_offset, batch.chunk_offset, batch.chunks, n,
                             sets=sets, xforms=xforms, xform_mask=xform_mask, u=u, seed=_gt_seed(seed, u), seed_dev=seed_dev,
                             mesh_base=mesh_base, return_faces=return_faces)


def gt_points(batch, dists, elevs, azims, *, n=GT_POINT_NUM, dist_invariant=False, seed=None, mesh_base=0, seed_dev=None):
    """The two point tensors of __getitem__ (dataset.py:42-46) for a batch: (canonical_points [S,n,3], view_center_points
    [S,n,3]) as two sets over one table: set 0 untransformed, set 1 under view_center_xforms(dists, elevs, azims,
    dist_invariant).  The sets use different draws, as the reference's two sample() calls do."""
    S = len(batch)
    view = view_center_xforms(dists, elevs, azims, dist_invariant)
    if view.size(0) != S:
        raise ValueError('dists, elevs and azims must have one entry per mesh (%d), got %d' % (S, view.size(0)))
    xf = torch.stack([torch.zeros_like(view), view], 1)            # set 0 is masked out: its rows are never read
    pts = sample_gt_points(batch, n, sets=2, xforms=xf, xform_mask=2, seed=seed, mesh_base=mesh_base, seed_dev=seed_dev)
    return pts[:, 0], pts[:, 1]


def gt_normals(batch, face, *, sets=1, xforms=None):
    """The unit normals of the ground-truth points of sample_gt_points(batch, ..., return_faces=True): face [S,sets,n] int32
    (mesh-local) -> [S,sets,n,3].  xforms [S,sets,3,4]: the maps the points were sampled under, for EVERY set (a set that
    xform_mask left unmapped takes the identity rows); the normal is taken from the mapped corners, so it is the normal of
    the mapped surface for any affine map.  A face without area gives (0,0,0).  One launch, no host synchronisation."""
    if not isinstance(batch, MeshBatch):
        raise TypeError('batch must be a MeshBatch (MeshBatch.pack / MeshBatch.from_objs)')
    if batch.verts is None:
        raise RuntimeError('vpn_amd operators run on the GPU only: pack the MeshBatch with a device; there is no CPU path')
    if xforms is not None and not isinstance(xforms, torch.Tensor):
        xforms = torch.as_tensor(xforms, dtype=torch.float32)
    return ops.ragged_face_normals(batch.verts, batch.faces, batch.vert_offset, batch.face_offset, face, sets=sets, xforms=xforms)
