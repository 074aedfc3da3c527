"""The on-disk formats either side of the hot path (row f4; modules/dataset/dataset.py of the reference): which
models belong to which split, the camera of every rendering, and how an RGBA rendering becomes the network input
and the GT silhouette.  The text parsers and split_rgba are host-side; prepare_images is the loader's image transform
(Resize, ColorJitter, ToTensor, the rotation of AUGMENT_3D['rotate'], the split, Normalize) for a whole batch on the
device, bit-exact to PIL (csrc/input.hip).  The dataset class itself (file discovery, PNG decoding, kaolin
mesh sampling) is out of scope; the device-side augmentations are in modules/augmentation.py."""
import torch

from .. import config, ops

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
