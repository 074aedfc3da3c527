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

Out of scope (host-side mesh processing through open3d / trimesh / an external binary): the rest of point_mixup_data
-- ball pivoting, convex decomposition, the Phong render -- and acd.py."""
import torch

from .. import ops

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
