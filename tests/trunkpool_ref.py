"""Restatement of the stem's pool op (the tp_ kernels of csrc/trunknorm.hip) in plain torch, in the dtype
of its inputs (the tests call it in float64): batch norm over (B, H, W) per channel, ReLU, then MaxPool2d(3, 2, 1), forward
and backward by the formulas of include/vpn_hip.h.  No autograd: the backward is written out and routes by the forward's
own tap indices, so that tests/test_trunkpool_cpu.py can hold it against torch's own."""
import torch

import trunknorm_ref as N


def out_size(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def taps(y):
    """[B,C,H,W] -> [B,C,PH,PW,9]: the nine taps r * 3 + s of every window (rows 2 ph - 1 + r, columns 2 pw - 1 + s), -inf
    where a tap lies outside the map."""
    B, C, H, W = y.shape
    PH, PW = out_size(H, W)
    pad = torch.full((B, C, 2 * PH + 1, 2 * PW + 1), float('-inf'), dtype=y.dtype)
    pad[:, :, 1:H + 1, 1:W + 1] = y
    return torch.stack([pad[:, :, r:r + 2 * PH:2, s:s + 2 * PW:2] for r in range(3) for s in range(3)], dim=-1)


def first_max(t):
    """(max, index of the FIRST maximum) along the last dimension: ATen's pool keeps a tap unless a later one is greater."""
    best = t.max(dim=-1).values
    first = (t == best.unsqueeze(-1)).to(torch.uint8).argmax(dim=-1)       # argmax of 0/1: the first 1
    return best, first.to(torch.uint8)


def forward(x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps):
    """-> (p, idx uint8, pre, save_mean, save_invstd, running_mean', running_var', num_batches_tracked'): `pre` is the
    full-size value the ReLU sees."""
    y, pre, mean, invstd, rm, rv, nbt = N.forward(x, weight, bias, running_mean, running_var, num_batches_tracked, None,
                                                  training, momentum, eps, True)
    p, idx = first_max(taps(y))
    return p, idx, pre, mean, invstd, rm, rv, nbt


def flat_from_taps(idx, H, W):
    """uint8 tap numbers -> ATen's flat indices h * W + w (int64)."""
    PH, PW = idx.shape[-2:]
    k = idx.long()
    h = 2 * torch.arange(PH).view(PH, 1) - 1 + k // 3
    w = 2 * torch.arange(PW).view(1, PW) - 1 + k % 3
    return h * W + w


def taps_from_flat(flat, H, W):
    """ATen's flat indices h * W + w -> uint8 tap numbers r * 3 + s."""
    PH, PW = flat.shape[-2:]
    r = flat // W - (2 * torch.arange(PH).view(PH, 1) - 1)
    s = flat % W - (2 * torch.arange(PW).view(1, PW) - 1)
    assert bool(((r >= 0) & (r < 3) & (s >= 0) & (s < 3)).all())
    return (r * 3 + s).to(torch.uint8)


def upstream(dp, p, idx, H, W):
    """g [B,C,H,W]: dp [p > 0] of every window added to the pixel its idx names."""
    B, C = dp.shape[:2]
    g = torch.zeros((B, C, H * W), dtype=dp.dtype)
    g.scatter_add_(2, flat_from_taps(idx, H, W).reshape(B, C, -1), (dp * (p > 0).to(dp.dtype)).reshape(B, C, -1))
    return g.view(B, C, H, W)


def backward(dp, x, p, idx, weight, mean, invstd, training):
    """-> (dx, d_weight, d_bias) from the forward's p and idx and (save_mean, save_invstd), or the running mean and
    1 / sqrt(running_var + eps) in eval."""
    g = upstream(dp, p, idx, x.shape[2], x.shape[3])
    dx, dw, db, _ = N.backward(g, x, None, weight, mean, invstd, training, False, False)
    return dx, dw, db
