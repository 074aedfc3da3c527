"""Restatement of csrc/trunknorm.hip in plain torch, in the dtype of its inputs (the tests call it in
float64): batch norm over (B, H, W) per channel, then `+ residual`, then ReLU; forward and backward by the formulas of
include/vpn_hip.h, training and eval, the running-statistics update and the batch counter included.  No autograd: the
backward is written out, so that tests/test_trunknorm_cpu.py can hold it against torch's own."""
import torch


def _c(t):
    return t.view(1, -1, 1, 1)


def forward(x, weight, bias, running_mean, running_var, num_batches_tracked, residual, training, momentum, eps, relu):
    """-> (y, pre, save_mean, save_invstd, running_mean', running_var', num_batches_tracked'): `pre` is the value the
    ReLU sees; the inputs are left as they are.  Eval: save_* are the running mean and 1 / sqrt(running_var + eps)."""
    C = x.shape[1]
    N = x.numel() // C
    if training:
        mean = x.mean(dim=(0, 2, 3))
        var = ((x - _c(mean)) ** 2).mean(dim=(0, 2, 3))
        new_mean = (1 - momentum) * running_mean + momentum * mean
        new_var = (1 - momentum) * running_var + momentum * (var * (N / (N - 1)))
        counter = num_batches_tracked + 1
    else:
        mean, var = running_mean, running_var
        new_mean, new_var, counter = running_mean.clone(), running_var.clone(), num_batches_tracked.clone()
    invstd = 1.0 / torch.sqrt(var + eps)
    pre = (x - _c(mean)) * _c(invstd)
    if weight is not None:
        pre = pre * _c(weight)
    if bias is not None:
        pre = pre + _c(bias)
    if residual is not None:
        pre = pre + residual
    y = pre.clamp_min(0) if relu else pre
    return y, pre, mean, invstd, new_mean, new_var, counter


def backward(dy, x, y, weight, mean, invstd, training, relu, has_residual):
    """-> (dx, d_weight, d_bias, d_residual | None) from the forward's output y and (save_mean, save_invstd), or the
    running mean and 1 / sqrt(running_var + eps) in eval."""
    C = x.shape[1]
    N = x.numel() // C
    g = dy * (y > 0).to(dy.dtype) if relu else dy
    xhat = (x - _c(mean)) * _c(invstd)
    db = g.sum(dim=(0, 2, 3))
    dw = (g * xhat).sum(dim=(0, 2, 3))
    k = invstd if weight is None else weight * invstd
    if training:
        dx = _c(k) * (g - _c(db) / N - xhat * _c(dw) / N)
    else:
        dx = g * _c(k)
    return dx, dw, db, (g if has_residual else None)
