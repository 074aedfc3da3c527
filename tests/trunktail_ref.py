"""Restatement of the trunk's tail (the tt_ kernels of csrc/trunknorm.hip) in plain torch, in the dtype of
its inputs (the tests call it in float64), on top of tests/trunknorm_ref.py: the last norm / add / ReLU site also gives
m = y.mean((2, 3)), the global average pool, and its backward takes m's gradient: the upstream gradient of an element is
dy[b,c,hw] + dm[b,c] / HW.  No autograd: the backward is written out."""
import torch

import trunknorm_ref as N


def forward(x, weight, bias, running_mean, running_var, num_batches_tracked, residual, training, momentum, eps, relu):
    """-> (y, m, pre, save_mean, save_invstd, running_mean', running_var', num_batches_tracked'): trunknorm_ref.forward with
    m [B,C] after y."""
    y, *rest = N.forward(x, weight, bias, running_mean, running_var, num_batches_tracked, residual, training, momentum, eps, relu)
    return (y, y.mean((2, 3)), *rest)


def upstream(dy, dm, shape):
    """dy + dm[:, :, None, None] / HW for the map of `shape`; dy or dm may be None (no gradient from that side)."""
    HW = shape[2] * shape[3]
    if dm is None:
        return dy
    g = (dm[:, :, None, None] / HW).expand(shape).contiguous()
    return g if dy is None else dy + g


def backward(dy, dm, x, y, weight, mean, invstd, training, relu, has_residual):
    """-> (dx, d_weight, d_bias, d_residual | None): trunknorm_ref.backward on the upstream gradient above."""
    return N.backward(upstream(dy, dm, x.shape), x, y, weight, mean, invstd, training, relu, has_residual)
