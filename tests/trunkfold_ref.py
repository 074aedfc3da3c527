"""Float64 restatement of the trunk's inference form (csrc/trunkfold.hip, vpn_amd.fold_batch_norm).

    op    y[b,co,oh,ow] = act(sum_{ci,r,s} x[b,ci,oh st+r-p,ow st+s-p] w[co,ci,r,s] + bias[co] + residual[b,co,oh,ow])
          in that order; act(v) = 0 where v < 0, else v (a NaN stays a NaN); bias and residual may be absent
    fold  s = gamma / sqrt(running_var + eps), w' = w s[co], b' = beta - running_mean s

The convolution is tests/trunkstride_ref.py's direct sum; torch's own convolution and batch norm are not called
(tests/test_trunkfold_cpu.py holds this file to them)."""
import torch

import trunkstride_ref

out_size = trunkstride_ref.out_size


def forward(x, w, bias=None, residual=None, stride=1, padding=0, relu=True):
    y = trunkstride_ref.forward(x, w, stride, padding)
    if bias is not None:
        y = y + bias.double().view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual.double()
    if relu:
        y = torch.where(y < 0, torch.zeros_like(y), y)
    return y


def fold(w, gamma, beta, mean, var, eps):
    """(w', b') in float64."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * s.view(-1, 1, 1, 1), beta.double() - mean.double() * s
