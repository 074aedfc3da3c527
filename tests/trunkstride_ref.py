"""Float64 restatement of the three products of the trunk's strided convolutions (csrc/trunkstride.hip):
square kernel R x R, stride st, padding p, dilation 1, groups 1, no bias.  A direct sum over the R R taps, each a strided
slice of the zero-padded image; torch's own convolution is not called (tests/test_trunkstride_cpu.py holds this file to it).

    OH = (H + 2 p - R) // st + 1, OW likewise
    forward          y[b,co,oh,ow]  = sum_{ci,r,s} x[b,ci,oh st+r-p,ow st+s-p] w[co,ci,r,s]
    data gradient    dx[b,ci,ih,iw] = sum_{co,r,s} dy[b,co,(ih+p-r)/st,(iw+p-s)/st] w[co,ci,r,s]   (exact quotients in range only)
    weight gradient  dw[co,ci,r,s]  = sum_{b,oh,ow} dy[b,co,oh,ow] x[b,ci,oh st+r-p,ow st+s-p]
"""
import torch


def out_size(H, W, R, stride, padding):
    return (H + 2 * padding - R) // stride + 1, (W + 2 * padding - R) // stride + 1


def _padded(x, p):
    B, C, H, W = x.shape
    xp = torch.zeros((B, C, H + 2 * p, W + 2 * p), dtype=x.dtype)
    xp[:, :, p:p + H, p:p + W] = x
    return xp


def _tap(t, r, s, OH, OW, st):
    """t[:, :, oh st + r, ow st + s] for oh < OH, ow < OW: a view."""
    return t[:, :, r:r + (OH - 1) * st + 1:st, s:s + (OW - 1) * st + 1:st]


def forward(x, w, stride, padding):
    x, w = x.double(), w.double()
    R = w.shape[2]
    OH, OW = out_size(x.shape[2], x.shape[3], R, stride, padding)
    xp = _padded(x, padding)
    y = torch.zeros((x.shape[0], w.shape[0], OH, OW), dtype=torch.float64)
    for r in range(R):
        for s in range(R):
            y += torch.einsum('bchw,oc->bohw', _tap(xp, r, s, OH, OW, stride), w[:, :, r, s])
    return y


def backward(dy, x, w, stride, padding):
    """(dx, dw)."""
    dy, x, w = dy.double(), x.double(), w.double()
    R, p = w.shape[2], padding
    H, W = x.shape[2:]
    OH, OW = out_size(H, W, R, stride, padding)
    assert tuple(dy.shape[2:]) == (OH, OW)
    xp = _padded(x, p)
    dxp, dw = torch.zeros_like(xp), torch.zeros_like(w)
    for r in range(R):
        for s in range(R):
            _tap(dxp, r, s, OH, OW, stride).add_(torch.einsum('bohw,oc->bchw', dy, w[:, :, r, s]))
            dw[:, :, r, s] = torch.einsum('bohw,bchw->oc', dy, _tap(xp, r, s, OH, OW, stride))
    return dxp[:, :, p:p + H, p:p + W].clone(), dw
