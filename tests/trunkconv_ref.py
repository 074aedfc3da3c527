"""Float64 restatement of the three products of the trunk's 3x3 convolution (csrc/trunkconv.hip): kernel 3x3,
stride 1, padding 1, no bias.  A direct nine-tap sum over shifted copies of the image; torch's own convolution is not called
(tests/test_trunkconv_cpu.py holds this file to it).

    forward          y[b,co,h,w]   = sum_{ci,r,s} x[b,ci,h+r-1,w+s-1] w[co,ci,r,s]
    data gradient    dx[b,ci,h,w]  = sum_{co,r,s} dy[b,co,h+1-r,w+1-s] w[co,ci,r,s]
    weight gradient  dw[co,ci,r,s] = sum_{b,h,w}  dy[b,co,h,w] x[b,ci,h+r-1,w+s-1]
"""
import torch


def shifted(t, dh, dw):
    """u[b,c,h,w] = t[b,c,h+dh,w+dw], zero where that lies outside the image (|dh|, |dw| <= 1)."""
    H, W = t.shape[2:]
    u = torch.zeros_like(t)
    h0, h1 = max(0, -dh), min(H, H - dh)
    w0, w1 = max(0, -dw), min(W, W - dw)
    if h0 < h1 and w0 < w1:
        u[:, :, h0:h1, w0:w1] = t[:, :, h0 + dh:h1 + dh, w0 + dw:w1 + dw]
    return u


def forward(x, w):
    x, w = x.double(), w.double()
    y = torch.zeros((x.shape[0], w.shape[0]) + tuple(x.shape[2:]), dtype=torch.float64)
    for r in range(3):
        for s in range(3):
            y += torch.einsum('bchw,oc->bohw', shifted(x, r - 1, s - 1), w[:, :, r, s])
    return y


def backward(dy, x, w):
    """(dx, dw)."""
    dy, x, w = dy.double(), x.double(), w.double()
    dx, dw = torch.zeros_like(x), torch.zeros_like(w)
    for r in range(3):
        for s in range(3):
            dx += torch.einsum('bohw,oc->bchw', shifted(dy, 1 - r, 1 - s), w[:, :, r, s])
            dw[:, :, r, s] = torch.einsum('bohw,bchw->oc', dy, shifted(x, r - 1, s - 1))
    return dx, dw
