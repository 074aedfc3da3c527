"""Float64 restatement of the reference's GCNModel (modules/network/gcn.py) for the tests: plain torch on the CPU, the
graph aggregation by index_add_ over the edge list (no dense N x N matrix), PyG GCNConv's gcn_norm (self loops with
weight 1, degree with the self loop, D^-1/2 (A + I) D^-1/2) and the reference's bounds loop read literally."""
import torch
import torch.nn.functional as F


def bounds(imgs):
    """get_bound_of_images: the reference's loop, in fp32 as it runs."""
    B, _, h, w = imgs.shape
    out = torch.zeros(B, 4)
    out[:, 1], out[:, 3] = w, h
    for b in range(B):
        m = imgs[b].sum(0) > 0.03
        xs, ys = m.any(0), m.any(1)
        for axis, occ, n in ((0, xs, w), (2, ys, h)):
            for i in range(n):
                j = n - i - 1
                if occ[i] and out[b, axis] == 0:
                    out[b, axis] = i
                if occ[j] and out[b, axis + 1] == n:
                    out[b, axis + 1] = j
                if out[b, axis] > 0 and out[b, axis + 1] < n:
                    break
    out[:, :2] = out[:, :2] / w * 2 - 1
    out[:, 2:] = out[:, 2:] / h * 2 - 1
    return out


def positional_encoding(x):
    enc = [x]
    for k in range(6):
        f = float(2 ** k)
        enc += [torch.sin(x * f), torch.cos(x * f)]
    return torch.cat(enc, -1)


def pooling(maps, points, bnd):
    """perceptual_feature_pooling in the dtype of its inputs: grid of gcn.py:141-153, grid_sample(align_corners=True)."""
    zmax, zmin = points[..., 2].max(1, keepdim=True)[0], points[..., 2].min(1, keepdim=True)[0]
    ymax, ymin = points[..., 1].max(1, keepdim=True)[0], points[..., 1].min(1, keepdim=True)[0]
    b = bnd[:, None, :]
    gx = b[..., 0] + (1 - (points[..., 2] - zmin) / (zmax - zmin)) * (b[..., 1] - b[..., 0])
    gy = b[..., 2] + (1 - (points[..., 1] - ymin) / (ymax - ymin)) * (b[..., 3] - b[..., 2])
    grid = torch.stack([gx, gy], -1)[:, None]
    out = [F.grid_sample(m, grid, align_corners=True) for m in maps]
    return torch.cat(out, 1)[:, :, 0].permute(0, 2, 1)


def gcn_norm(edges, n, dtype=torch.float64):
    """edges (E, 2) undirected -> (src, dst, weight) over both directions and the self loops."""
    e = edges.long()
    loops = torch.arange(n)
    src = torch.cat([e[:, 0], e[:, 1], loops])
    dst = torch.cat([e[:, 1], e[:, 0], loops])
    deg = torch.zeros(n, dtype=dtype).index_add_(0, dst, torch.ones(dst.numel(), dtype=dtype))
    dis = deg.pow(-0.5)
    return src, dst, dis[src] * dis[dst]


def aggregate(x, norm, bias=None):
    """sum_j A_hat[i, j] x[:, j] (+ bias) by index_add_ over the entries."""
    src, dst, w = norm
    out = torch.zeros_like(x).index_add_(1, dst, x[:, src] * w.to(x.dtype)[None, :, None])
    return out + bias if bias is not None else out


def unique_edges(faces):
    f = faces.long().reshape(-1, 3)
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = torch.stack([e.min(1)[0], e.max(1)[0]], 1)
    return torch.unique(e[e[:, 0] != e[:, 1]], dim=0)


def model(params, verts, rgbs, maps, glob, faces, use_position_encoding=True, masks=None, pre=None):
    """GCNModel.forward with parameters `params` (a state dict in the PyG 1.x layout: convK.weight (in, out)), in the
    dtype of its inputs (float64 in the tests).  masks: optional ReLU decisions of conv2 / conv4 / conv6 (bool, as
    another implementation took them) used instead of `pre > 0`; pre: optional list that receives the three
    pre-activations."""
    n = verts.shape[1]
    norm = gcn_norm(unique_edges(faces), n)
    x = positional_encoding(verts) if use_position_encoding else verts
    bnd = bounds(rgbs.float()).to(verts.dtype)
    parts = [x, pooling(maps, verts, bnd)]
    if glob is not None:
        parts.append(glob[:, None, :].expand(-1, n, -1))
    x = torch.cat(parts, 2)

    def conv(k, x):
        return aggregate(x @ params['conv%d.weight' % k], norm, params['conv%d.bias' % k])

    for i, (a, b) in enumerate(((1, 2), (3, 4), (5, 6))):
        x = conv(b, conv(a, x))
        if pre is not None:
            pre.append(x.detach())
        x = x * masks[i].to(x.dtype) if masks is not None else x.relu()
    x = x.reshape(x.shape[0], -1)
    for i in range(3):
        x = x @ params['fc.%d.weight' % i].t() + params['fc.%d.bias' % i]
    return verts + torch.tanh(x).view(x.shape[0], -1, 3) * 0.1
