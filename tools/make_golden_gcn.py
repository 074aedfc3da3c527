"""Capture tests/golden/g7_gcn_*.npz from the reference's own modules/network/gcn.py on the CPU.

    python tools/make_golden_gcn.py /path/to/reference

kaolin and torch_geometric are absent: stub `kaolin.rep` / `torch_geometric.nn` modules are put in sys.modules so that
gcn.py imports, and Tensor.cuda is the identity while its functions run.  Only data is written (allow_pickle=False):
the inputs and outputs of get_bound_of_images, positional_encoding and perceptual_feature_pooling, and the reference's
CPU-autograd gradients of sum(W * pooled) w.r.t. the maps and the vertices for a fixed W."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden')


def load_reference_gcn(ref_root):
    kaolin, rep = types.ModuleType('kaolin'), types.ModuleType('kaolin.rep')
    rep.TriangleMesh = type('TriangleMesh', (), {})
    kaolin.rep = rep
    tg, tgnn = types.ModuleType('torch_geometric'), types.ModuleType('torch_geometric.nn')
    for n in ('GCNConv', 'TAGConv', 'GraphUNet', 'BatchNorm'):
        setattr(tgnn, n, type(n, (), {}))
    tg.nn = tgnn
    sys.modules.update({'kaolin': kaolin, 'kaolin.rep': rep, 'torch_geometric': tg, 'torch_geometric.nn': tgnn})
    spec = importlib.util.spec_from_file_location('ref_gcn', os.path.join(ref_root, 'modules', 'network', 'gcn.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.GCNModel


def bound_images(H=32, W=40):
    imgs = torch.zeros(10, 3, H, W)
    imgs[0, :, 5:20, 7:30] = 0.5                       # interior box
    imgs[1, :, 0:12, 0:9] = 0.3                         # column 0 and row 0 occupied (with others)
    imgs[2, :, 3:9, 0] = 0.2                            # only column 0 occupied
    imgs[3, 1, 17, 23] = 1.0                            # a single pixel
    # imgs[4]: empty
    imgs[5] += 1.0                                      # full
    imgs[6, :, 4:10, 5:11] = 0.0099                     # channel sum 0.0297, just below 0.03 ...
    imgs[6, 0, 20, 30] = 0.0302                         # ... and one pixel just above it
    imgs[7, 0, 0, 0] = 0.5                              # only pixel (0, 0)
    imgs[8, :, H - 1, W - 1] = 0.4                      # only the last pixel
    imgs[9] = torch.rand(3, H, W, generator=torch.Generator().manual_seed(7)) * 0.02   # noise summing around 0.03
    return imgs


def main(ref_root):
    Ref = load_reference_gcn(ref_root)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        imgs = bound_images()
        bounds_img = Ref.get_bound_of_images(imgs)

        import vpn_amd.modules.meshing as M
        g = torch.Generator().manual_seed(2024)
        B, K = 3, 2
        sv, sf = M.uv_sphere()
        verts = []
        for b in range(B):
            parts = []
            for k in range(K):
                s = (torch.rand(3, generator=g) * 0.2 + 0.1)
                t = (torch.rand(3, generator=g) - 0.5) * 0.6
                parts.append(sv * s + t)
            verts.append(torch.cat(parts))
        verts = torch.stack(verts)                                       # (B, 256, 3)
        faces = torch.cat([sf + 128 * k for k in range(K)])
        enc = Ref.positional_encoding(verts)

        shapes = [(4, 32), (8, 16), (16, 8), (32, 4)]
        maps = [torch.randn(B, c, s, s, generator=g) for c, s in shapes]
        rgbs = torch.zeros(B, 3, 64, 64)
        rgbs[0, :, 10:50, 5:60] = 0.5
        rgbs[1, :, 0:30, 20:40] = 0.5
        bounds = Ref.get_bound_of_images(rgbs)
        mp = [m.clone().requires_grad_(True) for m in maps]
        vp = verts.clone().requires_grad_(True)
        pooled = Ref.perceptual_feature_pooling(mp, vp, bounds)
        Wt = torch.randn(pooled.shape, generator=g)
        (pooled * Wt).sum().backward()
    finally:
        torch.Tensor.cuda = cuda
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, 'g7_gcn_bounds.npz'), imgs=imgs.numpy(), bounds=bounds_img.numpy())
    np.savez_compressed(os.path.join(OUT, 'g7_gcn_encoding.npz'), verts=verts.numpy(), faces=faces.numpy(), encoding=enc.numpy())
    np.savez_compressed(os.path.join(OUT, 'g7_gcn_pooling.npz'), verts=verts.numpy(), rgbs=rgbs.numpy(), bounds=bounds.numpy(),
             **{'map%d' % i: m.numpy() for i, m in enumerate(maps)}, pooled=pooled.detach().numpy(), W=Wt.numpy(),
             **{'grad_map%d' % i: m.grad.numpy() for i, m in enumerate(mp)}, grad_verts=vp.grad.numpy())
    print('wrote g7_gcn_{bounds,encoding,pooling}.npz', bounds_img.tolist())


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get('VPN_REFERENCE', ''))
