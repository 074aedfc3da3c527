"""The point half of ShapeNetDataset.__getitem__ (dataset.py:42-46,161-165) for a batch, on the device: a directory of OBJ
files (or synthetic meshes when none is given) is packed into one ragged MeshBatch and sampled in three launches into the
canonical and the view-centred ground-truth points; --genre instead applies the normalisation of GenReDataset._load_points
(genre.py:66-74).  Prints the tensors' shapes and a checksum.

    python examples/gt_points.py [--objs DIR] [--n 2048] [--seed 1234] [--dist-invariant] [--genre]"""
import argparse
import glob
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vpn_amd  # noqa: E402


def synthetic(count):
    """UV spheres of growing resolution, squashed differently: meshes of different sizes without a dataset."""
    from vpn_amd.modules.meshing import uv_sphere
    g = torch.Generator().manual_seed(0)
    out = []
    for i in range(count):
        v, f = uv_sphere(4 + 3 * i, 8 + 5 * i)
        out.append((v * (0.2 + 0.3 * torch.rand(3, generator=g)), f))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--objs', default=None, help='directory of .obj files (default: eight synthetic meshes)')
    ap.add_argument('--n', type=int, default=2048)
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--dist-invariant', action='store_true')
    ap.add_argument('--genre', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda')
    if args.objs:
        paths = sorted(glob.glob(os.path.join(args.objs, '*.obj')))
        if not paths:
            raise SystemExit('no .obj files in ' + args.objs)
        batch = vpn_amd.MeshBatch.from_objs(paths, dev)
    else:
        batch = vpn_amd.MeshBatch.pack(synthetic(8), dev)
    S = len(batch)
    print('%d meshes, faces %s, %d chunks' % (S, batch.face_counts, batch.chunks.size(0)))
    if args.genre:
        pts = vpn_amd.sample_gt_points(batch, args.n, xforms=vpn_amd.genre_xforms(batch)[:, None], seed=args.seed)[:, 0]
        print('points', tuple(pts.shape), 'checksum %.6f' % float(pts.double().sum()))
        return
    g = torch.Generator().manual_seed(args.seed)
    dists = (vpn_amd.modules.dataset.DIST_SCALE * (0.6 + 0.4 * torch.rand(S, generator=g))).to(dev)     # rendering_metadata.txt ranges
    elevs, azims = (25 + 5 * torch.rand(S, generator=g)).to(dev), (360 * torch.rand(S, generator=g)).to(dev)
    canon, view = vpn_amd.gt_points(batch, dists, elevs, azims, n=args.n, dist_invariant=args.dist_invariant, seed=args.seed)
    print('canonical_points', tuple(canon.shape), 'checksum %.6f' % float(canon.double().sum()))
    print('view_center_points', tuple(view.shape), 'checksum %.6f' % float(view.double().sum()))


if __name__ == '__main__':
    main()
