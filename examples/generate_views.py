"""The view loop of the reference's generate.py:150-173 for one mesh: 20 random cameras, ONE PhongRenderer.views call (one
Phong launch and one silhouette launch for all of them), then per view the three files ACDMixDataset reads:

    img_%.6d.png    RGBA: the Phong render, alpha = the soft silhouette SilhouetteLoss renders during training
    mesh_%.6d.obj   the mesh in the view-centred frame (obj_to_view_points)
    meta_%.6d.json  {"dist", "elev", "azim"}

    python examples/generate_views.py OUT_DIR [--views 20] [--size 128] [--seed 0] [--obj A.obj B.obj ...]

Without --obj the mesh is two Meshing spheres merged by merge_meshes (one colour per part): no dataset is needed.  Every
--obj file is taken as one part of the atlas.

    python examples/generate_views.py OUT_DIR --dataset acd_mix [--batch 8] [--batches 1] [--views 20] [--size 128] [--obj A.obj B.obj ...]

writes the same triples for ACD mixes, the whole of generate.py:108-173 on the device (acd_mix_data): two
objects are decomposed into convex hulls, augmented, merged and decomposed again, then rendered from --views cameras each.
The objects are the vertices of the --obj files, paired at random as generate.py:120 does (at least two files); without
--obj they are surface samples of random ellipsoid pairs.

    python examples/generate_views.py OUT_DIR --dataset point_mixup [--batch 8] [--batches 1] [--size 128]

writes the files of generate.py:42-66 instead: per mixed sample `rgb_%d.png`, `silhouette_%d.png` and `mesh_%d.obj`, numbered
from 1, made by generate_point_mixup_data.  Without a dataset the clouds are surface samples of random
ellipsoid pairs.

--prepare (any dataset) also pushes what was rendered, still on the device, through prepare_images -- the transform the
reference's loader applies to every image it opens (Resize to --size, ColorJitter) -- and writes the network
input beside each image as `input_%.6d.png` (rgb and silhouette put back together as RGBA)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vpn_amd import Meshing, PhongRenderer, TriangleMesh, merge_meshes, obj_to_view_points  # noqa: E402


def default_mesh(device='cuda'):
    """Two ellipsoids made by Meshing.sphere_meshing, merged into one mesh with a two-texel atlas (colours: torch.rand)."""
    v = torch.tensor([[0.30, 0.22, 0.26], [0.18, 0.30, 0.20]], device=device)
    q = torch.tensor([[0.3, 0.5, 0.2, 0.4], [0.1, 0.9, 0.3, 1.1]], device=device)
    t = torch.tensor([[0.0, 0.05, 0.25], [0.05, -0.05, -0.30]], device=device)
    parts = [TriangleMesh(m.vertices.detach().clone(), m.faces) for m in Meshing.sphere_meshing(v, q, t)]
    return merge_meshes(parts)


def random_cameras(n):
    """generate.py:153-155, drawn in its order: dist 3 .. 5, elev -45 .. 45, azim 0 .. 360."""
    cams = []
    for _ in range(n):
        dist = 3.0 + torch.rand(1).item() * 2
        elev = (torch.rand(1).item() - 0.5) * 90
        azim = torch.rand(1).item() * 360
        cams.append((dist, elev, azim))
    return cams


def write_prepared(rgba_u8, out_dir, first, img_size):
    """rgba_u8 [N,H,W,4] uint8 on the device -> input_%.6d.png: what prepare_images makes of each rendering."""
    from PIL import Image
    from vpn_amd import prepare_images
    rgb, sil, _ = prepare_images(rgba_u8.contiguous(), size=img_size)
    out = (torch.cat([rgb, sil], 1) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    for i in range(out.shape[0]):
        Image.fromarray(out[i], 'RGBA').save(os.path.join(out_dir, 'input_%.6d.png' % (first + i)))


@torch.no_grad()
def generate(mesh, uv, texture, out_dir, n_views=20, img_size=128, first=0, prepare=False):
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    cams = random_cameras(n_views)
    rgb, alpha = PhongRenderer.views(mesh, cams, uv, texture, img_size=img_size)        # [V,S,S,3], [V,S,S,1]
    dev = mesh.vertices.device
    cam_t = torch.tensor(cams, dtype=torch.float32).to(dev)
    centred = obj_to_view_points(mesh.vertices.detach()[None].expand(n_views, -1, -1).contiguous(), cam_t[:, 0].contiguous(),
                                 cam_t[:, 1].contiguous(), cam_t[:, 2].contiguous())
    rgba = (torch.cat([rgb, alpha], -1).clamp(0.0, 1.0) * 255.0).to(torch.uint8)                    # ToPILImage's quantisation
    if prepare:
        write_prepared(rgba, out_dir, first, img_size)
    rgba = rgba.cpu().numpy()
    centred = centred.cpu()
    faces = mesh.faces.cpu()
    for j, (dist, elev, azim) in enumerate(cams):
        n = first + j
        Image.fromarray(rgba[j], 'RGBA').save(os.path.join(out_dir, 'img_%.6d.png' % n))
        TriangleMesh(centred[j], faces).save_mesh(os.path.join(out_dir, 'mesh_%.6d.obj' % n))
        with open(os.path.join(out_dir, 'meta_%.6d.json' % n), 'w') as f:
            f.write(json.dumps({'dist': dist, 'elev': elev, 'azim': azim}))
    return n_views


def default_clouds(B, n=2048, device='cuda'):
    """Stand-ins for data['view_center_points']: n surface points of two random ellipsoids per sample."""
    from vpn_amd import SPHERE, Sampling
    v = (torch.rand(B, 2, 3) + 0.3) / 5.0
    params = torch.cat([v, torch.rand(B, 2, 4), 0.25 * (torch.rand(B, 2, 3) * 2 - 1)], 2).to(device)
    return Sampling.sample_primitives(params, [SPHERE, SPHERE], n // 2, seed=int(torch.randint(0, 2 ** 31, (1,)).item()))


@torch.no_grad()
def generate_point_mixup(clouds, out_dir, img_size=128, first=1, prepare=False):
    """generate.py:54-66 for one batch of view-centred clouds [B,N,3]: -> the number of triples written."""
    from PIL import Image
    from vpn_amd import generate_point_mixup_data
    os.makedirs(out_dir, exist_ok=True)
    rgbs, silhouettes, meshes = generate_point_mixup_data(clouds, img_size=img_size)
    rgb8 = (rgbs.clamp(0.0, 1.0) * 255.0).to(torch.uint8).permute(0, 2, 3, 1)                       # ToPILImage's quantisation
    sil8 = (silhouettes.clamp(0.0, 1.0) * 255.0).to(torch.uint8)[:, 0]
    if prepare:
        write_prepared(torch.cat([rgb8, sil8[..., None]], -1), out_dir, first, img_size)
    rgb8, sil8 = rgb8.cpu().numpy(), sil8.cpu().numpy()
    for i, mesh in enumerate(meshes):
        n = first + i
        Image.fromarray(rgb8[i], 'RGB').save(os.path.join(out_dir, 'rgb_%d.png' % n))
        Image.fromarray(sil8[i], 'L').save(os.path.join(out_dir, 'silhouette_%d.png' % n))
        TriangleMesh(mesh.vertices.cpu(), mesh.faces.cpu()).save_mesh(os.path.join(out_dir, 'mesh_%d.obj' % n))
    return len(meshes)


@torch.no_grad()
def generate_acd_mix(clouds1, clouds2, out_dir, n_views=20, img_size=128, first=0, prepare=False):
    """generate.py:125-173 for S pairs of objects given as clouds [S,N,3]: -> the number of triples written, S * n_views."""
    from PIL import Image
    from vpn_amd import acd_mix_data
    os.makedirs(out_dir, exist_ok=True)
    rgba, centred, _gt, dists, elevs, azims, parts = acd_mix_data(clouds1, clouds2, views=n_views, img_size=img_size, return_parts=True)
    rgba8 = (rgba.clamp(0.0, 1.0) * 255.0).to(torch.uint8).permute(0, 1, 3, 4, 2)                   # ToPILImage's quantisation
    if prepare:
        write_prepared(rgba8.reshape((-1,) + tuple(rgba8.shape[2:])), out_dir, first, img_size)
    rgba8 = rgba8.cpu().numpy()
    centred, faces = centred.cpu(), parts['faces'].cpu()
    dists, elevs, azims = dists.cpu(), elevs.cpu(), azims.cpu()
    n = first
    for s in range(rgba8.shape[0]):
        for v in range(n_views):
            Image.fromarray(rgba8[s, v], 'RGBA').save(os.path.join(out_dir, 'img_%.6d.png' % n))
            TriangleMesh(centred[s, v], faces).save_mesh(os.path.join(out_dir, 'mesh_%.6d.obj' % n))
            with open(os.path.join(out_dir, 'meta_%.6d.json' % n), 'w') as f:
                f.write(json.dumps({'dist': float(dists[s, v]), 'elev': float(elevs[s, v]), 'azim': float(azims[s, v])}))
            n += 1
    return n - first


def obj_cloud_pairs(paths, B, n=2048, device='cuda'):
    """B random pairs of the OBJ files' vertex clouds (generate.py:120-126), each resampled to n vertices with replacement."""
    import random
    clouds = [TriangleMesh.from_obj(p).vertices.float() for p in paths]
    pick = lambda v: v[torch.randint(0, v.size(0), (n,))]
    pairs = [random.sample(clouds, 2) for _ in range(B)]
    return torch.stack([pick(a) for a, _ in pairs]).to(device), torch.stack([pick(b) for _, b in pairs]).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out_dir')
    ap.add_argument('-d', '--dataset', default='views', choices=['views', 'point_mixup', 'acd_mix'], help='what to write (generate.py -d)')
    ap.add_argument('--batch', type=int, default=8, help='point_mixup / acd_mix: samples per batch (config.py:9)')
    ap.add_argument('--batches', type=int, default=1, help='point_mixup / acd_mix: batches to write')
    ap.add_argument('--views', type=int, default=20)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--obj', nargs='*', default=[], help='OBJ files, one per part of the atlas')
    ap.add_argument('--prepare', action='store_true', help='also write input_%%.6d.png: each rendering after prepare_images')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the renderer runs on the GPU only'
    torch.manual_seed(args.seed)
    if args.dataset == 'point_mixup':
        n = 0
        for _ in range(args.batches):
            n += generate_point_mixup(default_clouds(args.batch), args.out_dir, args.size, first=n + 1, prepare=args.prepare)
        print('wrote %d rgb / silhouette / mesh triples to %s' % (n, args.out_dir))
        return
    if args.dataset == 'acd_mix':
        import random
        random.seed(args.seed)
        n = 0
        for _ in range(args.batches):
            if args.obj:
                assert len(args.obj) >= 2, 'a mix needs two objects'
                c1, c2 = obj_cloud_pairs(args.obj, args.batch)
            else:
                c1, c2 = default_clouds(args.batch), default_clouds(args.batch)
            n += generate_acd_mix(c1, c2, args.out_dir, args.views, args.size, first=n, prepare=args.prepare)
        print('wrote %d img / mesh / meta triples to %s' % (n, args.out_dir))
        return
    if args.obj:
        mesh, uv, texture = merge_meshes([TriangleMesh.from_obj(p).cuda() for p in args.obj])
    else:
        mesh, uv, texture = default_mesh()
    n = generate(mesh, uv, texture, args.out_dir, args.views, args.size, prepare=args.prepare)
    print('wrote %d img / mesh / meta triples to %s' % (n, args.out_dir))


if __name__ == '__main__':
    main()
