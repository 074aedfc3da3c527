"""Capture tests/golden/g8_cutmix.npz from the reference's own modules/augmentation/cutmix.py on the CPU.

    python tools/make_golden_augment.py /path/to/reference

cutmix.py imports only torch and `config`; a stub `config` module with DEVICE = 'cpu' is put in sys.modules so that it
loads.  Only data is written (allow_pickle=False): the inputs, and for each recorded torch.manual_seed the two draws the
reference made (ratio, permutation), the cut it derived, its output images and points, and per sample the eligible
list (count and candidate numbers: 0..N-1 the sample's own points, N..2N-1 its partner's).  The eligible list is checked
against the list the reference itself handed to adjust_point_num, and every row of the reference's output points is
checked to be a member of it, so the fixture is self-consistent before a GPU sees it.

Mix-up is not captured: the reference's auction is a CUDA extension; its expected values come from oracle.emd_auction."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'g8_cutmix.npz')
SIZE_CAP = 402312                        # the largest fixture committed before this one
B, N, H, W = 8, 640, 10, 13              # 2 N = 1280 candidates: two chunks of the kernel's 1024 threads; W odd, H != W
KINDS = ('more', 'fewer', 'equal_other', 'fixed_point')


def load_reference_cutmix(ref_root):
    cfg = types.ModuleType('config')
    cfg.DEVICE = 'cpu'
    sys.modules['config'] = cfg
    spec = importlib.util.spec_from_file_location('ref_cutmix', os.path.join(ref_root, 'modules', 'augmentation', 'cutmix.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs():
    g = torch.Generator().manual_seed(808)
    pts = torch.rand(B, N, 3, generator=g) - 0.5
    for b in (1, 3, 6):                                  # entirely above every cut the reference can draw (|cut| <= 0.1231)
        pts[b, :, 2] = pts[b, :, 2] * 0.2 + 0.35
    rgbs = torch.rand(B, 3, H, W, generator=g)
    sils = (torch.rand(B, 1, H, W, generator=g) > 0.5).float()
    return pts, rgbs, sils


def run_seed(ref, seed, pts, rgbs, sils):
    """One reference run under torch.manual_seed(seed) -> dict of arrays and the set of case kinds it contains."""
    torch.manual_seed(seed)
    ratio = 0.3 + torch.rand(1).item() * (0.7 - 0.3)     # the reference's two draws, repeated to record them
    perm = torch.randperm(B)
    lists = []
    inner = ref.adjust_point_num
    ref.adjust_point_num = lambda p, n: (lists.append(p.clone()), inner(p, n))[1]
    try:
        torch.manual_seed(seed)
        o_rgb, o_sil, o_pts = ref.cut_mix_data(rgbs, sils, pts)
    finally:
        ref.adjust_point_num = inner
    cut_index = int(W * ratio)
    cut = (0.5 - ratio) * 2 * 0.30769
    assert torch.equal(o_rgb[..., :cut_index], rgbs[..., :cut_index]) and torch.equal(o_rgb[..., cut_index:], rgbs[perm][..., cut_index:])
    count = np.zeros(B, np.int32)
    elig = -np.ones((B, 2 * N), np.int16)
    kinds = set()
    for b in range(B):
        p = int(perm[b])
        cand = torch.cat([pts[b], pts[p]])
        mask = torch.cat([pts[b][:, 2] >= cut, pts[p][:, 2] < cut])
        ids = torch.nonzero(mask).flatten()
        assert torch.equal(cand[ids], lists[b]), 'eligible list differs from what the reference gave adjust_point_num'
        c = ids.numel()
        count[b] = c
        elig[b, :c] = ids.numpy()
        # every output row is a member of the eligible list
        member = (o_pts[b][:, None, :] == cand[ids][None, :, :]).all(2).any(1)
        assert bool(member.all())
        if c == N:
            assert torch.equal(o_pts[b], cand[ids])
        kinds.add('fixed_point' if p == b else 'more' if c > N else 'fewer' if c < N else 'equal_other')
    rec = dict(seed=np.int64(seed), ratio=np.float64(ratio), indices=perm.numpy(), img_cut_index=np.int64(cut_index),
               point_cut_ratio=np.float64(cut), rgbs=o_rgb.numpy(), silhouettes=o_sil.numpy(), points=o_pts.numpy(),
               count=count, eligible=elig)
    return rec, kinds, int(count.min())


def main(ref_root):
    ref = load_reference_cutmix(ref_root)
    pts, rgbs, sils = inputs()
    chosen, seen = [], set()
    for seed in range(200):                              # the first seeds without an empty list: three of them, and
        rec, kinds, cmin = run_seed(ref, seed, pts, rgbs, sils)      # whichever later one adds a case kind still missing
        if cmin > 0 and (len(chosen) < 3 or kinds - seen):
            chosen.append(rec)
            seen |= kinds
        if len(chosen) >= 3 and seen == set(KINDS):
            break
    assert seen == set(KINDS), seen
    assert all(int(r['count'].min()) > 0 for r in chosen)         # the reference has no output for an empty list
    data = dict(points=pts.numpy(), rgbs=rgbs.numpy(), silhouettes=sils.numpy(), n_seeds=np.int64(len(chosen)))
    for k, rec in enumerate(chosen):
        data.update({'s%d_%s' % (k, name): v for name, v in rec.items()})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **data)
    size = os.path.getsize(OUT)
    assert size <= SIZE_CAP, size
    print('wrote %s: %d bytes, seeds %s' % (OUT, size, [int(r['seed']) for r in chosen]))
    for r in chosen:
        print(' seed %d ratio %.4f cut_index %d cut %.5f perm %s count %s' % (r['seed'], r['ratio'], r['img_cut_index'],
              r['point_cut_ratio'], r['indices'].tolist(), r['count'].tolist()))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get('VPN_REFERENCE', ''))
