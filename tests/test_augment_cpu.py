"""CPU checks of the batch augmentation stage (modules/augmentation.py, csrc/augment.hip): the new entry points validate
their arguments and refuse an N beyond the LDS bound without a GPU, the module mirrors the reference's names and
positional parameters, the g8 fixture holds the four case kinds and is self-consistent, and no new kernel uses scratch."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from test_kernel_budget_cpu import _resources

SIZE_CAP = 402312            # the largest fixture committed before g8_cutmix.npz


def test_entry_points_validate_without_a_gpu():
    import vpn_amd._lib as lib
    L = lib.lib()
    f = ctypes.c_void_p(64)              # never dereferenced: every call below is refused before a launch
    assert L.vpn_cutmix_points(None, None, None, 0.0, 1, 0, 2, 16, 16, None, None, None, None) == -1
    assert L.vpn_cutmix_points(f, f, None, 0.0, 1, 0, 0, 16, 16, f, f, f, None) == -1
    assert L.vpn_cutmix_images(None, None, None, 2, 3, 1, 8, 8, 4, None, None, None) == -1
    assert L.vpn_cutmix_images(f, f, f, 2, 3, 1, 8, 8, 9, f, f, None) == -1          # cut_index > W
    assert L.vpn_cutmix_images(f, None, f, 2, 3, 1, 8, 8, 4, f, None, None) == -1    # Cb > 0 without its pointers
    assert L.vpn_mixup_gather(None, None, 2, 16, None, None) == -1
    assert L.vpn_mixup_lerp(None, None, None, 2, 16, 0.5, 0.5, None, None) == -1
    # the LDS bound: refused with VPN_E_TOOBIG before anything is launched
    big = lib.lib().vpn_cutmix_points
    assert big(f, f, None, 0.0, 1, 0, 2, 8193, 8193, f, f, f, None) == -2
    assert big(f, f, None, 0.0, 1, 0, 2, 1 << 20, 1 << 20, f, f, f, None) == -2
    assert L.vpn_cutmix_points_lds(8193) == 0
    # 64-bit keys of the 2 N candidates padded to a power of two, one offset per (chunk of 1024, wave), the total
    assert L.vpn_cutmix_points_lds(2048) == 4096 * 8 + (4 * 16 + 1) * 4
    assert L.vpn_cutmix_points_lds(4096) == 8192 * 8 + (8 * 16 + 1) * 4
    assert L.vpn_cutmix_points_lds(8192) <= 160 * 1024
    assert b'documented limit' in L.vpn_error_string(-2)


def test_module_mirrors_the_reference_names_and_parameters():
    import vpn_amd
    from vpn_amd.modules import augmentation as A
    sig = inspect.signature
    assert list(sig(A.cut_mix_data).parameters)[:3] == ['rgbs', 'silhouettes', 'view_center_points']
    assert list(sig(A.cut_mix_batch_points).parameters)[:3] == ['view_center_points', 'indices', 'cut_ratio']
    assert list(sig(A.adjust_point_num).parameters)[:2] == ['points', 'N']
    assert list(sig(A.mixup_points).parameters)[:1] == ['points']
    kw = inspect.Parameter.KEYWORD_ONLY
    for fn, names in ((A.cut_mix_data, ('cut_ratio', 'indices', 'seed', 'sample_base')),
                      (A.mixup_points, ('ratio', 'indices', 'eps', 'iters'))):
        for n in names:
            assert sig(fn).parameters[n].kind == kw
    assert sig(A.mixup_points).parameters['eps'].default == 0.005 and sig(A.mixup_points).parameters['iters'].default == 100
    for name in ('cut_mix_data', 'cut_mix_batch_points', 'adjust_point_num', 'mixup_points'):
        assert getattr(vpn_amd, name) is getattr(A, name) is getattr(vpn_amd.modules, name)
    with pytest.raises(AssertionError):
        A.cut_mix_data(torch.rand(2, 3, 4), torch.rand(2, 1, 4, 4), torch.rand(2, 8, 3))
    with pytest.raises(AssertionError):
        A.mixup_points(torch.rand(8, 3))


def test_augmented_tensors_are_data_and_there_is_no_cpu_path():
    from vpn_amd import ops
    p = torch.rand(2, 8, 3)
    with pytest.raises(RuntimeError, match='gradients with respect'):
        ops.cutmix_points(p.clone().requires_grad_(True), None, 0.0, 1)
    with pytest.raises(RuntimeError, match='gradients with respect'):
        ops.mixup_points(p.clone().requires_grad_(True), None, 0.5)
    with pytest.raises(RuntimeError, match='gradients with respect'):
        ops.cutmix_images(torch.rand(2, 3, 4, 4).requires_grad_(True), None, None, 2)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.cutmix_points(p, None, 0.0, 1)
    with pytest.raises(ValueError):
        ops.partner_indices([0, 2], 2, 'cpu')


def test_g8_fixture_holds_the_four_case_kinds():
    path = os.path.join(GOLDEN, 'g8_cutmix.npz')
    assert os.path.getsize(path) <= SIZE_CAP
    with np.load(path, allow_pickle=False):
        pass
    z = load_golden('g8_cutmix')
    pts, rgbs, sils = z['points'], z['rgbs'], z['silhouettes']
    B, N, _ = pts.shape
    H, W = rgbs.shape[2:]
    assert H != W and W % 4 != 0 and sils.shape == (B, 1, H, W)
    kinds = set()
    assert int(z['n_seeds']) >= 3
    for k in range(int(z['n_seeds'])):
        g = lambda name: z['s%d_%s' % (k, name)]
        idx, cut, count, elig = g('indices'), float(g('point_cut_ratio')), g('count'), g('eligible').long()
        ratio = float(g('ratio'))
        torch.manual_seed(int(g('seed')))                       # the recorded draws are torch's under that seed
        assert 0.3 + torch.rand(1).item() * (0.7 - 0.3) == ratio and torch.equal(torch.randperm(B), idx)
        assert int(g('img_cut_index')) == int(W * ratio) and cut == (0.5 - ratio) * 2 * 0.30769
        ci = int(g('img_cut_index'))
        assert torch.equal(g('rgbs'), torch.cat([rgbs[..., :ci], rgbs[idx][..., ci:]], 3))
        assert torch.equal(g('silhouettes'), torch.cat([sils[..., :ci], sils[idx][..., ci:]], 3))
        assert int(count.min()) > 0
        for b in range(B):
            p, c = int(idx[b]), int(count[b])
            e = elig[b, :c]
            assert bool((elig[b, c:] == -1).all()) and bool((e[1:] > e[:-1]).all()) and int(e.max()) < 2 * N
            cand = torch.cat([pts[b], pts[p]])
            assert bool((cand[e[e < N], 2] >= cut).all()) and bool((cand[e[e >= N], 2] < cut).all())
            member = (g('points')[b][:, None, :] == cand[e][None]).all(2).any(1)
            assert bool(member.all())
            if c == N:
                assert torch.equal(g('points')[b], cand[e])
            kinds.add('fixed_point' if p == b else 'more' if c > N else 'fewer' if c < N else 'equal_other')
    assert kinds == {'more', 'fewer', 'equal_other', 'fixed_point'}


def test_augment_kernels_use_no_scratch():
    for kernel in ('cutmix_points_kernel', 'cutmix_images_kernelILb1', 'cutmix_images_kernelILb0', 'mixup_gather_kernel',
                   'mixup_lerp_kernel'):
        r = _resources('augment.hip', kernel)
        assert r['ScratchSize'] == 0, (kernel, r)
        assert r['LDS'] == 0, (kernel, r)            # only the dynamic part (vpn_cutmix_points_lds)
