"""CPU checks of the image input stage (modules/dataset.py::prepare_images, csrc/input.hip): the
restatement tests/input_ref.py equals the installed PIL exactly after every operation, on every case of the g10 fixture
and at the sizes the GPU tests use; the fixture regenerates identically; the entry points exist under ABI 9 and validate
their arguments without a GPU; the Resize(int) size rule, the host-side coefficient tables and the Python-side validation;
no new kernel uses scratch."""
import ctypes
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

import input_ref as R
from conftest import GOLDEN, ROOT
from test_kernel_budget_cpu import _resources
from PIL import Image, ImageEnhance

ENHANCERS = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)
CASES = ('d137', 'n41', 'u9')


@pytest.fixture(scope='module')
def g10():
    with np.load(os.path.join(GOLDEN, 'g10_input.npz'), allow_pickle=False) as z:
        return {k: np.array(z[k]) for k in z.files}


def _tool():
    spec = importlib.util.spec_from_file_location('make_golden_input', os.path.join(ROOT, 'tools', 'make_golden_input.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _angles(z):
    return [float(a) for a in z['fast_angles']] + [float(a) for a in z['general_angles']]


def test_fixture_regenerates_identically_and_is_small(g10):
    assert os.path.getsize(os.path.join(GOLDEN, 'g10_input.npz')) <= 256 * 1024
    again = _tool().build()
    assert sorted(again) == sorted(g10)
    for k, v in again.items():
        assert v.dtype == g10[k].dtype and np.array_equal(v, g10[k]), k


def test_fixture_holds_the_stated_cases(g10):
    tool = _tool()
    for name in CASES:
        src, (size, H, W) = g10[name + '_src'], g10[name + '_size']
        assert (H, W) == R.resized_hw(src.shape[1], src.shape[2], size)
        assert (src[1, ..., 3] == 255).all() and (src[2, ..., 3] == 0).all()              # fully opaque, fully transparent
        a = src[0, ..., 3]
        assert (a == 0).any() and (a == 255).any() and ((a > 0) & (a < 255)).any()
        f = g10[name + '_factors']
        assert f.dtype == np.float32 and (f >= 0.6).all() and (f <= 1.4).all()
    assert g10['n41_size'][1] != g10['n41_size'][2]                                       # non-square: 90 / 270 are general
    assert sorted(map(tuple, g10['orders'])) == sorted(R.ORDERS) and len(g10['orders']) == 6
    sizes = [tuple(g10[n + '_size'][1:]) for n in CASES]
    for a in g10['general_angles']:
        assert float(a) % 90.0 != 0.0
        for H, W in sizes:
            assert not tool.near_tie(float(a), int(H), int(W))
            fixed, raw = R.rotation_coefficients(float(a), int(H), int(W))
            for v in raw:                                                                 # 1e-6 clear of a rounding tie
                t = v * 65536.0 + 0.5
                assert abs(t - round(t)) >= 1e-6


@pytest.mark.parametrize('name', CASES)
def test_restatement_equals_the_fixture_after_every_operation(g10, name):
    z = g10
    src, (size, H, W), factors = z[name + '_src'], z[name + '_size'], z[name + '_factors']
    B = src.shape[0]
    resized = np.stack([R.resize(src[b], H, W) for b in range(B)])
    assert np.array_equal(resized, z[name + '_resized'])
    if name == 'd137':
        jit = [R.jitter(resized[b], factors[b], R.ORDERS[b]) for b in range(B)]
        assert np.array_equal(np.stack(jit), z[name + '_jittered'])
        rot = [R.rotate(jit[b], z['general_angles'][b]) for b in range(B)]
        assert np.array_equal(np.stack(rot), z[name + '_rotated'])
        return
    for op in range(3):
        for li, f in enumerate(z['factor_levels']):
            got = np.stack([R.enhance(resized[b], op, f) for b in range(B)])
            assert np.array_equal(got, z[name + '_single'][op, li]), (op, f)
    for oi, order in enumerate(z['orders']):
        got = np.stack([R.jitter(resized[b], factors[b], order) for b in range(B)])
        assert np.array_equal(got, z[name + '_jittered'][oi]), order
    for ai, a in enumerate(_angles(z)):
        got = np.stack([R.rotate(z[name + '_jittered'][b, b], a) for b in range(B)])
        assert np.array_equal(got, z[name + '_rotated'][ai]), a


@pytest.mark.parametrize('Hs,Ws,size', [(137, 137, 128), (41, 37, 16), (9, 9, 16), (137, 137, 256), (37, 41, 16), (64, 64, 64),
                                        (300, 200, 17)])
def test_restatement_equals_the_installed_pil(g10, Hs, Ws, size):
    """Live against PIL, beyond the fixture: noise images with every kind of alpha, each enhancer at and outside [0, 1],
    all six orders, the transposes and general angles, negative and beyond 360."""
    rng = np.random.default_rng(Hs * 1000 + Ws + size)
    H, W = R.resized_hw(Hs, Ws, size)
    for kind in range(3):
        a = rng.integers(0, 256, (Hs, Ws, 4), dtype=np.uint8)
        if kind == 0:
            a[..., 3] = np.clip(rng.integers(-128, 384, (Hs, Ws)), 0, 255)
        else:
            a[..., 3] = 255 if kind == 1 else 0
        r = R.resize(a, H, W)
        assert np.array_equal(r, np.asarray(Image.fromarray(a, 'RGBA').resize((W, H), Image.BILINEAR)))
        im = Image.fromarray(r, 'RGBA')
        for f in (0.6, 1.0, 1.4, 0.0, 0.873, 1.7):
            f = float(np.float32(f))
            for op, E in enumerate(ENHANCERS):
                assert np.array_equal(R.enhance(r, op, f), np.asarray(E(im).enhance(f))), (op, f)
        fs = rng.uniform(0.6, 1.4, 3).astype(np.float32)
        for order in R.ORDERS:
            p = im
            for op in order:
                p = ENHANCERS[op](p).enhance(float(fs[op]))
            assert np.array_equal(R.jitter(r, fs, order), np.asarray(p)), order
        for ang in [0.0, 90.0, 180.0, 270.0, 360.0, 450.0, -17.0] + [float(x) for x in g10['general_angles']]:
            p = im.rotate(ang, Image.NEAREST, False, None, fillcolor=(0, 0, 0, 0))
            assert np.array_equal(R.rotate(r, ang), np.asarray(p)), ang


def test_to_tensor_levels_and_normalisation():
    lv = np.arange(256, dtype=np.uint8)
    rgba = np.stack([lv, lv[::-1], lv, lv], -1)[None]                  # [1,256,4]
    rgb, sil = R.to_outputs(rgba)
    t = torch.from_numpy(rgba).permute(2, 0, 1).float().div(255)       # ToTensor
    assert np.array_equal(rgb, t[:3].numpy()) and np.array_equal(sil, t[3:].numpy())
    assert np.array_equal((t * 255).byte().numpy(), np.moveaxis(rgba, -1, 0))       # ToPILImage restores every level
    from vpn_amd.modules.dataset import split_rgba
    nrgb, nsil = split_rgba(t, normalize=True)
    rgb, sil = R.to_outputs(rgba, normalize=True)
    assert np.array_equal(rgb, nrgb.numpy()) and np.array_equal(sil, nsil.numpy())


def test_resize_int_size_rule():
    from vpn_amd.modules.dataset import resized_size
    assert resized_size(137, 137, 128) == (128, 128)
    assert resized_size(41, 37, 16) == (17, 16) and resized_size(37, 41, 16) == (16, 17)
    assert resized_size(9, 9, 16) == (16, 16)
    assert resized_size(300, 200, 17) == (25, 17) and resized_size(200, 300, 17) == (17, 25)
    assert resized_size(100, 333, 7) == (7, int(7 * 333 / 100))
    for hs, ws, s in ((5, 9, 3), (480, 640, 224), (1, 7, 2)):
        assert resized_size(hs, ws, s) == R.resized_hw(hs, ws, s)
        w, h = Image.new('RGBA', (ws, hs)).size
        short, long = (w, h) if w <= h else (h, w)                     # torchvision's _compute_resized_output_size
        want = (int(s * long / short), s) if w <= h else (s, int(s * long / short))
        assert resized_size(hs, ws, s) == want
    with pytest.raises(ValueError):
        resized_size(0, 4, 8)
    with pytest.raises(ValueError):
        resized_size(4, 4, 0)


def test_host_coefficient_tables():
    from vpn_amd import ops
    for n_in, n_out in ((137, 128), (137, 256), (9, 16), (41, 17), (37, 16), (64, 64), (300, 17)):
        b, k = ops.input_filter_table(n_in, n_out)
        rb, rk = R.filter_table(n_in, n_out)
        assert b.dtype == k.dtype == torch.int32
        assert np.array_equal(b.numpy(), rb) and np.array_equal(k.numpy(), rk)
        support = max(n_in / n_out, 1.0)
        assert k.shape == (n_out, int(np.ceil(support)) * 2 + 1)
        assert int(b[:, 0].min()) >= 0 and int((b[:, 0] + b[:, 1]).max()) <= n_in and int(b[:, 1].min()) >= 1
        assert int(b[:, 1].max()) <= k.shape[1] and bool((k >= 0).all())
        assert bool(((k.sum(1) - (1 << 22)).abs() <= k.shape[1]).all())          # each row sums to one in 22 bits, up to rounding
        for i in range(n_out):
            assert bool((k[i, int(b[i, 1]):] == 0).all())
    b, k = ops.input_filter_table(64, 64)                                        # unchanged size: the identity filter
    assert bool((k[:, 0] == 1 << 22).all()) and bool((k[:, 1:] == 0).all()) and b[:, 0].tolist() == list(range(64))
    t, ksh, ksv, rows = ops.input_tables(41, 37, 17, 16, 'cpu')
    assert t.dtype == torch.int32 and t.numel() == 16 * 2 + 16 * ksh + 17 * 2 + 17 * ksv
    vb = t[16 * 2 + 16 * ksh:][:17 * 2].reshape(17, 2)
    assert rows == max(int(vb[min(y + 8, 17) - 1].sum()) - int(vb[y, 0]) for y in range(0, 17, 8))
    assert ops.input_tables(41, 37, 17, 16, 'cpu')[0] is t                       # cached per (sizes, device)


def test_entry_points_exist_and_validate_without_a_gpu():
    import vpn_amd._lib as lib
    L = lib.lib()
    assert L.vpn_abi_version() == lib.ABI_VERSION == 9
    assert L.vpn_input_ws(0) == 0 and L.vpn_input_ws(3) == 3 * (8 + 64)
    f = ctypes.c_void_p(64)              # never dereferenced: every call below is refused before a launch

    def call(rgba=f, tab=f, ksh=5, ksv=5, rows=10, B=2, Hs=9, Ws=9, H=16, W=16, flags=7, ws=f, wsb=1 << 20, inter=f):
        return L.vpn_prepare_images(rgba, tab, ksh, ksv, rows, None, None, None, 1, None, 0, B, Hs, Ws, H, W, flags, ws, wsb,
                                    inter, f, f, f, None)
    assert call(rgba=None) == -1 and call(tab=None) == -1 and call(ws=None) == -1 and call(inter=None) == -1
    assert call(B=0) == -1 and call(H=0) == -1 and call(Ws=-1) == -1 and call(ksh=0) == -1 and call(rows=0) == -1
    assert call(flags=8) == -1
    assert call(rgba=ctypes.c_void_p(66)) == -1                                  # pixels are read as 4-byte words
    assert call(wsb=2 * 72 - 1) == -1
    assert call(Hs=8193) == -2 and call(W=8193) == -2 and call(B=65536) == -2
    assert call(B=4096, H=512, W=512) == -2                                      # B H W >= 2^29
    assert call(rows=513) == -2                                                  # the staged rows of a tile exceed 64 KB of LDS
    assert b'documented limit' in L.vpn_error_string(-2)


def test_module_interface_and_validation():
    import vpn_amd
    from vpn_amd import ops
    from vpn_amd.modules import dataset as D
    assert vpn_amd.prepare_images is D.prepare_images is vpn_amd.modules.prepare_images
    p = inspect.signature(D.prepare_images).parameters
    assert list(p)[0] == 'rgba_u8'
    for n in ('size', 'jitter', 'rotate', 'normalize', 'factors', 'order', 'angles', 'seed', 'sample_base', 'seed_dev'):
        assert p[n].kind == inspect.Parameter.KEYWORD_ONLY
    assert (p['size'].default, p['jitter'].default, p['rotate'].default, p['normalize'].default) == (None, True, False, False)
    assert D.IMAGENET_MEAN == R.IMAGENET_MEAN and D.IMAGENET_STD == R.IMAGENET_STD
    img = torch.zeros(2, 9, 9, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='GPU only'):
        D.prepare_images(img, size=16, jitter=False)
    with pytest.raises(AssertionError):
        D.prepare_images(img[0], size=16)
    with pytest.raises(ValueError):
        ops.prepare_images(img.float(), 16, 16)
    with pytest.raises(ValueError):
        ops.prepare_images(img.permute(0, 3, 1, 2), 16, 16)


def test_draw_restatement_ranges_and_sharding():
    f, o, a = R.draws(1234, 0, 64)
    assert f.dtype == np.float32 and (f >= np.float32(0.6)).all() and (f <= np.float32(1.4)).all()
    assert a.dtype == np.float32 and (a >= 0).all() and (a < 360).all()
    assert all(sorted(r) == [0, 1, 2] for r in o.tolist()) and len(set(map(tuple, o.tolist()))) == 6
    f2, o2, a2 = R.draws(1234, 32, 32)
    assert np.array_equal(f[32:], f2) and np.array_equal(o[32:], o2) and np.array_equal(a[32:], a2)
    assert not np.array_equal(R.draws(1235, 0, 64)[0], f)


def test_input_kernels_use_no_scratch():
    for kernel, vgprs in (('input_setup_kernel', 64), ('input_resize_kernel', 64), ('input_finish_kernel', 64)):
        r = _resources('input.hip', kernel)
        assert r['ScratchSize'] == 0, (kernel, r)
        assert r['LDS'] == 0, (kernel, r)            # only the dynamic part: 128 bytes per staged source row
        assert r['VGPRs'] + r.get('AGPRs', 0) <= vgprs, (kernel, r)          # eight waves per SIMD


def test_resize_kernel_packs_without_the_half_writing_shift():
    """in_clip8 (csrc/input.hip): hipcc fuses the signed clamp of two shifted sums into v_ashr_pk_u8_i32, whose upper
    destination half kept an accumulator's bits on the MI355X; the unsigned form must keep that instruction out."""
    import subprocess
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'volumetric-primitives-net_amd'))
    spec = importlib.util.spec_from_file_location('vpn_build', os.path.join(ROOT, 'volumetric-primitives-net_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    cmd = [b.hipcc()] + b.COMMON + b.PER_FILE['input.hip'] + ['--cuda-device-only', '-S', os.path.join(b.CSRC, 'input.hip'),
                                                              '-o', '-']
    asm = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stdout
    assert 'input_resize_kernel' in asm and 'v_ashr_pk_u8_i32' not in asm
