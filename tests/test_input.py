"""GPU checks of the image input stage (modules/dataset.py::prepare_images, csrc/input.hip).  Every
comparison is exact (torch.equal): the 8-bit resized intermediate and the fp32 outputs against tests/input_ref.py (held
to PIL by tests/test_input_cpu.py) and against PIL's own results in the g10 fixture."""
import os

import numpy as np
import pytest
import torch

import input_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def g10():
    with np.load(os.path.join(GOLDEN, 'g10_input.npz'), allow_pickle=False) as z:
        return {k: np.array(z[k]) for k in z.files}


def _run(src, size, **kw):
    import vpn_amd
    from vpn_amd import ops
    from vpn_amd.modules.dataset import resized_size
    H, W = resized_size(src.shape[1], src.shape[2], size)
    kw.setdefault('jitter', kw.get('factors') is not None)
    kw.setdefault('rotate', kw.get('angles') is not None)
    rgb, sil, ang, inter = ops.prepare_images(torch.from_numpy(src).to(DEV), H, W, return_intermediate=True, **kw)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), sil.cpu().numpy(), ang.cpu().numpy(), inter.cpu().numpy()


def _planes(u8, normalize=False):
    """[B,H,W,4] uint8 -> (rgb [B,3,H,W], sil [B,1,H,W]) as ToTensor / Normalize give them."""
    outs = [R.to_outputs(x, normalize) for x in u8]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def _same(got, want_u8, normalize=False):
    rgb, sil = _planes(want_u8, normalize)
    assert np.array_equal(got[0], rgb) and np.array_equal(got[1], sil)


@pytest.mark.parametrize('name', ['d137', 'n41', 'u9'])
def test_fixture_cases_equal_pil(g10, name):
    z = g10
    src, (size, H, W), factors = z[name + '_src'], z[name + '_size'], z[name + '_factors']
    B = src.shape[0]
    plain = _run(src, size)                                                      # the resize alone: nothing gathered
    assert np.array_equal(plain[3], z[name + '_resized']) and not plain[2].any()
    _same(plain, z[name + '_resized'])
    if name == 'd137':
        got = _run(src, size, factors=factors, order=np.array(R.ORDERS[:B], np.int32))
        _same(got, z[name + '_jittered'])
        got = _run(src, size, factors=factors, order=np.array(R.ORDERS[:B], np.int32), angles=z['general_angles'][:B])
        _same(got, z[name + '_rotated'])
        assert np.array_equal(got[2], z['general_angles'][:B]) and np.array_equal(got[3], z[name + '_resized'])
        return
    for op in range(3):                                                          # each operation alone: the other two at 1.0
        for li, f in enumerate(z['factor_levels']):
            fs = np.ones((B, 3), np.float32)
            fs[:, op] = f
            _same(_run(src, size, factors=fs, order=np.tile(np.array(R.ORDERS[op * 2], np.int32), (B, 1))), z[name + '_single'][op, li])
    for oi, order in enumerate(z['orders']):
        for normalize in (False, True):
            got = _run(src, size, factors=factors, order=np.tile(order, (B, 1)), normalize=normalize)
            _same(got, z[name + '_jittered'][oi], normalize)
    own = np.array(R.ORDERS[:B], np.int32)
    angles = [float(a) for a in z['fast_angles']] + [float(a) for a in z['general_angles']]
    for ai, a in enumerate(angles):
        for normalize in (False, True):
            got = _run(src, size, factors=factors, order=own, angles=np.full(B, a, np.float32), normalize=normalize)
            _same(got, z[name + '_rotated'][ai], normalize)
            assert np.array_equal(got[2], np.full(B, a, np.float32))


@pytest.mark.parametrize('Hs,Ws,size', [(137, 137, 256), (37, 41, 16), (64, 64, 64), (300, 200, 17)])
def test_other_shapes_equal_the_restatement(g10, Hs, Ws, size):
    """137 -> 256: the intermediate exceeds one workgroup's LDS and spans many tiles; a wide image; an unchanged size
    (PIL copies: no premultiplication round trip); a steep reduction (13 taps)."""
    rng = np.random.default_rng(Hs + Ws + size)
    B = 3
    src = rng.integers(0, 256, (B, Hs, Ws, 4), dtype=np.uint8)
    src[0, ..., 3] = np.clip(rng.integers(-128, 384, (Hs, Ws)), 0, 255)
    src[1, ..., 3], src[2, ..., 3] = 255, 0
    factors = np.array([[0.6, 1.4, 1.0], [1.4, 0.6, 0.6], [1.0, 1.0, 1.4]], np.float32)
    order = np.array([R.ORDERS[1], R.ORDERS[3], R.ORDERS[4]], np.int32)
    angles = np.array([g10['general_angles'][0], 90.0, 180.0], np.float32)
    for normalize in (False, True):
        want = R.prepare_images(src, size, factors, order, angles, normalize, return_stages=True)
        got = _run(src, size, factors=factors, order=order, angles=angles, normalize=normalize)
        assert np.array_equal(got[3], want[3])
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    want = R.prepare_images(src, size, None, None, None)
    got = _run(src, size)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_philox_draws_shard_and_match_the_restatement(g10):
    import vpn_amd
    src = np.concatenate([g10['n41_src'], g10['n41_src'][:1, ::-1]])                       # B = 4
    dev_src = torch.from_numpy(src).to(DEV)
    full = vpn_amd.prepare_images(dev_src, size=16, rotate=True, seed=77)
    lo = vpn_amd.prepare_images(dev_src[:2], size=16, rotate=True, seed=77, sample_base=0)
    hi = vpn_amd.prepare_images(dev_src[2:], size=16, rotate=True, seed=77, sample_base=2)
    for k in range(3):
        assert torch.equal(full[k], torch.cat([lo[k], hi[k]]))
    f, o, a = R.draws(77, 0, 4)
    assert (f >= np.float32(0.6)).all() and (f <= np.float32(1.4)).all() and (a >= 0).all() and (a < 360).all()
    assert np.array_equal(full[2].cpu().numpy(), a)
    want = R.prepare_images(src, 16, f, o, a)
    assert np.array_equal(full[0].cpu().numpy(), want[0]) and np.array_equal(full[1].cpu().numpy(), want[1])
    # a given draw is taken as given, the others are still drawn
    mixed = vpn_amd.prepare_images(dev_src, size=16, rotate=True, seed=77, angles=torch.zeros(4))
    want = R.prepare_images(src, 16, f, o, np.zeros(4, np.float32))
    assert np.array_equal(mixed[0].cpu().numpy(), want[0]) and not mixed[2].any()


def test_returned_angles_rotate_the_points_the_same_way(g10):
    """The angle that comes back is the one the image was gathered with: a second call with that angle GIVEN reproduces the
    drawn call, and it is what rotate_points_forward_x_axis takes (degrees, [B])."""
    import vpn_amd
    dev_src = torch.from_numpy(g10['u9_src']).to(DEV)
    rgb, sil, ang = vpn_amd.prepare_images(dev_src, size=16, jitter=False, rotate=True, seed=5)
    assert ang.shape == (3,) and ang.dtype == torch.float32 and bool(((ang >= 0) & (ang < 360)).all())
    again = vpn_amd.prepare_images(dev_src, size=16, jitter=False, rotate=True, angles=ang)
    assert torch.equal(again[0], rgb) and torch.equal(again[1], sil) and torch.equal(again[2], ang)
    want = R.prepare_images(g10['u9_src'], 16, None, None, ang.cpu().numpy())
    assert np.array_equal(rgb.cpu().numpy(), want[0]) and np.array_equal(sil.cpu().numpy(), want[1])
    pts = torch.rand(3, 32, 3, device=DEV)
    turned = vpn_amd.rotate_points_forward_x_axis(pts, ang)
    q = torch.cat([torch.tensor([[1.0, 0.0, 0.0]], device=DEV).repeat(3, 1), (ang / 360).view(-1, 1)], 1)
    assert torch.equal(turned, vpn_amd.rotate_points(pts, q))
    none = vpn_amd.prepare_images(dev_src, size=16, jitter=False, rotate=False)
    assert not none[2].any()


def test_seed_dev_advances_and_torch_seed_reproduces(g10):
    import vpn_amd
    dev_src = torch.from_numpy(g10['n41_src']).to(DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    a0 = vpn_amd.prepare_images(dev_src, size=16, rotate=True, seed=100, seed_dev=step)
    step += 3
    a3 = vpn_amd.prepare_images(dev_src, size=16, rotate=True, seed=100, seed_dev=step)
    b0 = vpn_amd.prepare_images(dev_src, size=16, rotate=True, seed=100)
    b3 = vpn_amd.prepare_images(dev_src, size=16, rotate=True, seed=103)
    for k in range(3):
        assert torch.equal(a0[k], b0[k]) and torch.equal(a3[k], b3[k])
    assert not torch.equal(a0[2], a3[2])
    torch.manual_seed(9)
    x = vpn_amd.prepare_images(dev_src, size=16, rotate=True)
    y = vpn_amd.prepare_images(dev_src, size=16, rotate=True)
    torch.manual_seed(9)
    x2 = vpn_amd.prepare_images(dev_src, size=16, rotate=True)
    assert torch.equal(x[0], x2[0]) and torch.equal(x[2], x2[2]) and not torch.equal(x[2], y[2])


def test_no_host_synchronisation_and_graph_replay(g10):
    import vpn_amd
    src = g10['d137_src']
    dev_src = torch.from_numpy(src).to(DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    kw = dict(size=128, rotate=True, normalize=True, seed=11, seed_dev=step)
    eager = vpn_amd.prepare_images(dev_src, **kw)              # also uploads the cached tables before the strict region
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        strict = vpn_amd.prepare_images(dev_src, **kw)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vpn_amd.prepare_images(dev_src, **kw)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = vpn_amd.prepare_images(dev_src, **kw)
    graph.replay()
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(strict[k], eager[k]) and torch.equal(captured[k], eager[k])
    f, o, a = R.draws(11, 0, 3)
    want = R.prepare_images(src, 128, f, o, a, normalize=True)
    assert np.array_equal(eager[0].cpu().numpy(), want[0]) and np.array_equal(eager[2].cpu().numpy(), a)
    step += 1                                                  # the replay reads the counter: new draws, the same bits as eager
    graph.replay()
    torch.cuda.synchronize()
    kw['seed_dev'] = None
    kw['seed'] = 12
    fresh = vpn_amd.prepare_images(dev_src, **kw)
    for k in range(3):
        assert torch.equal(captured[k], fresh[k])
    assert not torch.equal(fresh[2], eager[2])


def test_sizes_beyond_the_limits_are_refused_before_a_launch():
    from vpn_amd import ops
    img = torch.zeros(1, 1040, 8, 4, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match='documented limit'):
        ops.prepare_images(img, 8, 8, jitter=False)            # 8 output rows span 1040 source rows: above 64 KB of LDS
    with pytest.raises(ValueError):
        ops.prepare_images(img, 8, 8, jitter=False, factors=torch.ones(1, 3))
    with pytest.raises(ValueError):
        ops.prepare_images(img, 8, 8, order=[[0, 1, 1]])
    with pytest.raises(ValueError):
        ops.prepare_images(img, 8, 8, rotate=True, angles=[0.0, 1.0])
