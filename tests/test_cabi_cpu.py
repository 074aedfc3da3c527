"""CPU-only checks of the drop-in boundary: the C-ABI library builds, loads and exports every
symbol include/vpn_hip.h declares, argument validation works without a GPU, and the host-side
mirror keeps the reference's names and signatures.  No compute call is made here."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT


def _header_symbols():
    src = open(os.path.join(ROOT, 'include', 'vpn_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(vpn_[a-z0-9_]+)\s*\(', src)))


def test_library_builds_and_exports_header_symbols():
    import importlib.util
    spec = importlib.util.spec_from_file_location('vpn_build', os.path.join(ROOT, 'volumetric-primitives-net_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    path = b.build(verbose=False)
    L = ctypes.CDLL(path)
    syms = _header_symbols()
    assert len(syms) >= 12
    for s in syms:
        assert hasattr(L, s), 'libvpn_hip.so does not export ' + s
    import vpn_amd._lib as lib
    assert sorted(lib.SIGNATURES) == syms, 'ctypes binding and header disagree'
    assert lib.lib().vpn_abi_version() == lib.ABI_VERSION


def test_argument_validation_needs_no_gpu():
    import vpn_amd._lib as lib
    L = lib.lib()
    assert L.vpn_chamfer_fwd(None, None, 1, 1, 1, None, None, None, None, None) == -1
    assert L.vpn_sample_fwd(None, None, None, 0, None, 0, 1, 1, 1, None, None) == -1
    assert L.vpn_raster_fwd(None, None, None, 1, 1, 8, 8, 0.1, 0.1, 2.0, None, None, None, None, None) == -1
    assert L.vpn_raster_loss_fwd(None, None, None, 1, 1, 8, 8, 0.1, 0.1, 2.0, None, None, 0, None, None, None, None, None) == -1
    assert L.vpn_raster_total_fwd(None, None, None, 1, 1, 8, 8, 0.1, 0.1, 2.0, None, None, 0, 1.0, 1.0, None, None, None, 0, None) == -1
    assert L.vpn_loss_finalize(None, 1, 8, 8, None, None, 0, 0, 1.0, 1.0, 1.0, 1.0, 1.0, None, None, None) == -1
    assert L.vpn_raster_total_bwd(None, None, 1, 1, 8, 8, None, None, None, None, 0, None) == -1
    assert L.vpn_camera_transform_fwd(None, None, None, None, None, 1, 8, 1, None, None) == -1
    assert L.vpn_raster_records_size(2, 3, 32, 32) == 2 * 3 * 16 * 16 + 2 * 4 * 8         # records + one mask word per tile
    assert L.vpn_raster_records_size(1, 65, 16, 16) == 65 * 16 * 16 + 2 * 8
    assert L.vpn_raster_bwd_workspace(2, 3, 32, 32) == 2 * 4 * 3 * 12 * 4
    assert L.vpn_raster_bwd_workspace(0, 3, 32, 32) == 0
    assert L.vpn_raster_loss_workspace(2, 32, 32) == 16 + 2 * 16 + 2 * 4 * 2 * 4
    # round-3 entry points: the fused raster + finalisation and the triangle-mesh path
    assert L.vpn_raster_total_fwd_fin(None, None, None, 1, 1, 8, 8, 0.1, 0.1, 2.0, None, None, 0, 1.0, 1.0, None, None, None, 0,
                                      None, 0, 0, 0, 1.0, 1.0, 1.0, None, None, None, None, None) == -1
    assert L.vpn_mesh_raster_fwd(None, None, None, 1, 3, 1, 8, 8, 1e-4, None, None, None) == -1
    assert L.vpn_mesh_raster_bwd(None, None, None, 1, 3, 1, 8, 8, 1e-4, None, None, None, None, None) == -1
    assert L.vpn_mesh_sample_fwd(None, None, None, 0, 0, 1, 3, 1, 8, None, None, None, None, None) == -1
    assert L.vpn_mesh_sample_bwd(None, None, None, None, 1, 3, 1, 8, None, None) == -1
    assert L.vpn_mesh_raster_workspace(2, 10) == 2 * 10 * (16 + 8) and L.vpn_mesh_raster_workspace(0, 10) == 0
    assert L.vpn_emd_workspace(2, 100) == 2 * 100 * 10 * 4 + 16
    assert b'null pointer' in L.vpn_error_string(-1)
    with pytest.raises(RuntimeError):
        lib.check(-2)


def test_no_cpu_fallback():
    """The product path must fail loudly on CPU tensors (no oracle / eager fallback)."""
    import vpn_amd
    p = torch.rand(1, 4, 3)
    with pytest.raises(RuntimeError, match='GPU only'):
        vpn_amd.ChamferDistanceLoss()(p, p)
    with pytest.raises(RuntimeError, match='GPU only'):
        vpn_amd.Sampling.sphere_sampling(torch.rand(1, 3), torch.rand(1, 4), torch.rand(1, 3), 8)
    src = ''
    pkg = os.path.join(ROOT, 'volumetric-primitives-net_amd')
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src += open(os.path.join(root, f)).read()
    assert not re.search(r'^\s*(from|import)\s+\S*oracle', src, flags=re.M), 'the package must not import the oracle'
    assert 'vpn_oracle.' not in re.sub(r'#.*', '', re.sub(r'"""(.|\n)*?"""', '', src))


def test_reference_surface_is_mirrored():
    """Names / argument order of the reference call sites."""
    import vpn_amd
    from vpn_amd.modules import sampling, loss, render, transform, meshing
    sig = inspect.signature
    # kaolin's TriangleMesh as train_sphere.py:50-78 uses it
    for name in ('from_obj', 'cuda', 'sample', 'vertices', 'faces'):
        assert hasattr(meshing.TriangleMesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)), name) or hasattr(meshing.TriangleMesh, name)
    assert list(sig(meshing.TriangleMesh.sample).parameters)[:2] == ['self', 'num_samples']
    assert list(sig(sampling.Sampling.sphere_sampling).parameters)[:4] == ['v', 'q', 't', 'num_points']
    assert list(sig(sampling.Sampling.cuboid_sampling).parameters)[:4] == ['v', 'q', 't', 'num_points']
    assert sig(sampling.Sampling.sphere_sampling).parameters['num_points'].default == 1000
    assert sampling.Sampling.cone_sampling(None, None, None) is None
    assert list(sig(loss.ChamferDistanceLoss.forward).parameters) == ['self', 'points1', 'points2', 'each_batch', 'w1', 'w2']
    assert list(sig(loss.VPDiverseLoss.forward).parameters) == ['self', 'translates', 'gt_points']
    assert list(sig(loss.SilhouetteLoss.forward).parameters) == ['self', 'predict_meshes', 'gt_silhouettes', 'dists', 'elevs', 'azims']
    assert list(sig(render.VertexRenderer.render).parameters)[:5] == ['mesh', 'dist', 'elev', 'azim', 'colors']
    assert list(sig(transform.transform_points).parameters) == ['points', 'q', 't']
    assert list(sig(transform.view_to_obj_points).parameters) == ['points', 'dists', 'elevs', 'azims', 'angles']
    # shape assertions like the reference
    with pytest.raises(AssertionError):
        vpn_amd.Sampling.check_parameters(torch.rand(2, 3), torch.rand(2, 3), torch.rand(2, 3))
    with pytest.raises(AssertionError):
        vpn_amd.ChamferDistanceLoss.check_parameters(torch.rand(2, 3))
    with pytest.raises(ValueError):
        vpn_amd.kinds_from_counts(0, 1, cone_num=1)
    with pytest.raises(ValueError):
        vpn_amd.kinds_tensor([0, 2], torch.device('cpu'))
    assert vpn_amd.kinds_from_counts(1, 2) == [1, 0, 0]          # cuboids first (train.py:112-116)
    v = [torch.rand(2, 3) for _ in range(3)]
    q = [torch.rand(2, 4) for _ in range(3)]
    t = [torch.rand(2, 3) for _ in range(3)]
    p = vpn_amd.pack_primitives(v, q, t)
    assert p.shape == (2, 3, 10) and torch.equal(p[:, 1, 3:7], q[1])


# ---- the binding is derived from include/vpn_hip.h (_lib._header_constants / _header_signatures)

def test_derived_signatures_equal_the_frozen_rows():
    """Rows of the hand-written table the reader replaced, kept as they stood: between them every type kind the header uses
    and the longest parameter lists (vpn_profile_read with all pointers as void*, the reader's uniform rule)."""
    import vpn_amd._lib as lib
    _c_f = ctypes.c_void_p
    _i, _f, _u64, _sz = ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_size_t
    FcStack, FcGrad = lib.FcStack, lib.FcGrad
    frozen = {
        'vpn_trainstep_bwd': (_i, [_c_f, _c_f, _u64, _c_f, _u64, _i, _i, _i, _c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _f, _f, _c_f, _i, _i,
                                   _c_f, _c_f, _c_f, _c_f, _c_f, _f, _c_f, _c_f, _c_f, _c_f, _f, _f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f,
                                   _f, _f, _i, _c_f, _c_f]),
        'vpn_raster_total_fwd_fin': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _f, _f, _f, _c_f, _c_f, _i, _f, _f, _c_f, _c_f, _c_f, _i,
                                          _c_f, _sz, _i, _i, _f, _f, _f, _c_f, _c_f, _c_f, _c_f, _c_f]),
        'vpn_gcn_input_fwd': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _i] + [_c_f] * 4 + [_i] * 12 + [_c_f] * 6),
        'vpn_fc_stack_bwd': (_i, [FcStack, FcGrad, _i, _f, _u64, _c_f, _i, _i, _i, _f, _f, _f, _f, _f, _c_f, _sz, _c_f]),
        'vpn_ragged_sample': (_i, [_c_f] * 7 + [ctypes.c_uint, _c_f, _u64, _c_f, _u64] + [_i] * 6 + [_c_f, _sz] + [_c_f] * 4),
        'vpn_prepare_images': (_i, [_c_f, _c_f, _i, _i, _i, _c_f, _c_f, _c_f, _u64, _c_f, _u64] + [_i] * 6 + [_c_f, _sz] + [_c_f] * 5),
        'vpn_vis_mesh': (_i, [_c_f, _c_f, _c_f, _c_f, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _c_f, _c_f, _sz, ctypes.c_longlong, _c_f, _c_f]),
        'vpn_emd_fwd_ex': (_i, [_c_f, _c_f, _i, _i, _f, _i, _c_f, _c_f, _c_f, _i, _c_f, ctypes.c_uint]),
        'vpn_emd_recovered_samples': (ctypes.c_longlong, []),
        'vpn_error_string': (ctypes.c_char_p, [_i]),
        'vpn_chamfer_workspace': (_sz, [_i, _i, _i]),
        'vpn_profile_read': (_i, [_c_f, _i, _c_f, _c_f, _i]),
    }
    assert len(frozen['vpn_trainstep_bwd'][1]) == 44 and len(frozen['vpn_raster_total_fwd_fin'][1]) == 31
    for name, (res, args) in frozen.items():
        got_res, got_args = lib.SIGNATURES[name]
        assert got_res is res, name
        assert [t.__name__ for t in got_args] == [t.__name__ for t in args], name
        assert all(a is b for a, b in zip(got_args, args)), name


def test_header_reader_on_its_own_text():
    import vpn_amd._lib as lib
    sig = lambda text: lib._header_signatures(text, lib.BY_VALUE)
    with pytest.raises(RuntimeError, match='vpn_x.*double'):              # a type outside the map is an error that names the place
        sig('int vpn_x(double y);')
    with pytest.raises(RuntimeError, match='vpn_x.*double'):
        sig('double vpn_x(int y);')
    with pytest.raises(RuntimeError, match='vpn_x'):                      # ... and so is a pointer result that is no C string
        sig('float* vpn_x(int y);')
    split = '''#define VPN_LIMIT 4
    size_t vpn_two_lines(const float* a,   /* first [B,3] */
                         int n, /* a block comment
                         over two lines, with a (parenthesis) and a vpn_name( in it */ uint64_t seed,
                         const long long* offsets, unsigned mask,   // a line comment; with a semicolon
                         long long pitch, VpnFcStack stack,
                         void* stream);
    int vpn_none(void);
    const char* vpn_text(int code);'''
    got = sig(split)
    assert got == {'vpn_two_lines': (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint,
                                                       ctypes.c_longlong, lib.FcStack, ctypes.c_void_p]),
                   'vpn_none': (ctypes.c_int, []),
                   'vpn_text': (ctypes.c_char_p, [ctypes.c_int])}
    assert sig('int vpn_empty();') == {'vpn_empty': (ctypes.c_int, [])}
    consts = lib._header_constants('#define VPN_E_BADARG (-1)\n#define VPN_E_TOOBIG  ( -2 )   /* too big */\n#define VPN_N 12 // twelve\n'
                                   '#define VPN_HIP_H\n#define VPN_RATIO 0.5f\n/* #define VPN_GONE 3 */\n#define OTHER 7\n')
    assert consts == {'VPN_E_BADARG': -1, 'VPN_E_TOOBIG': -2, 'VPN_N': 12}


def test_python_constants_are_the_headers():
    """Every limit and flag the package names is the header's #define (read here with this test's own pattern); the two that
    are properties of the kernels, and from which other tests build shapes, are pinned as numbers too."""
    import vpn_amd._lib as lib
    from vpn_amd import ops
    from vpn_amd.modules import dataset
    hdr = open(os.path.join(ROOT, 'include', 'vpn_hip.h')).read()

    def define(name):
        found = re.findall(r'^#define %s +\(?(-?\d+)\)?' % name, hdr, flags=re.M)
        assert len(found) == 1, name
        return int(found[0])

    pairs = [(lib.ABI_VERSION, 'VPN_ABI_VERSION'), (lib.FC_MAX_LAYERS, 'VPN_FC_MAX_LAYERS'), (lib.FC_MAX_SLOTS, 'VPN_FC_MAX_SLOTS'),
             (lib.FC_NONE, 'VPN_FC_NONE'), (lib.FC_TANH, 'VPN_FC_TANH'), (lib.FC_VP_PACK, 'VPN_FC_VP_PACK'),
             (lib.FC_DROPOUT_OFF, 'VPN_FC_DROPOUT_OFF'), (lib.FC_DROPOUT_MASK, 'VPN_FC_DROPOUT_MASK'),
             (lib.FC_DROPOUT_PHILOX, 'VPN_FC_DROPOUT_PHILOX'), (ops.SPHERE, 'VPN_SPHERE'), (ops.CUBOID, 'VPN_CUBOID'),
             (ops.PARAM_STRIDE, 'VPN_PARAM_STRIDE'), (ops.RAGGED_MAX_SETS, 'VPN_RAGGED_MAX_SETS'), (ops.INPUT_JITTER, 'VPN_INPUT_JITTER'),
             (ops.INPUT_ROTATE, 'VPN_INPUT_ROTATE'), (ops.INPUT_NORMALIZE, 'VPN_INPUT_NORMALIZE'),
             (ops.FUSED_BWD_MAX_GT, 'VPN_FUSED_BWD_MAX_GT'), (ops.INPUT_TILE_ROWS, 'VPN_INPUT_TILE_ROWS'),
             (dataset.CHUNK, 'VPN_RAGGED_CHUNK')]
    for value, name in pairs:
        assert type(value) is int and value == define(name), name
    assert lib.CONSTANTS['VPN_E_BADARG'] == define('VPN_E_BADARG') == -1 and lib.CONSTANTS['VPN_E_TOOBIG'] == define('VPN_E_TOOBIG') == -2
    assert ops.FUSED_BWD_MAX_GT == 7680 and ops.INPUT_TILE_ROWS == 8
    assert ctypes.sizeof(lib.FcStack) == 4 * 4 + define('VPN_FC_MAX_SLOTS') * (2 * 4 + 5 * 8)


def test_tile_rider_fits_is_the_old_arithmetic():
    """vpn_hotpath_tile_rider_fits (host arithmetic, no GPU) against the Python expression it replaced."""
    import vpn_amd._lib as lib
    from vpn_amd import ops

    def lds(K, H, W):
        return K * 84 + (K + 2) * 4 + ((W + 15) // 16) * ((H + 15) // 16)

    def old(K, H, W):
        return K <= 64 and ((W + 15) // 16) * ((H + 15) // 16) <= 16384 and lds(K, H, W) <= 24576

    k_lds = next(K for K in range(1, 1 << 12) if lds(K, 128, 128) > 24576)      # the first K whose scratch outgrows the scan's LDS
    cases = [(16, 128, 128), (64, 128, 128), (65, 128, 128), (1, 2048, 2048), (64, 2048, 2048), (1, 1808, 2320), (1, 2048, 2049),
             (k_lds - 1, 128, 128), (k_lds, 128, 128), (16, 127, 129), (16, 1, 1)]
    assert (2048 // 16) ** 2 == 16384 and (1808 // 16) * (2320 // 16) == 16385 and lds(k_lds - 1, 128, 128) <= 24576
    assert old(16, 128, 128) and old(64, 2048, 2048) and not old(65, 128, 128) and not old(1, 1808, 2320)
    L = lib.lib()
    for K, H, W in cases:
        assert L.vpn_hotpath_tile_rider_fits(K, H, W) == int(old(K, H, W)), (K, H, W)
        assert bool(ops._tile_rider_fits(K, H, W)) == (ops.TILE_ORDER and old(K, H, W)), (K, H, W)
