"""ctypes binding of libvpn_hip.so (C ABI declared in include/vpn_hip.h).

There is no CPU or PyTorch fallback: if the library is missing or a call fails the
binding raises.  PyTorch is used only for device memory and the current HIP stream."""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('VPN_HIP_LIB') or os.path.join(_HERE, 'libvpn_hip.so')     # VPN_HIP_LIB: the sanitizer build of the tests
ABI_VERSION = 9

_c_f = ctypes.c_void_p      # device pointers travel as void*
_i, _f, _u64, _sz = ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_size_t

FC_MAX_LAYERS, FC_MAX_SLOTS = 8, 24      # VPN_FC_MAX_LAYERS, VPN_FC_MAX_SLOTS
FC_NONE, FC_TANH, FC_VP_PACK = 0, 1, 2
FC_DROPOUT_OFF, FC_DROPOUT_MASK, FC_DROPOUT_PHILOX = 0, 1, 2


class FcStack(ctypes.Structure):
    """VpnFcStack of include/vpn_hip.h, passed by value: slot g * L + l is layer l of group g."""
    _fields_ = [('G', ctypes.c_int32), ('L', ctypes.c_int32), ('B', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('in0', ctypes.c_int32 * FC_MAX_SLOTS), ('out', ctypes.c_int32 * FC_MAX_SLOTS),
                ('x', ctypes.c_void_p * FC_MAX_SLOTS), ('w', ctypes.c_void_p * FC_MAX_SLOTS),
                ('bias', ctypes.c_void_p * FC_MAX_SLOTS), ('keep', ctypes.c_void_p * FC_MAX_SLOTS),
                ('act', ctypes.c_void_p * FC_MAX_SLOTS)]


class FcGrad(ctypes.Structure):
    """VpnFcGrad of include/vpn_hip.h, passed by value."""
    _fields_ = [('gout', ctypes.c_void_p * FC_MAX_SLOTS), ('dw', ctypes.c_void_p * FC_MAX_SLOTS),
                ('db', ctypes.c_void_p * FC_MAX_SLOTS), ('dx', ctypes.c_void_p * FC_MAX_SLOTS)]


SIGNATURES = {
    'vpn_abi_version': (ctypes.c_int, []),
    'vpn_error_string': (ctypes.c_char_p, [_i]),
    'vpn_profile_enable': (_i, [_i]),
    'vpn_profile_read': (_i, [ctypes.c_char_p, _i, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int), _i]),
    'vpn_sample_fwd': (_i, [_c_f, _c_f, _c_f, _u64, _c_f, _u64, _i, _i, _i, _c_f, _c_f]),
    'vpn_sample_bwd': (_i, [_c_f, _c_f, _c_f, _u64, _c_f, _u64, _i, _i, _i, _c_f, _c_f, _c_f]),
    'vpn_sample_chamfer_bwd': (_i, [_c_f, _c_f, _c_f, _u64, _c_f, _u64, _i, _i, _i, _c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _c_f,
                                    _f, _f, _c_f, _c_f]),
    'vpn_transform_fwd': (_i, [_c_f, _c_f, _c_f, _i, _i, _c_f, _c_f]),
    'vpn_transform_bwd': (_i, [_c_f, _c_f, _c_f, _i, _i, _c_f, _c_f, _c_f, _c_f]),
    'vpn_chamfer_fwd': (_i, [_c_f, _c_f, _i, _i, _i, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'vpn_chamfer_nn': (_i, [_c_f, _c_f, _i, _i, _i, _c_f, _c_f, _c_f]),
    'vpn_chamfer_workspace': (_sz, [_i, _i, _i]),
    'vpn_chamfer_fwd_ws': (_i, [_c_f, _c_f, _i, _i, _i, _c_f, _c_f, _c_f, _c_f, _c_f, _sz, _i, _c_f]),
    'vpn_chamfer_loss': (_i, [_c_f, _c_f, _i, _i, _i, _f, _f, _c_f, _c_f]),
    'vpn_chamfer_bwd': (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i, _i, _i, _f, _f, _c_f, _c_f, _c_f]),
    'vpn_raster_records_size': (_sz, [_i, _i, _i, _i]),
    'vpn_raster_fwd': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _f, _f, _f, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'vpn_raster_bwd_workspace': (_sz, [_i, _i, _i, _i]),
    'vpn_raster_bwd': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _f, _f, _f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'vpn_raster_loss_workspace': (_sz, [_i, _i, _i]),
    'vpn_raster_loss_fwd': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _f, _f, _f, _c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'vpn_raster_total_fwd': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _f, _f, _f, _c_f, _c_f, _i, _f, _f, _c_f, _c_f, _c_f, _i, _c_f]),
    'vpn_raster_total_fwd_fin': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _f, _f, _f, _c_f, _c_f, _i, _f, _f, _c_f, _c_f, _c_f, _i,
                                      _c_f, _sz, _i, _i, _f, _f, _f, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'vpn_hotpath_sample_fwd': (_i, [_c_f, _c_f, _c_f, _u64, _c_f, _u64, _i, _i, _i, _c_f, _c_f, _i, _i, _f, _c_f, _c_f,
                                    _c_f, _i, _c_f, _sz, _c_f]),
    'vpn_hotpath_fused_features': (_i, [_i, _i, _i, _i]),
    'vpn_raster_order_size': (_sz, [_i, _i, _i]),
    'vpn_hotpath_chamfer_fwd': (_i, [_c_f, _c_f, _i, _i, _i, _c_f, _c_f, _c_f, _c_f, _c_f, _sz, _i, _c_f, _i, _i, _i, _c_f, _c_f]),
    'vpn_loss_finalize': (_i, [_c_f, _i, _i, _i, _c_f, _c_f, _i, _i, _f, _f, _f, _f, _f, _c_f, _c_f, _c_f]),
    'vpn_raster_total_bwd': (_i, [_c_f, _c_f, _i, _i, _i, _i, _c_f, _c_f, _c_f, _c_f, _i, _c_f]),
    'vpn_hotpath_bwd': (_i, [_c_f, _c_f, _c_f, _u64, _c_f, _u64, _i, _i, _i, _c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _c_f,
                             _f, _f, _c_f, _i, _i, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'vpn_raster_loss_bwd': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _f, _f, _f, _c_f, _c_f, _c_f, _c_f, _i, _c_f, _c_f, _c_f,
                                 _i, _c_f]),
    'vpn_camera_transform_fwd': (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _i, _i, _i, _c_f, _c_f]),
    'vpn_camera_transform_bwd': (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _i, _i, _i, _c_f, _c_f]),
    'vpn_mesh_fwd': (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _i, _i, _i, _c_f, _c_f]),
    'vpn_mesh_bwd': (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _i, _i, _i, _c_f, _c_f, _c_f]),
    'vpn_mesh_raster_workspace': (_sz, [_i, _i]),
    'vpn_mesh_raster_fwd': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _i, _f, _c_f, _c_f, _c_f]),
    'vpn_mesh_raster_bwd': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _i, _f, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'vpn_mesh_sample_fwd': (_i, [_c_f, _c_f, _c_f, _u64, _u64, _i, _i, _i, _i, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'vpn_mesh_sample_bwd': (_i, [_c_f, _c_f, _c_f, _c_f, _i, _i, _i, _i, _c_f, _c_f]),
    'vpn_head_pack_fwd': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _f, _f, _f, _f, _f, _c_f, _c_f]),
    'vpn_head_pack_bwd': (_i, [_c_f, _c_f, _c_f, _c_f, _i, _i, _i, _f, _f, _f, _f, _f, _c_f, _c_f, _c_f, _c_f]),
    'vpn_vpdiv_workspace': (_sz, [_i, _i]),
    'vpn_vpdiv_fwd': (_i, [_c_f, _c_f, _i, _i, _i, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'vpn_trainstep_workspace': (_sz, [_i]),
    'vpn_camera_matrix': (_i, [_c_f, _c_f, _c_f, _c_f, _i, _i, _c_f, _c_f]),
    'vpn_trainstep_finalize': (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f]),
    'vpn_trainstep_bwd': (_i, [_c_f, _c_f, _u64, _c_f, _u64, _i, _i, _i, _c_f, _c_f, _i, _c_f, _c_f, _c_f, _c_f, _f, _f, _c_f, _i, _i,
                               _c_f, _c_f, _c_f, _c_f, _c_f, _f, _c_f, _c_f, _c_f, _c_f, _f, _f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _c_f,
                               _f, _f, _i, _c_f, _c_f]),
    'vpn_emd_workspace': (_sz, [_i, _i]),
    'vpn_emd_fwd': (_i, [_c_f, _c_f, _i, _i, _f, _i, _c_f, _c_f, _c_f, _i, _c_f]),
    'vpn_emd_fwd_ex': (_i, [_c_f, _c_f, _i, _i, _f, _i, _c_f, _c_f, _c_f, _i, _c_f, ctypes.c_uint]),
    'vpn_emd_recovered_samples': (ctypes.c_longlong, []),
    'vpn_emd_last_group': (_i, []),
    'vpn_emd_bwd': (_i, [_c_f, _c_f, _c_f, _c_f, _i, _i, _c_f, _c_f]),
    'vpn_gcn_aggregate': (_i, [_c_f, _c_f, _c_f, _c_f, _c_f, _c_f, _i, _i, _i, _i, _c_f, _c_f]),
    'vpn_gcn_colsum_workspace': (_sz, [_i, _i, _i]),
    'vpn_gcn_colsum': (_i, [_c_f, _c_f, _i, _i, _i, _i, _i, _c_f, _c_f, _c_f]),
    'vpn_gcn_bounds': (_i, [_c_f, _i, _i, _i, _i, _c_f, _c_f]),
    'vpn_gcn_maps_workspace': (_sz, [_i, _i] + [_i] * 12),
    'vpn_gcn_input_fwd': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _i] + [_c_f] * 4 + [_i] * 12 + [_c_f] * 6),
    'vpn_gcn_input_bwd_workspace': (_sz, [_i, _i, _i] + [_i] * 12),
    'vpn_gcn_input_bwd': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _i] + [_i] * 12 + [_c_f] * 11),
    'vpn_cutmix_points_lds': (_sz, [_i]),
    'vpn_cutmix_points': (_i, [_c_f, _c_f, _c_f, _f, _u64, _u64, _i, _i, _i, _c_f, _c_f, _c_f, _c_f]),
    'vpn_cutmix_images': (_i, [_c_f, _c_f, _c_f, _i, _i, _i, _i, _i, _i, _c_f, _c_f, _c_f]),
    'vpn_mixup_gather': (_i, [_c_f, _c_f, _i, _i, _c_f, _c_f]),
    'vpn_mixup_lerp': (_i, [_c_f, _c_f, _c_f, _i, _i, _f, _f, _c_f, _c_f]),
    'vpn_eval_state_size': (_sz, [_i]),
    'vpn_eval_accumulate': (_i, [_c_f, _c_f, _c_f, _c_f, _i, _i, _i, _i, _f, _f, _f, _c_f, _c_f, _c_f, _c_f]),
    'vpn_vis_primitives': (_i, [_c_f, _c_f, _c_f, _c_f, _i, _i, _i, _i, _i, _f, _f, _f, _f, _c_f, _sz, ctypes.c_longlong, _c_f, _c_f]),
    'vpn_vis_mesh_workspace': (_sz, [_i, _i, _i]),
    'vpn_vis_mesh': (_i, [_c_f, _c_f, _c_f, _c_f, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _c_f, _c_f, _sz, ctypes.c_longlong, _c_f, _c_f]),
    'vpn_phong_mesh_workspace': (_sz, [_i, _i, _i]),
    'vpn_phong_mesh': (_i, [_c_f] * 7 + [_f] + [_i] * 8 + [_c_f, _c_f, _c_f]),
    'vpn_cluster_points': (_i, [_c_f, _i, _i, _i, _i, _c_f, _c_f, _c_f, _c_f]),
    'vpn_support_hulls': (_i, [_c_f, _c_f, _c_f, _c_f, _i, _i, _i, _i, _c_f, _c_f, _c_f]),
    'vpn_hull_augment': (_i, [_c_f] * 8 + [_i] * 4 + [_c_f, _c_f, _c_f]),
    'vpn_union_surface': (_i, [_c_f] * 5 + [_i] * 5 + [_f] + [_c_f] * 6),
    'vpn_input_ws': (_sz, [_i]),
    'vpn_prepare_images': (_i, [_c_f, _c_f, _i, _i, _i, _c_f, _c_f, _c_f, _u64, _c_f, _u64] + [_i] * 6 + [_c_f, _sz] + [_c_f] * 5),
    'vpn_ragged_sample_workspace': (_sz, [_i, _i, _i]),
    'vpn_ragged_sample': (_i, [_c_f] * 7 + [ctypes.c_uint, _c_f, _u64, _c_f, _u64] + [_i] * 6 + [_c_f, _sz] + [_c_f] * 4),
    'vpn_fc_stack_workspace': (_sz, [_i, _i, _i]),
    'vpn_fc_stack_fwd': (_i, [FcStack, _i, _f, _u64, _c_f, _i, _i, _i, _f, _f, _f, _f, _f, _c_f, _c_f]),
    'vpn_fc_stack_bwd': (_i, [FcStack, FcGrad, _i, _f, _u64, _c_f, _i, _i, _i, _f, _f, _f, _f, _f, _c_f, _sz, _c_f]),
}

_lib = None


def lib():
    """Load libvpn_hip.so once.  Raises if it has not been built (no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError('libvpn_hip.so is missing: build it with '
                               '`python volumetric-primitives-net_amd/build.py` (needs hipcc, gfx950)')
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)        # AttributeError if the .so does not export the symbol
            fn.restype, fn.argtypes = res, args
        if L.vpn_abi_version() != ABI_VERSION:
            raise RuntimeError('libvpn_hip.so ABI %d != binding ABI %d: rebuild' % (L.vpn_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


class KernelTimer:
    """Brackets every C-ABI call with a pair of HIP events on the stream the kernels are
    launched on (torch's current stream) so bench.py can report per-entry-point device time.
    Off by default; the timed throughput region of bench.py runs without it."""

    def __init__(self):
        self.records = []

    def __enter__(self):
        global _timer
        _timer = self
        return self

    def __exit__(self, *exc):
        global _timer
        _timer = None

    def summary(self):
        """name -> (calls, mean milliseconds).  Synchronises."""
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.records:
            n, t = out.get(name, (0, 0.0))
            out[name] = (n + 1, t + a.elapsed_time(b))
        return {k: (n, t / n) for k, (n, t) in out.items()}


_timer = None


class KernelProfile:
    """Per-KERNEL device times measured by the library itself (HIP events around every launch on the
    launch stream): `with KernelProfile() as kp: ...; kp.summary()` -> {kernel: (calls, mean ms)}."""

    def __enter__(self):
        lib().vpn_profile_enable(1)
        return self

    def __exit__(self, *exc):
        self._summary = self._read()
        lib().vpn_profile_enable(0)

    def _read(self):
        names = ctypes.create_string_buffer(8192)
        ms = (ctypes.c_float * 64)()
        calls = (ctypes.c_int * 64)()
        n = lib().vpn_profile_read(names, 8192, ms, calls, 64)
        if n < 0:
            check(n)
        keys = names.value.decode().split('\n')[:n]
        return {k: (calls[i], ms[i]) for i, k in enumerate(keys)}

    def summary(self):
        return getattr(self, '_summary', None) or self._read()


def call(name, *args):
    """Invoke entry point `name`, raise on a non-zero return code.  A tensor argument travels as its device pointer
    (ptr(): GPU only, contiguous); None, numbers and ctypes values (the stream, pointers the caller built) pass as they are."""
    fn = getattr(lib(), name)
    args = [ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    if _timer is None:
        check(fn(*args))
        return
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    rc = fn(*args)
    b.record()
    _timer.records.append((name, a, b))
    check(rc)


def check(rc):
    if rc != 0:
        raise RuntimeError('libvpn_hip: %s (code %d)' % (lib().vpn_error_string(rc).decode(), rc))


def ptr(t):
    """Device pointer of a contiguous CUDA(HIP) tensor, or NULL for None."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError('vpn_amd operators run on the GPU only (got a %s tensor); there is no CPU path'
                           % t.device.type)
    if not t.is_contiguous():
        raise RuntimeError('vpn_amd: tensor must be contiguous')
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
