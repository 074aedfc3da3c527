"""ctypes binding of libvpn_hip.so (C ABI declared in include/vpn_hip.h).

There is no CPU or PyTorch fallback: if the library is missing or a call fails the
binding raises.  PyTorch is used only for device memory and the current HIP stream."""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('VPN_HIP_LIB') or os.path.join(_HERE, 'libvpn_hip.so')     # VPN_HIP_LIB: the sanitizer build of the tests
HEADER_PATH = os.path.join(_HERE, '..', 'include', 'vpn_hip.h')


# ---- include/vpn_hip.h is the one place a limit, a flag or a signature of the C ABI is written: the binding reads it

def _header_code(text):
    """Header text without its comments."""
    return re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)


def _header_constants(text):
    """{name: value} of the integer `#define VPN_*` of header `text` (a negative one stands in parentheses)."""
    pattern = r'^[ \t]*#[ \t]*define[ \t]+(VPN_\w+)[ \t]+(?:(\d+)|\([ \t]*(-?\d+)[ \t]*\))[ \t]*$'
    return {m.group(1): int(m.group(2) or m.group(3)) for m in re.finditer(pattern, _header_code(text), flags=re.M)}


def _header_signatures(text, by_value):
    """{name: (restype, [argtypes])} of every `vpn_*` prototype of header `text`.  A pointer parameter travels as void*
    whatever it points to (device pointers, and ctypes arrays and buffers convert to it), a `const char*` result is a C
    string, every other type is looked up in `by_value`; one that is not there is an error, never a guess."""
    code = ';' + re.sub(r'^[ \t]*#.*$', '', _header_code(text), flags=re.M)

    def ctype(c_type, table, where):
        if c_type not in table:
            raise RuntimeError('vpn_hip.h: %s has type %r, which the binding cannot pass' % (where, c_type))
        return table[c_type]

    out = {}
    for m in re.finditer(r'(?<=[;{}])([\w\s*]+?)\b(vpn_\w+)\s*\(([^()]*)\)\s*;', code):
        res, name, params = ' '.join(m.group(1).replace('*', ' * ').split()), m.group(2), m.group(3).strip()
        args = []
        for param in ([] if params in ('', 'void') else params.split(',')):
            words = [w for w in param.split() if w != 'const']                      # the type, then the parameter's name
            args.append(ctypes.c_void_p if '*' in param else
                        ctype(' '.join(words[:-1]), by_value, '%s: parameter %r' % (name, ' '.join(param.split()))))
        out[name] = (ctype(res, dict(by_value, **{'const char *': ctypes.c_char_p}), name + ': the result'), args)
    return out


with open(HEADER_PATH) as _f:
    _HEADER = _f.read()
CONSTANTS = _header_constants(_HEADER)
ABI_VERSION = CONSTANTS['VPN_ABI_VERSION']
FC_MAX_LAYERS, FC_MAX_SLOTS = CONSTANTS['VPN_FC_MAX_LAYERS'], CONSTANTS['VPN_FC_MAX_SLOTS']
FC_NONE, FC_TANH, FC_VP_PACK = CONSTANTS['VPN_FC_NONE'], CONSTANTS['VPN_FC_TANH'], CONSTANTS['VPN_FC_VP_PACK']
FC_DROPOUT_OFF, FC_DROPOUT_MASK, FC_DROPOUT_PHILOX = (CONSTANTS['VPN_FC_DROPOUT_OFF'], CONSTANTS['VPN_FC_DROPOUT_MASK'],
                                                      CONSTANTS['VPN_FC_DROPOUT_PHILOX'])


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


# every type the header passes by value (parameters and results)
BY_VALUE = {'int': ctypes.c_int, 'unsigned': ctypes.c_uint, 'long long': ctypes.c_longlong, 'float': ctypes.c_float,
            'uint64_t': ctypes.c_uint64, 'size_t': ctypes.c_size_t, 'VpnFcStack': FcStack, 'VpnFcGrad': FcGrad}
SIGNATURES = _header_signatures(_HEADER, BY_VALUE)

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
