"""torch.autograd.Function wrappers over the C ABI (include/vpn_hip.h).

Pattern follows the reference's own native op, emdFunction (modules/loss/emd/
emd_module.py:29-70): forward allocates the outputs, calls native code, saves what
backward needs; backward returns one gradient per tensor input and None for the rest.
Unlike it, a non-zero return code raises."""
import collections
import ctypes
import math
import os
import weakref

import torch
from torch.autograd import Function

from . import _lib

_H = _lib.CONSTANTS            # the #define VPN_* of include/vpn_hip.h: limits and flags are written there only
SPHERE, CUBOID, PARAM_STRIDE = _H['VPN_SPHERE'], _H['VPN_CUBOID'], _H['VPN_PARAM_STRIDE']


def _f32c(t):
    if not t.is_cuda:
        raise RuntimeError('vpn_amd operators run on the GPU only (got a %s tensor); there is no CPU path'
                           % t.device.type)
    return t.contiguous().float()          # emd_module.py:41-42 does the same to its inputs


def _workspace(query, *dims, dev, dtype=torch.float32, floor=0):
    """Uninitialised buffer of the size in bytes that the library's `query`(*dims) reports, as `dtype` elements and at least
    `floor` of them (an empty tensor has a null pointer).  Like _nn_outputs, torch.empty alone: the hot path is captured
    into HIP graphs and stays free of host synchronisation and of ATen kernels."""
    nbytes = getattr(_lib.lib(), query)(*dims)
    return torch.empty((max(floor, nbytes // dtype.itemsize),), dtype=dtype, device=dev)


def _nn_outputs(B, N, M, dev):
    """(dist1 [B,N], idx1 [B,N] int32, dist2 [B,M], idx2 [B,M] int32): the outputs of a nearest-neighbour scan."""
    d1 = torch.empty((B, N), dtype=torch.float32, device=dev)
    d2 = torch.empty((B, M), dtype=torch.float32, device=dev)
    i1 = torch.empty((B, N), dtype=torch.int32, device=dev)
    i2 = torch.empty((B, M), dtype=torch.int32, device=dev)
    return d1, i1, d2, i2


# Host copies of device kind tensors: id(tensor) -> (weak reference to it, the version counter it had then, the kinds as a
# tuple).  The entry dies with its tensor (weakref callback) and a hit also requires the reference to be the same object, so
# a later tensor that reuses the id or the device address is never mistaken for a known one.  Kind tensors made from a
# host list are cached per (kinds, device): the list train.py:112-116 implies is the same every step, and the B composed
# meshes of a batch share ONE tensor -- equality checks and validation then never touch the device.
_KINDS_HOST = {}
_KINDS_BY_TUPLE = {}


def _check_kinds(kinds):
    if any(k not in (SPHERE, CUBOID) for k in kinds):
        raise ValueError('unknown primitive kind in %r (0 = sphere, 1 = cuboid; cones are not implemented '
                         'in the reference either)' % (kinds,))


def _kinds_remember(t, tup):
    key = id(t)
    _KINDS_HOST[key] = (weakref.ref(t, lambda _r, key=key: _KINDS_HOST.pop(key, None)), t._version, tup)


def kinds_host(t):
    """The kinds of a device kind tensor as a host tuple: from the registry, or -- the first time this (tensor, version) is
    seen -- through one device-to-host copy, which also validates them."""
    hit = _KINDS_HOST.get(id(t))
    if hit is not None and hit[0]() is t and hit[1] == t._version:
        return hit[2]
    tup = tuple(int(k) for k in t.detach().cpu().tolist())
    _check_kinds(tup)
    _kinds_remember(t, tup)
    return tup


def kinds_tensor(kinds, device):
    """int32 device tensor of primitive kinds; rejects cones (sampling.py:39-45 is `pass`).  A tensor already on the
    device is validated once per (tensor object, version) -- one host copy the first time -- so that an unknown kind never
    reaches a kernel; a host list maps to one cached tensor per (list, device)."""
    device = torch.device(device)
    if isinstance(kinds, torch.Tensor):
        if kinds.device.type == device.type and kinds.dtype == torch.int32 and kinds.is_contiguous():
            kinds_host(kinds)
            return kinds
        kinds = kinds.detach().cpu().tolist()
    tup = tuple(int(k) for k in kinds)
    _check_kinds(tup)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (tup, str(device))
    t = _KINDS_BY_TUPLE.get(key)
    if t is None:
        t = torch.tensor(tup, dtype=torch.int32, device=device)
        _KINDS_BY_TUPLE[key] = t
        _kinds_remember(t, tup)
    return t


def _seed_args(seed):
    """(host seed, device seed pointer) of the sampler entry points: `seed` is an int, or a device int64 tensor of
    one element (a step counter bumped on the stream: read by the kernel, so HIP-graph replays draw fresh points)."""
    if isinstance(seed, torch.Tensor):
        if not (seed.is_cuda and seed.dtype == torch.int64 and seed.numel() == 1):
            raise ValueError('a device seed must be a CUDA int64 tensor with one element')
        return 0, _lib.ptr(seed)
    return int(seed), None


class SampleFunction(Function):
    """Sampling.{sphere,cuboid}_sampling + transform_points + torch.cat over K primitives
    (sampling.py:11-37, train.py:105-120) -> points [B, K*n, 3]."""

    @staticmethod
    def forward(ctx, params, kinds, u, seed, sample_base, n):
        params = _f32c(params)
        B, K, S = params.shape
        kinds = kinds_tensor(kinds, params.device)
        assert S == PARAM_STRIDE and kinds.numel() == K
        if u is not None:
            u = _f32c(u)
            assert u.shape == (B, K, n, 3)
        points = torch.empty((B, K * n, 3), dtype=torch.float32, device=params.device)
        _lib.call('vpn_sample_fwd', params, kinds, u, int(seed), None, int(sample_base), B, K, n, points, _lib.stream())
        ctx.save_for_backward(params, kinds, u if u is not None else torch.empty(0, device=params.device))
        ctx.has_u = u is not None
        ctx.meta = (int(seed), int(sample_base), B, K, n)
        return points

    @staticmethod
    def backward(ctx, grad_points):
        params, kinds, u = ctx.saved_tensors
        seed, base, B, K, n = ctx.meta
        grad_points = _f32c(grad_points)
        grad_params = torch.empty_like(params)
        _lib.call('vpn_sample_bwd', params, kinds, u if ctx.has_u else None, seed, None, base, B, K, n, grad_points,
                  grad_params, _lib.stream())
        return grad_params, None, None, None, None, None


class TransformFunction(Function):
    """transform_points / rotate_points (transform.py:6-9, rotate.py:7-25): R(q) p (+ t)."""

    @staticmethod
    def forward(ctx, points, q, t):
        points, q = _f32c(points), _f32c(q)
        t = _f32c(t) if t is not None else None
        B, N, _ = points.shape
        out = torch.empty_like(points)
        _lib.call('vpn_transform_fwd', points, q, t, B, N, out, _lib.stream())
        ctx.save_for_backward(points, q)
        ctx.has_t = t is not None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        points, q = ctx.saved_tensors
        B, N, _ = points.shape
        grad_out = _f32c(grad_out)
        need_p, need_q, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_t and ctx.needs_input_grad[2]
        gp = torch.empty_like(points) if need_p else None
        gq = torch.empty_like(q) if need_q else None
        gt = torch.empty((B, 3), dtype=torch.float32, device=points.device) if need_t else None
        _lib.call('vpn_transform_bwd', points, q, grad_out, B, N, gp, gq, gt, _lib.stream())
        return gp, gq, gt


class MeshFunction(Function):
    """Vertices of all K primitives of all B samples in one launch (modules/meshing of the reference):
    params [B,K,10], templates [P,3] -> verts [B, sum_k P_kind(k), 3] in primitive order."""

    @staticmethod
    def forward(ctx, params, kinds, offsets, tpl_sphere, tpl_cuboid, ptot):
        params = _f32c(params)
        B, K, _ = params.shape
        kinds = kinds_tensor(kinds, params.device)
        ts = _f32c(tpl_sphere) if tpl_sphere is not None else None
        tc = _f32c(tpl_cuboid) if tpl_cuboid is not None else None
        verts = torch.empty((B, int(ptot), 3), dtype=torch.float32, device=params.device)
        _lib.call('vpn_mesh_fwd', params, kinds, offsets, ts, tc, B, K, int(ptot), verts, _lib.stream())
        ctx.save_for_backward(params, kinds, offsets, *(x for x in (ts, tc) if x is not None))
        ctx.which = (ts is not None, tc is not None, int(ptot))
        return verts

    @staticmethod
    def backward(ctx, grad_verts):
        params, kinds, offsets, *tpls = ctx.saved_tensors
        has_s, has_c, ptot = ctx.which
        ts = tpls[0] if has_s else None
        tc = tpls[-1] if has_c else None
        B, K, _ = params.shape
        g = _f32c(grad_verts)
        gp = torch.empty_like(params)
        _lib.call('vpn_mesh_bwd', params, kinds, offsets, ts, tc, B, K, ptot, g, gp, _lib.stream())
        return gp, None, None, None, None, None


_FACES = {}
_FACES_FP = {}


def faces_fingerprint(faces):
    """Content key of a face tensor: (shape, hash of its bytes), computed once per (tensor object, version).  Free for a
    host tensor; one device-to-host copy for a device tensor that is seen for the first time (TriangleMesh.to carries the
    key of the host tensor over, so meshes loaded from OBJ files never pay it)."""
    hit = _FACES_FP.get(id(faces))
    if hit is not None and hit[0]() is faces and hit[1] == faces._version:
        return hit[2]
    host = faces.detach().cpu().contiguous()
    fp = (tuple(host.shape), str(host.dtype), hash(host.numpy().tobytes()))
    faces_remember(faces, fp)
    return fp


def faces_fingerprint_known(faces):
    """The content key of a face tensor if it is already known (remembered for this object and version), else None;
    never reads the device."""
    hit = _FACES_FP.get(id(faces))
    if hit is not None and hit[0]() is faces and hit[1] == faces._version:
        return hit[2]
    return None


def faces_remember(faces, fp):
    key = id(faces)
    _FACES_FP[key] = (weakref.ref(faces, lambda _r, key=key: _FACES_FP.pop(key, None)), faces._version, fp)


def faces_i32(faces, device):
    """[F,3] int32 contiguous device copy of a face tensor (the reference's are int64: meshing.py:38-39), one per CONTENT
    and device: keyed by the fingerprint, never by an address the allocator may hand to another tensor."""
    if faces.dtype == torch.int32 and faces.is_cuda and faces.is_contiguous():
        return faces
    key = (faces_fingerprint(faces), str(torch.device(device)))
    hit = _FACES.get(key)
    if hit is None:
        if len(_FACES) > 256:
            _FACES.clear()
        hit = faces.detach().to(device=device, dtype=torch.int32).contiguous()
        _FACES[key] = hit
    return hit


class MeshRasterFunction(Function):
    """Soft silhouette of triangle meshes WITHOUT primitives (the mesh input of vertex_renderer.py:20-24 as
    train_sphere.py:128 passes it): verts [B,P,3], faces [F,3] int32, cam [B,3] -> alpha [B,H,W]."""

    @staticmethod
    def forward(ctx, verts, faces, cam, H, W, sigma):
        verts, cam = _f32c(verts), _f32c(cam)
        B, P, _ = verts.shape
        F = faces.shape[0]
        assert faces.dtype == torch.int32 and faces.is_cuda and faces.is_contiguous() and cam.shape == (B, 3)
        dev = verts.device
        ws = _workspace('vpn_mesh_raster_workspace', B, P, dev=dev)
        alpha = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        _lib.call('vpn_mesh_raster_fwd', verts, faces, cam, B, P, F, H, W, float(sigma), ws, alpha, _lib.stream())
        ctx.save_for_backward(verts, faces, cam, ws, alpha)
        ctx.meta = (B, P, F, H, W, float(sigma))
        return alpha

    @staticmethod
    def backward(ctx, grad_alpha):
        verts, faces, cam, ws, alpha = ctx.saved_tensors
        B, P, F, H, W, sigma = ctx.meta
        g = _f32c(grad_alpha)
        gv = torch.empty_like(verts)
        _lib.call('vpn_mesh_raster_bwd', verts, faces, cam, B, P, F, H, W, sigma, ws, alpha, g, gv, _lib.stream())
        return gv, None, None, None, None, None


class MeshSampleFunction(Function):
    """kaolin's TriangleMesh.sample as train_sphere.py:76 uses it: n area-weighted uniform surface points per mesh.
    verts [B,P,3], faces [F,3] int32 -> points [B,n,3] (differentiable w.r.t. verts), face index [B,n] int32."""

    @staticmethod
    def forward(ctx, verts, faces, n, u, seed, mesh_base):
        verts = _f32c(verts)
        B, P, _ = verts.shape
        F = faces.shape[0]
        assert faces.dtype == torch.int32 and faces.is_cuda and faces.is_contiguous()
        dev = verts.device
        if u is not None:
            u = _f32c(u)
            assert u.shape == (B, n, 3)
        cdf = torch.empty((B, F), dtype=torch.float32, device=dev)
        points = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
        fidx = torch.empty((B, n), dtype=torch.int32, device=dev)
        bary = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
        _lib.call('vpn_mesh_sample_fwd', verts, faces, u, int(seed), int(mesh_base), B, P, F, int(n), cdf, points, fidx, bary,
                  _lib.stream())
        ctx.save_for_backward(faces, fidx, bary)
        ctx.meta = (B, P, F, int(n))
        ctx.mark_non_differentiable(fidx)
        return points, fidx

    @staticmethod
    def backward(ctx, grad_points, _grad_idx):
        faces, fidx, bary = ctx.saved_tensors
        B, P, F, n = ctx.meta
        g = _f32c(grad_points)
        gv = torch.empty((B, P, 3), dtype=torch.float32, device=g.device)
        _lib.call('vpn_mesh_sample_bwd', faces, fidx, bary, g, B, P, F, n, gv, _lib.stream())
        return gv, None, None, None, None, None


class HeadPackFunction(Function):
    """restrict_range + split + restrict_volumes of the reference's model (vpnet_one_resnet.py:34-41, :67-85) fused:
    raw head outputs volumes [B,3K], rotates [B,4K], translates [B,3K] -> packed params [B,K,10]."""

    @staticmethod
    def forward(ctx, volumes, rotates, translates, is_sigmoid, clamp_min, clamp_max, restrict):
        volumes, rotates, translates = _f32c(volumes), _f32c(rotates), _f32c(translates)
        B = volumes.shape[0]
        assert volumes.shape[1] % 3 == 0
        K = volumes.shape[1] // 3
        assert rotates.shape == (B, 4 * K) and translates.shape == (B, 3 * K)
        r = [float(x) for x in restrict]
        assert len(r) == 3
        params = torch.empty((B, K, PARAM_STRIDE), dtype=torch.float32, device=volumes.device)
        _lib.call('vpn_head_pack_fwd', volumes, rotates, translates, B, K, int(bool(is_sigmoid)), float(clamp_min),
                  float(clamp_max), r[0], r[1], r[2], params, _lib.stream())
        ctx.save_for_backward(volumes, rotates, translates)
        ctx.cfg = (B, K, int(bool(is_sigmoid)), float(clamp_min), float(clamp_max), r)
        return params

    @staticmethod
    def backward(ctx, grad_params):
        volumes, rotates, translates = ctx.saved_tensors
        B, K, sig, cmin, cmax, r = ctx.cfg
        g = _f32c(grad_params)
        gv = torch.empty_like(volumes) if ctx.needs_input_grad[0] else None
        gq = torch.empty_like(rotates) if ctx.needs_input_grad[1] else None
        gt = torch.empty_like(translates) if ctx.needs_input_grad[2] else None
        _lib.call('vpn_head_pack_bwd', volumes, rotates, translates, g, B, K, sig, cmin, cmax, r[0], r[1], r[2], gv, gq, gt,
                  _lib.stream())
        return gv, gq, gt, None, None, None, None


class FcStackFunction(Function):
    """G groups of L nn.Linear layers each, forward and backward on csrc/fcstack.hip: the FC heads of the reference's
    networks (vpnet_one_resnet.py:31-41, :87-107; vpnet_two_resnet.py:34-44; sdnet.py:19, :24-25, :41-50), one launch per
    layer for all groups.  apply(cfg, *tensors), tensors = the G inputs (B,in_g) -- one tensor may be passed for several
    groups, autograd adds its gradients --, then weight, bias of every layer (group-major, layer-minor, nn.Linear's
    layout), then, under cfg['dropout'] == 'mask', the uint8 keep masks (B,out) of layers 0..L-2 of every group.
    cfg: G, L, epilogue 'none' | 'tanh' | 'vp_pack', dropout None | 'mask' | 'philox', p, seed (an int, or a CUDA int64
    tensor of one element read by the kernels: bump it between steps, never between a forward and its backward), and for 'vp_pack'
    is_sigmoid, clamp_min, clamp_max, volume_restrict.  Returns the G raw outputs ('none'), tanh of the one output
    (B,out) ('tanh'), or the packed parameters (B,K,10) ('vp_pack')."""

    EPILOGUES = {'none': _lib.FC_NONE, 'tanh': _lib.FC_TANH, 'vp_pack': _lib.FC_VP_PACK}
    DROPOUTS = {None: _lib.FC_DROPOUT_OFF, 'mask': _lib.FC_DROPOUT_MASK, 'philox': _lib.FC_DROPOUT_PHILOX}

    @staticmethod
    def forward(ctx, cfg, *tensors):
        G, L = int(cfg['G']), int(cfg['L'])
        epi, drop = FcStackFunction.EPILOGUES[cfg.get('epilogue', 'none')], FcStackFunction.DROPOUTS[cfg.get('dropout')]
        if not (1 <= L <= _lib.FC_MAX_LAYERS and 1 <= G and G * L <= _lib.FC_MAX_SLOTS):
            raise ValueError('FcStackFunction: 1 <= L <= %d and G * L <= %d' % (_lib.FC_MAX_LAYERS, _lib.FC_MAX_SLOTS))
        n_masks = G * (L - 1) if drop == _lib.FC_DROPOUT_MASK else 0
        assert len(tensors) == G + 2 * G * L + n_masks, 'FcStackFunction: G inputs, G L (weight, bias) pairs, then the masks'
        xs = [_f32c(t) for t in tensors[:G]]
        wb = [_f32c(t) for t in tensors[G:G + 2 * G * L]]
        masks = list(tensors[G + 2 * G * L:])
        dev, B = xs[0].device, xs[0].shape[0]
        st = _lib.FcStack()
        st.G, st.L, st.B = G, L, B
        acts, hold = [], []
        for g in range(G):
            assert xs[g].dim() == 2 and xs[g].shape[0] == B
            st.in0[g], st.x[g] = xs[g].shape[1], xs[g].data_ptr()
            width = xs[g].shape[1]
            for l in range(L):
                i = g * L + l
                w, b = wb[2 * i], wb[2 * i + 1]
                assert w.dim() == 2 and w.shape[1] == width and b.shape == (w.shape[0],), 'layer %d of group %d: shapes' % (l, g)
                width = w.shape[0]
                st.out[i], st.w[i], st.bias[i] = width, w.data_ptr(), b.data_ptr()
                acts.append(torch.empty((B, width), dtype=torch.float32, device=dev))
                st.act[i] = acts[-1].data_ptr()
                if n_masks and l < L - 1:
                    m = masks[g * (L - 1) + l]
                    if not m.is_cuda:
                        raise RuntimeError('vpn_amd operators run on the GPU only (got a %s tensor); there is no CPU path' % m.device.type)
                    assert m.dtype == torch.uint8 and m.shape == (B, width) and m.is_contiguous()
                    st.keep[i] = m.data_ptr()
                    hold.append(m)
        K, final = 0, None
        if epi == _lib.FC_TANH:
            assert G == 1
            final = torch.empty((B, st.out[L - 1]), dtype=torch.float32, device=dev)
        elif epi == _lib.FC_VP_PACK:
            assert G == 3 and st.out[L - 1] % 3 == 0
            K = st.out[L - 1] // 3
            assert st.out[2 * L - 1] == 4 * K and st.out[3 * L - 1] == 3 * K, 'vp_pack: the heads end in 3K | 4K | 3K'
            final = torch.empty((B, K, PARAM_STRIDE), dtype=torch.float32, device=dev)
        r = [float(v) for v in cfg.get('volume_restrict', (1.0, 1.0, 1.0))]
        seed_host, seed_dev = _seed_args(cfg.get('seed', 0))     # an int, or a device int64 step counter
        tail = (drop, float(cfg.get('p', 0.5)), seed_host & 0xFFFFFFFFFFFFFFFF, seed_dev, epi, K,
                int(bool(cfg.get('is_sigmoid', True))), float(cfg.get('clamp_min', 0.0)), float(cfg.get('clamp_max', 1.0)),
                r[0], r[1], r[2])
        _lib.call('vpn_fc_stack_fwd', st, *tail, final, _lib.stream())
        ctx.save_for_backward(*xs, *wb, *acts, *hold)
        ctx.meta = (G, L, B, n_masks, tail, max([st.in0[g] for g in range(G)] + [st.out[i] for i in range(G * L)]))
        ctx.n_inputs = len(tensors)
        if epi == _lib.FC_NONE:
            outs = tuple(acts[g * L + L - 1] for g in range(G))
            return outs if G > 1 else outs[0]
        return final

    @staticmethod
    def backward(ctx, *grads):
        G, L, B, n_masks, tail, maxw = ctx.meta
        saved = ctx.saved_tensors
        xs, wb = saved[:G], saved[G:G + 2 * G * L]
        acts, hold = saved[G + 2 * G * L:G + 3 * G * L], saved[G + 3 * G * L:]
        dev = xs[0].device
        st, gr = _lib.FcStack(), _lib.FcGrad()
        st.G, st.L, st.B = G, L, B
        need = ctx.needs_input_grad[1:]
        out = [None] * ctx.n_inputs
        gouts = []
        for g in range(G if tail[4] == _lib.FC_NONE else 1):
            go = grads[g]
            gouts.append(_f32c(go) if go is not None else torch.zeros_like(acts[g * L + L - 1]))
            gr.gout[g] = gouts[-1].data_ptr()
        for g in range(G):
            st.in0[g], st.x[g] = xs[g].shape[1], xs[g].data_ptr()
            if need[g]:
                out[g] = torch.empty_like(xs[g])
                gr.dx[g] = out[g].data_ptr()
            for l in range(L):
                i = g * L + l
                st.out[i], st.w[i], st.bias[i], st.act[i] = wb[2 * i].shape[0], wb[2 * i].data_ptr(), wb[2 * i + 1].data_ptr(), acts[i].data_ptr()
                if n_masks and l < L - 1:
                    st.keep[i] = hold[g * (L - 1) + l].data_ptr()
                if need[G + 2 * i]:
                    out[G + 2 * i] = torch.empty_like(wb[2 * i])
                    gr.dw[i] = out[G + 2 * i].data_ptr()
                if need[G + 2 * i + 1]:
                    out[G + 2 * i + 1] = torch.empty_like(wb[2 * i + 1])
                    gr.db[i] = out[G + 2 * i + 1].data_ptr()
        ws = _workspace('vpn_fc_stack_workspace', G, B, maxw, dev=dev, floor=4)
        _lib.call('vpn_fc_stack_bwd', st, gr, *tail, ws, ws.numel() * 4, _lib.stream())
        return (None, *out)


class CameraTransformFunction(Function):
    """view_to_obj_points / obj_to_view_points (modules/transform/transform.py:21-73) in one launch.
    dists, elevs, azims, angles are dataset values (dataset.py:145-165): constants for autograd."""

    @staticmethod
    def forward(ctx, points, dists, elevs, azims, angles, to_object):
        points = _f32c(points)
        B, N, _ = points.shape
        cam = [_f32c(c.reshape(-1)) for c in (dists, elevs, azims)]
        ang = _f32c(angles.reshape(-1)) if angles is not None else None
        for c in cam + ([ang] if ang is not None else []):
            if c.numel() != B:
                raise ValueError('camera arguments must hold one value per sample')
        out = torch.empty_like(points)
        _lib.call('vpn_camera_transform_fwd', points, cam[0], cam[1], cam[2], ang, B, N, int(bool(to_object)), out,
                  _lib.stream())
        ctx.save_for_backward(*cam, *([ang] if ang is not None else []))
        ctx.to_object = int(bool(to_object))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        d, e, a = saved[:3]
        ang = saved[3] if len(saved) > 3 else None
        g = _f32c(grad_out)
        B, N, _ = g.shape
        gp = torch.empty_like(g)
        _lib.call('vpn_camera_transform_bwd', g, d, e, a, ang, B, N, ctx.to_object, gp, _lib.stream())
        return gp, None, None, None, None, None


class ChamferFunction(Function):
    """ChamferDistanceLoss.forward up to the per-sample loss (chamfer_distance.py:14-28).
    Returns loss_b [B]; the caller takes .mean() unless each_batch (chamfer_distance.py:30)."""

    @staticmethod
    def forward(ctx, p1, p2, w1, w2):
        p1, p2 = _f32c(p1), _f32c(p2)
        B, N, _ = p1.shape
        M = p2.shape[1]
        dev = p1.device
        d1, i1, d2, i2 = _nn_outputs(B, N, M, dev)
        loss_b = torch.empty((B,), dtype=torch.float32, device=dev)
        s = _lib.stream()
        ws = _workspace('vpn_chamfer_workspace', B, N, M, dev=dev)
        _lib.call('vpn_chamfer_fwd_ws', p1, p2, B, N, M, d1, i1, d2, i2, ws, ws.numel() * 4, 0, s)
        _lib.call('vpn_chamfer_loss', d1, d2, B, N, M, float(w1), float(w2), loss_b, s)
        ctx.save_for_backward(p1, p2, d1, i1, d2, i2)
        ctx.w = (float(w1), float(w2))
        return loss_b

    @staticmethod
    def backward(ctx, grad_loss_b):
        p1, p2, d1, i1, d2, i2 = ctx.saved_tensors
        B, N, _ = p1.shape
        M = p2.shape[1]
        g = _f32c(grad_loss_b)
        g1 = torch.empty_like(p1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(p2) if ctx.needs_input_grad[1] else None
        _lib.call('vpn_chamfer_bwd', p1, p2, d1, i1, d2, i2, g, B, N, M, ctx.w[0], ctx.w[1], g1, g2, _lib.stream())
        return g1, g2, None, None


CHAMFER_MODES = {'auto': 0, 'brute': 1, 'pruned': 2, 'mfma': 3, 'mfma32': 4, 'sorted': 5, 'mfma16': 6}


def chamfer_nn(p1, p2, mode='auto'):
    """Nearest-neighbour distances and indices in both directions (no autograd):
    (dist1 [B,N], idx1 [B,N] int32, dist2 [B,M], idx2 [B,M] int32).  mode, one of CHAMFER_MODES (same results bit for
    bit; the numbered modes of vpn_chamfer_fwd_ws in include/vpn_hip.h):
        'auto'    'mfma16' for large clouds, else 'brute'
        'brute'   brute force
        'pruned'  box-pruned: the clouds Morton-sorted per call, target chunks farther than the current best skipped
        'mfma'    matrix-pipe filter on bf16 MFMA (coordinates split exactly into three bf16 pieces), finished exactly
        'mfma32'  the same filter on fp32-input MFMA
        'sorted'  'mfma' over Morton-sorted clouds with per-block boxes: target blocks that cannot hold a nearer point skipped
        'mfma16'  the filter with one fp16 MFMA per 32x32 block (coordinates scaled and split into two fp16 pieces)"""
    p1, p2 = _f32c(p1.detach()), _f32c(p2.detach())
    B, N, _ = p1.shape
    M = p2.shape[1]
    dev = p1.device
    d1, i1, d2, i2 = _nn_outputs(B, N, M, dev)
    ws = _workspace('vpn_chamfer_workspace', B, N, M, dev=dev)
    _lib.call('vpn_chamfer_fwd_ws', p1, p2, B, N, M, d1, i1, d2, i2, ws, ws.numel() * 4, CHAMFER_MODES[mode], _lib.stream())
    return d1, i1, d2, i2


# Test hook of the auction (vpn_emd_fwd_ex): bit b set = sample b < 32 of every EMD call in this process gives up at its
# first group barrier whenever the call runs with G > 1, so the G = 1 recovery launch redoes it.  0 in normal use.
EMD_TEST_GIVEUP_MASK = 0


def _emd_group(max_group):
    """The auction's cap on the workgroups per sample (see EmdFunction.forward): `max_group`, or for None 1 under
    VPN_CONCURRENT=1 and else what the environment asks for (0, the default: automatic)."""
    if max_group is None:
        return 1 if CONCURRENT_BRANCHES else int(os.environ.get('VPN_EMD_GROUP', '0'))
    return int(max_group)


def emd_recovered_samples():
    """Samples the auction's G = 1 recovery launches have recomputed on the current device since the library was loaded
    (workgroups of a sample that could not all be resident together: another process or stream held the CUs).  Waits
    for the device: call it between steps."""
    v = _lib.lib().vpn_emd_recovered_samples()
    if v < 0:
        _lib.check(int(-v))
    return int(v)


def emd_last_group():
    """Workgroups per sample (G) of the last auction launch in this process (0: none yet)."""
    return int(_lib.lib().vpn_emd_last_group())


def _auction(xyz1, xyz2, eps, iters, group, stream):
    """The auction launch (vpn_emd_fwd_ex) of contiguous fp32 clouds [B,n,3] on `stream` (a hipStream_t as ctypes gives it)
    with at most `group` workgroups per sample (see _emd_group) -> (dist [B,n], assignment [B,n] int32, the workspace).
    When `stream` is not the current stream the caller keeps all three alive until it has joined that stream: the
    allocator hands a freed block to the next torch.empty on the current stream, while the auction may still be running."""
    B, n, _ = xyz1.shape
    dev = xyz1.device
    dist = torch.empty((B, n), dtype=torch.float32, device=dev)
    assignment = torch.empty((B, n), dtype=torch.int32, device=dev)
    ws = _workspace('vpn_emd_workspace', B, n, dev=dev, floor=1)
    _lib.call('vpn_emd_fwd_ex', xyz1, xyz2, B, n, float(eps), int(iters), dist, assignment, ws, group, stream,
              EMD_TEST_GIVEUP_MASK)
    return dist, assignment, ws


class EmdFunction(Function):
    """emdFunction (modules/loss/emd/emd_module.py:29-70) on vpn_emd_fwd / vpn_emd_bwd: auction
    approximation of the Earth Mover's Distance.  Returns (dist [B,n] squared distance to the assigned
    point, assignment [B,n] int32).  The reference's nine scratch tensors are one workspace here."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, eps, iters, max_group=None):
        """max_group: cap on the workgroups per sample (None: _emd_group's default; 1: no inter-workgroup barrier --
        what VPN_CONCURRENT=1 picks, since there other streams of this process share the GPU by design).  The library
        bounds the group by the occupancy query of an idle GPU and launches plainly (VPN_EMD_COOP_LAUNCH=1: a cooperative
        launch, which falls back to one workgroup per sample if the runtime refuses the grid).  When another process or
        stream keeps some of a sample's workgroups from being resident, their bounded wait gives up and the launch at
        G = 1 that follows every G > 1 launch recomputes the sample (emd_recovered_samples() counts them): sharing the
        GPU costs time, not correctness.  The kernel follows from n (VPN_EMD_FORM=team|local|streaming overrides it).
        The result is the same bits in every case."""
        B, n, _ = xyz1.size()
        assert n == xyz2.size(1)                       # emd_module.py:36-37
        assert B == xyz2.size(0)
        xyz1, xyz2 = _f32c(xyz1), _f32c(xyz2)
        dist, assignment, _ = _auction(xyz1, xyz2, eps, iters, _emd_group(max_group), _lib.stream())
        ctx.save_for_backward(xyz1, xyz2, assignment)
        ctx.mark_non_differentiable(assignment)
        return dist, assignment

    @staticmethod
    def backward(ctx, graddist, gradidx):
        xyz1, xyz2, assignment = ctx.saved_tensors
        B, n, _ = xyz1.shape
        g = _f32c(graddist)
        g1 = torch.empty_like(xyz1)
        _lib.call('vpn_emd_bwd', xyz1, xyz2, g, assignment, B, n, g1, _lib.stream())
        g2 = torch.zeros_like(xyz2) if ctx.needs_input_grad[1] else None     # emd_module.py:67
        return g1, g2, None, None, None


class RasterFunction(Function):
    """Primitive soft raster behind VertexRenderer.render (vertex_renderer.py:14-26):
    params [B,K,10], cam [B,3] = (dist, elev_deg, azim_deg) -> alpha, depth [B,H,W]."""

    @staticmethod
    def forward(ctx, params, kinds, cam, H, W, sigma, gamma, z_far):
        params, cam = _f32c(params), _f32c(cam)
        B, K, S = params.shape
        kinds = kinds_tensor(kinds, params.device)
        assert S == PARAM_STRIDE and kinds.numel() == K and cam.shape == (B, 3)
        dev = params.device
        alpha = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        depth = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        aux = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        rec = _workspace('vpn_raster_records_size', B, K, H, W, dev=dev)
        _lib.call('vpn_raster_fwd', params, kinds, cam, B, K, H, W, float(sigma), float(gamma), float(z_far), alpha, depth, aux,
                  rec, _lib.stream())
        ctx.save_for_backward(params, kinds, cam, aux, rec)
        ctx.meta = (B, K, H, W, float(sigma), float(gamma), float(z_far))
        return alpha, depth

    @staticmethod
    def backward(ctx, grad_alpha, grad_depth):
        params, kinds, cam, aux, rec = ctx.saved_tensors
        B, K, H, W, sigma, gamma, z_far = ctx.meta
        ga = _f32c(grad_alpha) if grad_alpha is not None else None
        gd = _f32c(grad_depth) if grad_depth is not None else None
        ws = _workspace('vpn_raster_bwd_workspace', B, K, H, W, dev=params.device)
        grad_params = torch.empty_like(params)
        _lib.call('vpn_raster_bwd', params, kinds, cam, B, K, H, W, sigma, gamma, z_far, aux, rec, ga, gd, ws, grad_params,
                  _lib.stream())
        return grad_params, None, None, None, None, None, None, None


class RasterLossFunction(Function):
    """SilhouetteLoss.forward (silhouette.py:13-23) fused into the raster: render + L1/MSE mean against
    the GT silhouette (+ optional L1 depth loss) without materialising the images.
    Returns a [2] tensor: (silhouette loss, depth loss)."""

    @staticmethod
    def forward(ctx, params, kinds, cam, gt_sil, gt_depth, H, W, sigma, gamma, z_far, sil_mse):
        params, cam = _f32c(params), _f32c(cam)
        B, K, S = params.shape
        kinds = kinds_tensor(kinds, params.device)
        assert S == PARAM_STRIDE and kinds.numel() == K and cam.shape == (B, 3)
        if gt_sil is not None:
            gt_sil = _f32c(gt_sil).reshape(B, H, W)
        if gt_depth is not None:
            gt_depth = _f32c(gt_depth).reshape(B, H, W)
        dev = params.device
        aux = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        rec = _workspace('vpn_raster_records_size', B, K, H, W, dev=dev)
        lws = _workspace('vpn_raster_loss_workspace', B, H, W, dev=dev)
        losses = torch.empty((4,), dtype=torch.float32, device=dev)
        _lib.call('vpn_raster_loss_fwd', params, kinds, cam, B, K, H, W, float(sigma), float(gamma), float(z_far), gt_sil,
                  gt_depth, int(bool(sil_mse)), aux, rec, lws, losses, _lib.stream())
        losses = losses[:2]
        empty = torch.empty(0, device=dev)
        ctx.save_for_backward(params, kinds, cam, aux, rec, gt_sil if gt_sil is not None else empty,
                              gt_depth if gt_depth is not None else empty)
        ctx.meta = (B, K, H, W, float(sigma), float(gamma), float(z_far), int(bool(sil_mse)),
                    gt_sil is not None, gt_depth is not None)
        return losses

    @staticmethod
    def backward(ctx, grad_losses):
        params, kinds, cam, aux, rec, gt_sil, gt_depth = ctx.saved_tensors
        B, K, H, W, sigma, gamma, z_far, sil_mse, has_sil, has_depth = ctx.meta
        g = _f32c(grad_losses)
        ws = _workspace('vpn_raster_bwd_workspace', B, K, H, W, dev=params.device)
        grad_params = torch.empty_like(params)
        _lib.call('vpn_raster_loss_bwd', params, kinds, cam, B, K, H, W, sigma, gamma, z_far, aux, rec,
                  gt_sil if has_sil else None, gt_depth if has_depth else None, sil_mse, g, ws, grad_params, 0, _lib.stream())
        return (grad_params,) + (None,) * 10


class RasterTotalFunction(Function):
    """total_img = w_sil * SilhouetteLoss + w_dep * L1(depth), forward and backward in one pass over the image
    (vpn_raster_total_fwd: no aux tensor, GT read once, the gradient partials are produced by the forward launch;
    backward is the small finishing kernel).  Returns (silhouette loss, depth loss, total_img); only the total is
    differentiable."""

    @staticmethod
    def forward(ctx, params, kinds, cam, gt_sil, gt_depth, H, W, sigma, gamma, z_far, sil_mse, w_sil, w_dep):
        params, cam = _f32c(params), _f32c(cam)
        B, K, S = params.shape
        kinds = kinds_tensor(kinds, params.device)
        assert S == PARAM_STRIDE and kinds.numel() == K and cam.shape == (B, 3)
        gt_sil = _f32c(gt_sil).reshape(B, H, W) if gt_sil is not None else None
        gt_depth = _f32c(gt_depth).reshape(B, H, W) if gt_depth is not None else None
        dev = params.device
        s = _lib.stream()
        rec = _workspace('vpn_raster_records_size', B, K, H, W, dev=dev)
        lws = _workspace('vpn_raster_loss_workspace', B, H, W, dev=dev)
        ws = _workspace('vpn_raster_bwd_workspace', B, K, H, W, dev=dev)
        losses = torch.empty((4,), dtype=torch.float32, device=dev)
        # render, image losses, gradient partials and the loss finalisation: one launch after the record launch
        _lib.call('vpn_raster_total_fwd_fin', params, kinds, cam, B, K, H, W, float(sigma), float(gamma), float(z_far), gt_sil,
                  gt_depth, int(bool(sil_mse)), float(w_sil), float(w_dep), rec, lws, ws, 0, None, 0, 0, 0, 0.0, 0.0, 0.0,
                  losses, None, None, None, s)
        ctx.save_for_backward(params, cam, rec, ws)
        ctx.meta = (B, K, H, W)
        sil, dep, tot, _ = losses.unbind(0)
        ctx.mark_non_differentiable(sil, dep)
        ctx.set_materialize_grads(False)       # no zero-filled gradients for the two reported values
        return sil, dep, tot

    @staticmethod
    def backward(ctx, _g_sil, _g_dep, grad_total):
        params, cam, rec, ws = ctx.saved_tensors
        B, K, H, W = ctx.meta
        if grad_total is None:
            return (None,) * 13
        g = _f32c(grad_total).reshape(1)
        grad_params = torch.empty_like(params)
        _lib.call('vpn_raster_total_bwd', params, cam, B, K, H, W, rec, ws, g, grad_params, 0, _lib.stream())
        return (grad_params,) + (None,) * 12


TILE_ORDER = os.environ.get('VPN_TILE_ORDER', '1') != '0'     # 0: position-based launch order of the tile waves (A/B switch)
_PATTERNS = {}
_RIDER_FITS = {}
FUSED_BWD_MAX_GT = _H['VPN_FUSED_BWD_MAX_GT']      # vpn_sample_chamfer_bwd keeps per-wave match lists of the GT points in LDS
_SIDE = {}
# optionally run the raster branch of HotPathLossFunction on a second HIP stream (VPN_CONCURRENT=1)
# TrainStepLossFunction: the auction on a second stream, beside the scans and the raster (measured at C5: 1.10 -> 0.94 ms per
# step; VPN_EMD_SIDE=0 puts it back in line)
EMD_SIDE_STREAM = os.environ.get('VPN_EMD_SIDE', '1') == '1'
CONCURRENT_BRANCHES = os.environ.get('VPN_CONCURRENT', '0') == '1'   # measured: no gain at C3 (each kernel already fills the GPU)


def _side_stream(dev):
    key = str(dev)
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=dev)
    return _SIDE[key]


def _fork_side(dev):
    """The side stream of `dev`, made to wait for everything enqueued on the current stream so far (the fork; the caller
    joins with current_stream().wait_stream(side)).  Both are captured into HIP graphs as such."""
    side = _side_stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    return side


def _grad_pattern(B, w_cd, dev):
    """d total / d loss_b[0..B): constant per configuration, cached on the device (created outside any graph capture
    by the first eager call)."""
    key = (B, float(w_cd), str(dev))
    if key not in _PATTERNS:
        _PATTERNS[key] = torch.full((B,), w_cd / B, dtype=torch.float32, device=dev)
    return _PATTERNS[key]


def _tile_rider_fits(K, H, W):
    """Whether the Chamfer scan's launch can carry the rider that tests the raster's 16 x 16 pixel tiles (R_TW, R_TH) against
    the K primitives and sorts them by weight: the library's own answer (vpn_hotpath_chamfer_fwd returns VPN_E_TOOBIG where
    this is False), asked once per shape.  TILE_ORDER = False (VPN_TILE_ORDER=0) turns the rider off."""
    if (K, H, W) not in _RIDER_FITS:
        _RIDER_FITS[K, H, W] = _lib.lib().vpn_hotpath_tile_rider_fits(K, H, W) == 1
    return TILE_ORDER and _RIDER_FITS[K, H, W]


def _hotpath_sample(params, kinds, cam, gt_points, n, seed_host, seed_dev, sample_base, Hr, Wr, sigma, features, s):
    """First launch of the one-stream hot path: the sampler, which also writes the raster records of the same primitives for
    an Hr x Wr image and, when `features`, the features of both clouds that the Chamfer scan's matrix-pipe filter (mode 7)
    reads from its workspace.  It keeps the seed it used at loss workspace + 8 bytes for the backward launch.  Returns
    (points [B,K*n,3], records, loss workspace, raster backward workspace, Chamfer workspace)."""
    B, K, _ = params.shape
    N, M = K * n, gt_points.shape[1]
    dev = params.device
    rec = _workspace('vpn_raster_records_size', B, K, Hr, Wr, dev=dev)
    lws = _workspace('vpn_raster_loss_workspace', B, Hr, Wr, dev=dev)
    rws = _workspace('vpn_raster_bwd_workspace', B, K, Hr, Wr, dev=dev)
    points = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
    cws = _workspace('vpn_chamfer_workspace', B, N, M, dev=dev)
    _lib.call('vpn_hotpath_sample_fwd', params, kinds, None, seed_host, seed_dev, int(sample_base), B, K, n, points, cam, Hr, Wr,
              float(sigma), rec, lws, gt_points, M, cws if features else None, cws.numel() * 4, s)
    return points, rec, lws, rws, cws


def _hotpath_scan(points, gt_points, cws, mode, rider, rec, K, Hr, Wr, s):
    """The Chamfer scan of the hot path in `mode` of vpn_chamfer_fwd_ws.  With `rider` (see _tile_rider_fits) the launch also
    prepares the raster's tiles in its tail: one entry per tile wave -- which tile (heaviest first), which primitives it
    sees, which quadrants each of them reaches -- instead of every tile wave finding that out for itself.  Returns
    (dist1, idx1, dist2, idx2, the tile entries or None)."""
    B, N, _ = points.shape
    M = gt_points.shape[1]
    d1, i1, d2, i2 = _nn_outputs(B, N, M, points.device)
    order = None
    if rider:
        order = _workspace('vpn_raster_order_size', B, Hr, Wr, dev=points.device, dtype=torch.int64)    # 48-byte tile entries
        _lib.call('vpn_hotpath_chamfer_fwd', points, gt_points, B, N, M, d1, i1, d2, i2, cws, cws.numel() * 4, mode, rec, K, Hr, Wr,
                  order, s)
    else:
        _lib.call('vpn_chamfer_fwd_ws', points, gt_points, B, N, M, d1, i1, d2, i2, cws, cws.numel() * 4, mode, s)
    return d1, i1, d2, i2, order


def _hotpath_raster_fin(params, kinds, cam, gt_sil, gt_depth, H, W, sigma, gamma, z_far, sil_mse, w_sil, w_depth, rec, lws, rws,
                        cws, N, M, cd_w1, cd_w2, w_cd, losses, step_counter, order, s):
    """Last forward launch of the hot path: the raster's forward+backward pass and the loss finalisation (image losses,
    per-sample Chamfer terms from the mode-7 scan's per-workgroup sums in `cws`, total -> losses [4]; `step_counter`, the
    device seed, is advanced by one unless None) in ONE launch.  `order`: the scan rider's tile entries, or None."""
    B, K, _ = params.shape
    _lib.call('vpn_raster_total_fwd_fin', params, kinds, cam, B, K, H, W, float(sigma), float(gamma), float(z_far), gt_sil,
              gt_depth, sil_mse, float(w_sil), float(w_depth), rec, lws, rws, 1, cws, cws.numel() * 4, N, M, cd_w1, cd_w2,
              float(w_cd), losses, None, step_counter, order, s)


class HotPathLossFunction(Function):
    """One training-step loss of the reference's hot path in a single autograd node (train.py:243-262):
        total = w_cd * ChamferDistanceLoss(sample(params), gt_points; cd_w1, cd_w2) + w_sil * SilhouetteLoss
                + w_depth * L1(depth)
    Forward: sampler (+ raster records) -> Chamfer scans -> raster forward+backward pass (image losses and their gradient
    partials in one launch) -> loss finalisation (per-sample Chamfer losses, image losses, total).  Backward:
    Chamfer + sampler backward (writes d/dparams) -> raster finishing kernel (adds to it).  No intermediate ever goes
    through an ATen kernel.  Returns three scalars (silhouette loss, depth loss, total); only the total is
    differentiable (the first two are reported values: they are marked non-differentiable, so `out[0].backward()`
    raises instead of returning a wrong gradient).
    `seed`: int, or a device int64 tensor of one element read by the kernels (see _seed_args).
    cd_w1 / cd_w2 = config.CD_W1 / CD_W2 (chamfer_distance.py:10), sil_mse = SILHOUETTE_LOSS_FUNC != 'L1'."""

    @staticmethod
    def forward(ctx, params, kinds, cam, gt_points, gt_sil, gt_depth, n, seed, sample_base, H, W, sigma, gamma,
                z_far, w_cd, w_sil, w_depth, cd_w1=1.0, cd_w2=1.0, sil_mse=False, advance_seed=False):
        params, cam, gt_points = _f32c(params), _f32c(cam), _f32c(gt_points)
        B, K, _ = params.shape
        M = gt_points.shape[1]
        N = K * n
        dev = params.device
        kinds = kinds_tensor(kinds, dev)
        assert kinds.numel() == K and cam.shape == (B, 3) and gt_points.shape[0] == B
        s = _lib.stream()
        seed_host, seed_dev = _seed_args(seed)
        cd_w1, cd_w2, sil_mse = float(cd_w1), float(cd_w2), int(bool(sil_mse))
        gt_sil = _f32c(gt_sil).reshape(B, H, W) if gt_sil is not None else None
        gt_depth = _f32c(gt_depth).reshape(B, H, W) if gt_depth is not None else None
        losses = torch.empty((4,), dtype=torch.float32, device=dev)
        if advance_seed and seed_dev is None:
            raise ValueError('advance_seed needs a device seed (a CUDA int64 tensor of one element)')

        def raster_alone(rec, lws, rws, records_ready, stream):     # the forms whose finalisation is a launch of its own
            _lib.call('vpn_raster_total_fwd', params, kinds, cam, B, K, H, W, float(sigma), float(gamma), float(z_far), gt_sil,
                      gt_depth, sil_mse, float(w_sil), float(w_depth), rec, lws, rws, records_ready, stream)

        side = _side_stream(dev) if CONCURRENT_BRANCHES else None
        # fused: the Chamfer scan is the matrix-pipe filter on features that the sampler's launch wrote (mode 7)
        fused = side is None and bool(_lib.lib().vpn_hotpath_fused_features(B, K, n, M))
        if side is None:
            points, rec, lws, rws, cws = _hotpath_sample(params, kinds, cam, gt_points, n, seed_host, seed_dev, sample_base, H, W,
                                                         sigma, fused, s)
            d1, i1, d2, i2, order = _hotpath_scan(points, gt_points, cws, 7 if fused else 0, fused and _tile_rider_fits(K, H, W),
                                                  rec, K, H, W, s)
            if fused:
                _hotpath_raster_fin(params, kinds, cam, gt_sil, gt_depth, H, W, sigma, gamma, z_far, sil_mse, w_sil, w_depth, rec,
                                    lws, rws, cws, N, M, cd_w1, cd_w2, w_cd, losses, seed_dev if advance_seed else None, order, s)
            else:
                raster_alone(rec, lws, rws, 1, s)
        else:
            # the raster branch (independent of the sampler + Chamfer branch until the finalisation) runs on a side stream;
            # fork / join is captured into HIP graphs as such
            main = torch.cuda.current_stream()
            rec = _workspace('vpn_raster_records_size', B, K, H, W, dev=dev)
            lws = _workspace('vpn_raster_loss_workspace', B, H, W, dev=dev)
            rws = _workspace('vpn_raster_bwd_workspace', B, K, H, W, dev=dev)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                raster_alone(rec, lws, rws, 0, _lib.stream())
                for t in (params, kinds, cam, gt_sil, gt_depth, rec, lws, rws):
                    if t is not None:
                        t.record_stream(side)
            points = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
            cws = _workspace('vpn_chamfer_workspace', B, N, M, dev=dev)
            _lib.call('vpn_sample_fwd', params, kinds, None, seed_host, seed_dev, int(sample_base), B, K, n, points, s)
            d1, i1, d2, i2, _ = _hotpath_scan(points, gt_points, cws, 0, False, None, K, H, W, s)
            main.wait_stream(side)
        if not fused:
            _lib.call('vpn_loss_finalize', lws, B, H, W, d1, d2, N, M, cd_w1, cd_w2, float(w_cd), float(w_sil), float(w_depth),
                      losses, None, s)
        pattern = _grad_pattern(B, w_cd, dev)
        empty = torch.empty(0, device=dev)
        seed_t = seed if isinstance(seed, torch.Tensor) else empty
        if advance_seed and not fused:
            # the side-stream / unfused form advances the caller's counter here; when the sampler launch did not keep the
            # seed it used (side stream), the backward must not read the advanced counter: it gets a copy of the old one
            if not (side is None and seed_dev is not None):
                seed_t = seed.clone()
            seed.add_(1)
        # the sampler's launch of the one-stream path keeps the seed it used at loss_ws + 8: backward reads it from there,
        # whatever has happened to the caller's counter since
        seed_saved = side is None and seed_dev is not None
        ctx.save_for_backward(params, kinds, cam, gt_points, points, d1, i1, d2, i2, rec, rws, pattern,
                              lws if seed_saved else seed_t)
        ctx.meta = (B, K, n, M, H, W, 0 if seed_saved else seed_host, seed_dev is not None, int(sample_base), cd_w1, cd_w2,
                    float(w_cd) / B, seed_saved)
        sil, dep, tot, _ = losses.unbind(0)
        ctx.mark_non_differentiable(sil, dep)
        ctx.set_materialize_grads(False)       # no zero-filled gradients for the two reported (non-differentiable) values
        return sil, dep, tot

    @staticmethod
    def backward(ctx, _g_sil, _g_dep, grad_total):
        (params, kinds, cam, gt_points, points, d1, i1, d2, i2, rec, rws, pattern, seed_t) = ctx.saved_tensors
        B, K, n, M, H, W, seed, has_seed_dev, base, cd_w1, cd_w2, w_cd_over_b, seed_saved = ctx.meta
        N = K * n
        s = _lib.stream()
        seed_dev = None
        if seed_saved:                                          # seed_t is the loss workspace: effective seed at byte 8
            seed_dev = ctypes.c_void_p(seed_t.data_ptr() + 8)
        elif has_seed_dev:
            seed_dev = seed_t
        if grad_total is None:                                  # the total was not used (set_materialize_grads(False))
            return (None,) * 21
        grad_total = _f32c(grad_total).reshape(1)
        # Chamfer backward and sampler backward in one launch: the [B,N,3] point gradient never exists
        grad_params = torch.empty_like(params)
        if M <= FUSED_BWD_MAX_GT:          # ... and the raster's finishing step rides in the same launch
            # d total / d loss_b = (w_cd / B) * grad_total for every sample: the constant goes into the two Chamfer
            # weights and the kernel reads grad_total itself (no ATen kernel between autograd and the launch)
            _lib.call('vpn_hotpath_bwd', params, kinds, None, seed, seed_dev, base, B, K, n, points, gt_points, M, d1, i1, d2, i2,
                      None, cd_w1 * w_cd_over_b, cd_w2 * w_cd_over_b, cam, H, W, rec, rws, grad_total, grad_params, s)
            return (grad_params,) + (None,) * 20
        else:                                                   # GT clouds beyond the fused kernel's LDS match lists
            gvec = pattern * grad_total                         # d total / d loss_b [B]
            grad_points = torch.empty_like(points)
            _lib.call('vpn_chamfer_bwd', points, gt_points, d1, i1, d2, i2, gvec, B, N, M, cd_w1, cd_w2, grad_points, None, s)
            _lib.call('vpn_sample_bwd', params, kinds, None, seed, seed_dev, base, B, K, n, grad_points, grad_params, s)
        # the raster's gradient partials were produced by the forward launch: chain rule x upstream gradient, added
        _lib.call('vpn_raster_total_bwd', params, cam, B, K, H, W, rec, rws, grad_total, grad_params, 1, s)
        return (grad_params,) + (None,) * 20


_CAMS = {}


def _view_camera(B, dev):
    """cam [B,3] = (dist 1, elev 0, azim 0): the view-centred camera of train.py:172-174, cached per (B, device)."""
    key = (B, str(dev))
    if key not in _CAMS:
        _CAMS[key] = torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float32, device=dev).expand(B, 3).contiguous()
    return _CAMS[key]


class TrainStepLossFunction(Function):
    """The loss of one training iteration of the reference (train.py:243-262) as ONE autograd node, BASELINE config C5:

        total = L_VIEW_CD * ChamferDistanceLoss(pred, view_center_points)                          train.py:160
              + L_CAN_CD  * ChamferDistanceLoss(view_to_obj_points(pred, ...), canonical_points)   train.py:158-161
              + L_SIL     * SilhouetteLoss(primitives, silhouettes; dist 1, elev 0, azim 0)        train.py:169-176
              + L_VP_DIV  * VPDiverseLoss(translates, view_center_points)                          train.py:185
              + L_EMD     * sqrt(EarthMoverDistanceLoss(pred, view_center_points, eps, iters)[0]).mean()   train.py:193-195

    with pred = sample_predict_points (train.py:105-120) of params [B,K,10].  Forward: the hot path's three launches
    (sampler + raster records + Chamfer features, Chamfer scan + tile rider, raster with the loss finalisation), the
    auction, the object-centred cloud (camera transform, its Chamfer scan), the VP-diversity neighbours, one reduction;
    backward: ONE launch (vpn_trainstep_bwd).  No ATen kernel runs in either.  `weights` = (L_VIEW_CD, L_CAN_CD, L_SIL,
    L_VP_DIV, L_EMD) of config.py:13-17; a zero weight skips that term's backward (the reference multiplies it by 0), and
    L_SIL = 0 skips the render like train.py:167.  Returns six scalars (the five weighted terms, then the total); only the
    total is differentiable: backward through `out[5]` (the terms are marked non-differentiable)."""

    @staticmethod
    def forward(ctx, params, kinds, gt_view, gt_canon, gt_sil, dists, elevs, azims, angles, n, seed, sample_base, H, W,
                weights, eps=0.005, iters=50, advance_seed=False, cd_w1=1.0, cd_w2=1.0, sil_mse=False):
        from . import config
        params, gt_view = _f32c(params), _f32c(gt_view)
        B, K, _ = params.shape
        M = gt_view.shape[1]
        N = K * n
        dev = params.device
        kinds = kinds_tensor(kinds, dev)
        w_view, w_can, w_sil, w_div, w_emd = (float(x) for x in weights)
        cd_w1, cd_w2, sil_mse = float(cd_w1), float(cd_w2), int(bool(sil_mse))
        s = _lib.stream()
        seed_host, seed_dev = _seed_args(seed)
        if advance_seed and seed_dev is None:
            raise ValueError('advance_seed needs a device seed (a CUDA int64 tensor of one element)')
        if w_emd and N != M:
            raise ValueError('the EMD term needs as many predicted as ground-truth points (emd_module.py:36): %d vs %d' % (N, M))
        if M > FUSED_BWD_MAX_GT:           # the one-launch backward would refuse it, after the whole forward has run
            raise ValueError('TrainStepLossFunction takes at most %d ground-truth points (the match lists of its backward launch), '
                             'got %d' % (FUSED_BWD_MAX_GT, M))
        if not _lib.lib().vpn_hotpath_fused_features(B, K, n, M):
            raise ValueError('TrainStepLossFunction needs a shape the fused sampler / Chamfer path takes (K <= 64, large clouds)')
        f32 = dict(dtype=torch.float32, device=dev)
        render = w_sil != 0.0 and gt_sil is not None
        cam = _view_camera(B, dev)
        gt_sil = _f32c(gt_sil).reshape(B, H, W) if render else None
        sigma, gamma, z_far = config.RASTER_SIGMA, config.RASTER_GAMMA, config.RASTER_Z_FAR
        # the render's buffers exist (tiny) even when the silhouette term is off: the sampler launch writes the records
        Hr, Wr = (H, W) if render else (16, 16)
        hot = torch.empty((4,), **f32)
        # ---- hot path: sampler (+ records + features) -> view-centred Chamfer (+ tile rider) -> raster + finalisation
        points, rec, lws, rws, cws = _hotpath_sample(params, kinds, cam, gt_view, n, seed_host, seed_dev, sample_base, Hr, Wr,
                                                     sigma, True, s)
        # ---- EMD auction on the sampled cloud (train.py:193).  On a second stream when EMD_SIDE_STREAM: it needs only the
        #      sampler's points, nothing needs it before the final sums, and its workgroups (one per CU, 16 waves) leave
        #      every CU half of its wave slots and 32 KB of LDS -- the Chamfer scans and the raster run beside it
        emd_dist = emd_assign = None
        side = None
        if w_emd:
            side = _fork_side(dev) if EMD_SIDE_STREAM else None
            # ews: the auction's workspace stays alive until the join in front of the finalisation
            emd_dist, emd_assign, ews = _auction(points, gt_view, eps, iters, _emd_group(None),
                                            ctypes.c_void_p(side.cuda_stream) if side is not None else s)
        d1, i1, d2, i2, order = _hotpath_scan(points, gt_view, cws, 7, render and _tile_rider_fits(K, Hr, Wr), rec, K, Hr, Wr, s)
        if render:
            _hotpath_raster_fin(params, kinds, cam, gt_sil, None, H, W, sigma, gamma, z_far, sil_mse, w_sil, 0.0, rec, lws, rws,
                                cws, N, M, cd_w1, cd_w2, w_view, hot, seed_dev if advance_seed else None, order, s)
        else:
            # train.py:167: no render; the Chamfer term alone (H = W = 0: no image losses)
            _lib.call('vpn_loss_finalize', lws, B, 0, 0, d1, d2, N, M, cd_w1, cd_w2, w_view, 0.0, 0.0, hot, None, s)
            if advance_seed:
                raise ValueError('advance_seed rides in the raster launch: it needs the silhouette term (L_SIL != 0)')
        # ---- object-centred Chamfer (train.py:158-161): computed even at weight 0, like the reference
        cn = None
        if gt_canon is not None:
            gt_canon = _f32c(gt_canon)
            Mc = gt_canon.shape[1]
            cam4 = [_f32c(c.reshape(-1)) for c in (dists, elevs, azims, angles)]
            canon = torch.empty_like(points)
            _lib.call('vpn_camera_transform_fwd', points, cam4[0], cam4[1], cam4[2], cam4[3], B, N, 1, canon, s)
            cd1, ci1, cd2, ci2 = _nn_outputs(B, N, Mc, dev)
            ccws = _workspace('vpn_chamfer_workspace', B, N, Mc, dev=dev)
            _lib.call('vpn_chamfer_fwd_ws', canon, gt_canon, B, N, Mc, cd1, ci1, cd2, ci2, ccws, ccws.numel() * 4, 0, s)
            mat = None
            if w_can:
                mat = torch.empty((B, 9), **f32)
                _lib.call('vpn_camera_matrix', cam4[0], cam4[1], cam4[2], cam4[3], B, 1, mat, s)
            cn = (canon, gt_canon, mat, cd1, ci1, cd2, ci2, Mc)
        # ---- VP-diversity (train.py:185)
        dv = dws = None
        if w_div:
            dv = _nn_outputs(B, K, M, dev)
            dws = _workspace('vpn_vpdiv_workspace', B, K, dev=dev, dtype=torch.int64)
            # the centres' direction stays in the workspace: the finalisation's per-sample pass merges it
            _lib.call('vpn_vpdiv_fwd', params, gt_view, B, K, M, None, None, dv[2], dv[3], dws, s)
        out = torch.empty((6,), **f32)
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)
        fws = _workspace('vpn_trainstep_workspace', B, dev=dev)
        _lib.call('vpn_trainstep_finalize', hot, emd_dist, cn[3] if cn else None, cn[5] if cn else None, None,
                  dv[2] if dv else None, B, N, M, cn[7] if cn else 0, K, w_view, w_can, w_sil if render else 0.0, w_div, w_emd,
                  cd_w1, cd_w2, fws, dws, dv[0] if dv else None, dv[1] if dv else None, out, s)
        ctx.meta = (B, K, n, M, H, W, seed_host, int(sample_base), cd_w1, cd_w2, w_view, w_can, w_div, w_emd, render,
                    seed_dev is not None, cn[7] if cn else 0)
        # the sampler's launch keeps the seed it used at loss_ws + 8: backward reads it from there
        ctx.tensors = dict(params=params, kinds=kinds, cam=cam, gt_view=gt_view, points=points, d1=d1, i1=i1, d2=d2, i2=i2, rec=rec,
                           rws=rws, lws=lws, emd_dist=emd_dist, emd_assign=emd_assign, dv=dv, cn=cn if (cn and w_can) else None)
        terms = out.unbind(0)
        ctx.mark_non_differentiable(*terms[:5])
        ctx.set_materialize_grads(False)       # no zero-filled gradients for the five reported terms
        return terms

    @staticmethod
    def backward(ctx, _g0, _g1, _g2, _g3, _g4, grad_total):
        t = ctx.tensors
        if grad_total is None:
            return (None,) * 21
        (B, K, n, M, H, W, seed_host, base, cd_w1, cd_w2, w_view, w_can, w_div, w_emd, render, has_seed_dev, Mc) = ctx.meta
        N = K * n
        g = _f32c(grad_total).reshape(1)
        grad_params = torch.empty_like(t['params'])
        seed_dev = ctypes.c_void_p(t['lws'].data_ptr() + 8) if has_seed_dev else None
        has_cn = t['cn'] is not None
        dv, cn = t['dv'] or (None,) * 4, t['cn'] or (None,) * 7       # a term that is off: NULL for each of its tensors
        _lib.call('vpn_trainstep_bwd', t['params'], t['kinds'], 0 if has_seed_dev else seed_host, seed_dev, base, B, K, n,
                  t['points'], t['gt_view'], M, t['d1'], t['i1'], t['d2'], t['i2'], cd_w1 * w_view / B, cd_w2 * w_view / B,
                  t['cam'], H, W, t['rec'] if render else None, t['rws'] if render else None, g,
                  t['emd_dist'], t['emd_assign'], w_emd / (B * N), *dv, w_div * 0.5 / (K * B), w_div * 1.0 / (M * B), *cn[:7],
                  (w_can * cd_w1 / (N * B)) if has_cn else 0.0, (w_can * cd_w2 / (Mc * B)) if has_cn else 0.0, Mc if has_cn else 0,
                  grad_params, _lib.stream())
        return (grad_params,) + (None,) * 20


# ---- the GCN refinement stage (modules/network/gcn.py of the reference; modules/gcn.py here)

class GcnGraph:
    """The normalised mesh adjacency of PyG's GCNConv in CSR form, on one device: row_ptr [N+1] int32, col [nnz] int32,
    w [nnz] fp32 (see gcn_normalized_adjacency), plus the (2, 2E) int64 edge index it was built from."""

    def __init__(self, row_ptr, col, w, n, edge_index):
        self.row_ptr, self.col, self.w, self.n, self.edge_index = row_ptr, col, w, n, edge_index


def gcn_edges(faces):
    """Unique undirected edges (E, 2) int64 (host) of a triangle list, each as (min, max), sorted lexicographically."""
    f = faces.detach().cpu().long().reshape(-1, 3)
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = torch.stack([e.min(1)[0], e.max(1)[0]], 1)
    e = e[e[:, 0] != e[:, 1]]
    return torch.unique(e, dim=0)


def gcn_edge_index(edges):
    """(E, 2) -> (2, 2E) with both directions, as gcn.py:63-67 builds it: `torch.cat([edges, edges.flip(1)]).view(2, -1)`
    reinterprets memory, so row 0 is edges.flatten() and row 1 is edges.flip(1).flatten(): column 2m is (a_m, b_m) and
    column 2m + 1 is (b_m, a_m)."""
    return torch.cat([edges, edges.flip(1)]).view(2, -1)


def gcn_normalized_adjacency(edges, n):
    """CSR of A_hat = D^-1/2 (A + I) D^-1/2 over n vertices, PyG GCNConv's default `gcn_norm` (Kipf & Welling, ICLR 2017,
    eq. 2): A_ij = 1 for every undirected edge (both directions), self loops added with weight 1, the degree counted with
    the self loop (deg_i = 1 + number of neighbours), no edge weights, fp32 deg^-1/2 and fp32 products
    w_ij = deg_i^-1/2 * deg_j^-1/2.  Entries of a row are sorted by column (the self loop among them).  Host tensors:
    (row_ptr [n+1] int32, col [nnz] int32, w [nnz] fp32)."""
    e = edges.long()
    loops = torch.arange(n, dtype=torch.long)
    src = torch.cat([e[:, 0], e[:, 1], loops])
    dst = torch.cat([e[:, 1], e[:, 0], loops])
    deg = torch.zeros(n, dtype=torch.float32).index_add_(0, dst, torch.ones(dst.numel(), dtype=torch.float32))
    dis = deg.pow(-0.5)
    order = torch.argsort(dst * n + src)
    row, col = dst[order], src[order]
    w = dis[row] * dis[col]
    row_ptr = torch.zeros(n + 1, dtype=torch.long)
    row_ptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
    return row_ptr.int(), col.int(), w.float()


_GCN_GRAPHS = {}


def gcn_graph(faces, n, device):
    """The GcnGraph of a face topology over n vertices on `device`, built on the host once per (face content, n, device)
    (keyed by ops.faces_fingerprint, like the face cache): a repeated step does no host work and no synchronisation."""
    key = (faces_fingerprint(faces), int(n), str(torch.device(device)))
    hit = _GCN_GRAPHS.get(key)
    if hit is None:
        if len(_GCN_GRAPHS) > 64:
            _GCN_GRAPHS.clear()
        edges = gcn_edges(faces)
        if edges.numel() and int(edges.max()) >= n:
            raise ValueError('faces index vertex %d of a %d-vertex mesh' % (int(edges.max()), n))
        rp, col, w = gcn_normalized_adjacency(edges, int(n))
        hit = GcnGraph(rp.to(device), col.to(device), w.to(device), int(n), gcn_edge_index(edges).to(device))
        _GCN_GRAPHS[key] = hit
    return hit


def _colsum(x, mask, S, R, ld, off, C):
    ws = _workspace('vpn_gcn_colsum_workspace', S, R, C, dev=x.device)
    out = torch.empty((S, C), dtype=torch.float32, device=x.device)
    _lib.call('vpn_gcn_colsum', x, mask, S, R, ld, off, C, ws, out, _lib.stream())
    return out


class GcnAggregateFunction(Function):
    """y [B,N,C] = A_hat h [B,N,C] + bias [C] (ReLU'd when relu): the propagation of GCNConv over a GcnGraph.  Backward:
    A_hat is symmetric, so dh = A_hat (g * [y > 0]) by the same gather; dbias = sum over (b, i) in a fixed order."""

    @staticmethod
    def forward(ctx, h, bias, row_ptr, col, w, relu=False):
        h = _f32c(h)
        B, N, C = h.shape
        assert row_ptr.numel() == N + 1, 'graph has %d vertices, features %d' % (row_ptr.numel() - 1, N)
        b = _f32c(bias) if bias is not None else None
        y = torch.empty_like(h)
        _lib.call('vpn_gcn_aggregate', h, row_ptr, col, w, b, None, B, N, C, int(bool(relu)), y, _lib.stream())
        ctx.save_for_backward(row_ptr, col, w, y if relu else None)
        ctx.meta = (B, N, C, bias is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        row_ptr, col, w, y = ctx.saved_tensors
        B, N, C, has_bias = ctx.meta
        g = _f32c(g)
        gh = gb = None
        if ctx.needs_input_grad[0]:
            gh = torch.empty_like(g)
            _lib.call('vpn_gcn_aggregate', g, row_ptr, col, w, None, y, B, N, C, 0, gh, _lib.stream())
        if has_bias and ctx.needs_input_grad[1]:
            gb = _colsum(g, y, 1, B * N, C, 0, C).reshape(C)
        return gh, gb, None, None, None, None


def gcn_bounds(rgbs):
    """get_bound_of_images (gcn.py:90-133) on the device: rgbs [B,C,H,W] -> bounds [B,4] fp32, bit-exact, no host sync.
    Not differentiable (the reference's bounds are integers written into a fresh tensor)."""
    img = _f32c(rgbs.detach())
    assert img.dim() == 4
    B, C, H, W = img.shape
    out = torch.empty((B, 4), dtype=torch.float32, device=img.device)
    _lib.call('vpn_gcn_bounds', img, B, C, H, W, out, _lib.stream())
    return out


def _gcn_dims(maps):
    dims = []
    for m in maps:
        dims += [int(m.shape[1]), int(m.shape[2]), int(m.shape[3])]
    return dims + [0] * (12 - len(dims))


GCN_SORT_MAX_N = 8192           # csrc/gcn.hip: the vertices per sample the pooling backward sorts in LDS


class GcnInputFunction(Function):
    """conv1's input [B,N,venc + sum C_l + G] = [encoding | pooled | global] (gcn.py:36-42) in one pass, no torch.cat:
    venc = 39 (positional encoding, gcn.py:73-82), 3 (the vertices) or 0; pooled = perceptual_feature_pooling
    (gcn.py:135-164) of the L <= 4 NCHW maps at the grid given by bounds [B,4] and the per-sample z / y extents of
    verts [B,N,3]; global_features [B,G] (or None) repeated over the vertices.  Differentiable w.r.t. verts (through
    the encoding, the grid and the min / max), the maps and the global features.  The maps' gradient sorts the vertices
    of a sample in LDS: with N > GCN_SORT_MAX_N a map that requires a gradient is a ValueError here, before any launch
    (the forward and the vertices' gradient take any N)."""

    @staticmethod
    def forward(ctx, verts, bounds, global_features, venc, *maps):
        verts = _f32c(verts)
        B, N, _ = verts.shape
        L = len(maps)
        assert L <= 4 and verts.shape[2] == 3
        if N > GCN_SORT_MAX_N and any(ctx.needs_input_grad[4:4 + L]):
            raise ValueError('GcnInputFunction: N = %d vertices and a map requires a gradient; its backward sorts at most '
                             '%d per sample' % (N, GCN_SORT_MAX_N))
        maps = tuple(_f32c(m) for m in maps)
        for m in maps:
            assert m.dim() == 4 and m.shape[0] == B, m.shape
        gf = _f32c(global_features) if global_features is not None else None
        G = int(gf.shape[1]) if gf is not None else 0
        dev = verts.device
        dims = _gcn_dims(maps)
        ctot = int(venc) + sum(int(m.shape[1]) for m in maps) + G
        out = torch.empty((B, N, ctot), dtype=torch.float32, device=dev)
        ext = ext_idx = grid = mws = None
        if L:
            bounds = _f32c(bounds)
            ext = torch.empty((B, 4), dtype=torch.float32, device=dev)
            ext_idx = torch.empty((B, 4), dtype=torch.int32, device=dev)
            grid = torch.empty((B, N, 2), dtype=torch.float32, device=dev)
            mws = _workspace('vpn_gcn_maps_workspace', B, L, *dims, dev=dev)
        fp = [maps[l] if l < L else None for l in range(4)]
        _lib.call('vpn_gcn_input_fwd', verts, bounds if L else None, gf, B, N, G, int(venc), L, *fp, *dims, ext, ext_idx, grid,
                  mws, out, _lib.stream())
        ctx.save_for_backward(verts, bounds if L else None, ext, ext_idx, grid, mws)
        ctx.meta = (B, N, G, int(venc), L, dims, [tuple(m.shape) for m in maps])
        return out

    @staticmethod
    def backward(ctx, g):
        verts, bounds, ext, ext_idx, grid, mws = ctx.saved_tensors
        B, N, G, venc, L, dims, shapes = ctx.meta
        g = _f32c(g)
        dev = g.device
        need_v = ctx.needs_input_grad[0]
        need_m = any(ctx.needs_input_grad[4:4 + L])
        gv = torch.empty((B, N, 3), dtype=torch.float32, device=dev) if need_v else None
        gm = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes] if need_m else []
        if need_v or need_m:
            ws = _workspace('vpn_gcn_input_bwd_workspace', B, N, L, *dims, dev=dev, floor=1)
            fp = [gm[l] if l < len(gm) else None for l in range(4)]
            _lib.call('vpn_gcn_input_bwd', g, verts, bounds, B, N, G, venc, L, *dims, ext, ext_idx, grid, mws, ws, gv, *fp,
                      _lib.stream())
        gg = None
        if G and ctx.needs_input_grad[2]:
            ctot = g.shape[2]
            gg = _colsum(g, None, B, N, ctot, ctot - G, G)
        return (gv, None, gg, None) + (tuple(gm) if need_m else (None,) * L)


def _gcn_factored_check(verts, global_features, weight, venc, maps):
    """The contract of gcn_factored_input, from shapes alone: ValueError before any launch."""
    if venc not in (0, 3, 39):
        raise ValueError('gcn_factored_input: venc is %r; the kernels take 0, 3 or 39' % (venc,))
    if len(maps) > 4:
        raise ValueError('gcn_factored_input: %d maps; at most 4' % len(maps))
    if verts.dim() != 3 or verts.shape[2] != 3 or verts.shape[0] < 1 or verts.shape[1] < 1:
        raise ValueError('gcn_factored_input: verts must be [B,N,3], got %r' % (tuple(verts.shape),))
    B, N = int(verts.shape[0]), int(verts.shape[1])
    if N > GCN_SORT_MAX_N:
        raise ValueError('gcn_factored_input: N = %d vertices; at most %d' % (N, GCN_SORT_MAX_N))
    for m in maps:
        if m.dim() != 4 or m.shape[0] != B or min(m.shape[1:]) < 1:
            raise ValueError('gcn_factored_input: a map must be [B,C,H,W] with B = %d, got %r' % (B, tuple(m.shape)))
    G = 0
    if global_features is not None:
        if global_features.dim() != 2 or global_features.shape[0] != B:
            raise ValueError('gcn_factored_input: global_features must be [B,G] with B = %d, got %r'
                             % (B, tuple(global_features.shape)))
        G = int(global_features.shape[1])
    if weight.dim() != 2:
        raise ValueError('gcn_factored_input: weight must be [ctot,Cout], got %r' % (tuple(weight.shape),))
    ctot = int(venc) + sum(int(m.shape[1]) for m in maps) + G
    if int(weight.shape[0]) != ctot:
        raise ValueError('gcn_factored_input: weight has %d rows; venc + sum C_l + G = %d' % (weight.shape[0], ctot))
    if int(weight.shape[1]) < 4 or int(weight.shape[1]) % 4:
        raise ValueError('gcn_factored_input: Cout = %d is not a positive multiple of 4' % weight.shape[1])
    return B, N, G, int(weight.shape[1])


class GcnFactoredInputFunction(Function):
    """h [B,N,Cout] = [encoding | pooled | global] weight, the product GcnInputFunction + torch.matmul form, without the
    [B,N,ctot] row: the maps and the global features are projected first (small dense GEMMs, here and
    not on the autograd tape), then every vertex gathers its 4 corners per level from the projected maps.  weight
    [venc + sum C_l + G, Cout] is conv1's parameter as it stands and receives one full gradient.  Differentiable w.r.t.
    verts, global_features, weight and each map; a gradient nobody needs is not computed."""

    @staticmethod
    def forward(ctx, verts, bounds, global_features, weight, venc, *maps):
        venc = int(venc)
        B, N, G, Cout = _gcn_factored_check(verts, global_features, weight, venc, maps)
        verts, weight = _f32c(verts), _f32c(weight)
        maps = tuple(_f32c(m) for m in maps)
        gf = _f32c(global_features) if G else None
        L, dev = len(maps), verts.device
        hw = []
        for m in maps:
            hw += [int(m.shape[2]), int(m.shape[3])]
        hw += [0] * (8 - len(hw))
        rows = [venc]                                        # first weight row of every level, then of the global block
        for m in maps:
            rows.append(rows[-1] + int(m.shape[1]))
        ext = ext_idx = grid = proj = gth = None
        if L:
            bounds = _f32c(bounds)
            ext = torch.empty((B, 4), dtype=torch.float32, device=dev)
            ext_idx = torch.empty((B, 4), dtype=torch.int32, device=dev)
            grid = torch.empty((B, N, 2), dtype=torch.float32, device=dev)
            proj = _workspace('vpn_gcn_factored_proj_workspace', B, Cout, L, *hw, dev=dev).view(B, -1, Cout)
            p0 = 0
            for l, m in enumerate(maps):                     # P_l = map_l (NHWC) Theta_l, straight into its pixels
                n = hw[2 * l] * hw[2 * l + 1]
                torch.bmm(m.flatten(2).transpose(1, 2), weight[rows[l]:rows[l + 1]].expand(B, -1, -1),
                          out=proj[:, p0:p0 + n])
                p0 += n
        if G:
            gth = torch.mm(gf, weight[rows[L]:])
        out = torch.empty((B, N, Cout), dtype=torch.float32, device=dev)
        _lib.call('vpn_gcn_factored_fwd', verts, bounds if L else None, gth, weight if venc else None, proj, B, N, Cout,
                  venc, L, *hw, ext, ext_idx, grid, out, _lib.stream())
        ctx.save_for_backward(verts, bounds if L else None, gf, weight, ext, ext_idx, grid, proj, *maps)
        ctx.meta = (B, N, G, Cout, venc, L, hw, rows)
        return out

    @staticmethod
    def backward(ctx, g):
        verts, bounds, gf, weight, ext, ext_idx, grid, proj = ctx.saved_tensors[:8]
        maps = ctx.saved_tensors[8:]
        B, N, G, Cout, venc, L, hw, rows = ctx.meta
        g = _f32c(g)
        dev = g.device
        need_v, need_g, need_w = ctx.needs_input_grad[0], bool(G) and ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        need_m = [bool(x) for x in ctx.needs_input_grad[5:5 + L]]
        gv = torch.empty((B, N, 3), dtype=torch.float32, device=dev) if need_v else None
        gw = torch.empty_like(weight) if need_w else None
        gproj = None
        if L and (need_w or any(need_m)):
            gproj = _workspace('vpn_gcn_factored_proj_workspace', B, Cout, L, *hw, dev=dev).view(B, -1, Cout)
        if need_v or gproj is not None or (need_w and venc):
            ws = _workspace('vpn_gcn_factored_bwd_workspace', B, N, Cout, venc, L, *hw, dev=dev, floor=1)
            _lib.call('vpn_gcn_factored_bwd', g, verts, bounds, weight if venc else None, proj, B, N, Cout, venc, L, *hw,
                      ext, ext_idx, grid, ws, gv, gproj, gw if venc else None, _lib.stream())   # dTheta_e: gw's first rows
        gm = [None] * L
        p0 = 0
        for l, m in enumerate(maps):
            n = hw[2 * l] * hw[2 * l + 1]
            if need_w:                                       # dTheta_l = sum_b map_l^T dP_l
                torch.sum(torch.bmm(m.flatten(2), gproj[:, p0:p0 + n]), 0, out=gw[rows[l]:rows[l + 1]])
            if need_m[l]:                                    # dmap_l = Theta_l dP_l^T, NCHW as it comes out
                gm[l] = torch.bmm(weight[rows[l]:rows[l + 1]].expand(B, -1, -1),
                                  gproj[:, p0:p0 + n].transpose(1, 2)).view(m.shape)
            p0 += n
        gg = None
        if G and (need_w or need_g):
            gsum = _colsum(g, None, B, N, Cout, 0, Cout)     # d(g Theta_g) [B,Cout]
            if need_w:
                torch.mm(gf.t(), gsum, out=gw[rows[L]:])
            if need_g:
                gg = torch.mm(gsum, weight[rows[L]:].t())
        return (gv, None, gg, gw, None) + tuple(gm)


def gcn_factored_input(verts, bounds, global_features, weight, venc, maps):
    """[encoding(verts) | pooled(maps at the grid of verts and bounds) | global_features] @ weight -> [B,N,Cout] in factored
    form (GcnFactoredInputFunction).  venc in {0, 3, 39}; at most 4 maps [B,C_l,H_l,W_l] (none allowed: bounds is then
    unused); global_features [B,G] or None; N <= 8192; weight [venc + sum C_l + G, Cout] with Cout % 4 == 0.  Anything else
    raises ValueError before any launch."""
    return GcnFactoredInputFunction.apply(verts, bounds, global_features, weight, venc, *maps)


# ---- the layer pairs of the GCN as one linear map each (csrc/gcnpair.hip)

GCN_HOP2_MAX_ROWS = 128         # csrc/gcnpair.hip: the rows of a block, both hops of which run in LDS
GCN_PROJECT_MAX_CI = 1024       # csrc/gcnpair.hip: the rows of Theta the skinny projection stages in LDS
GCN_PROJECT_MAX_CO = 4

_GCN_BLOCKS = {}


def gcn_closed_ranges(edges, n):
    """Starts (ascending, the first is 0) of the finest split of [0, n) into consecutive index ranges that no edge of
    `edges` (E, 2) crosses: i starts a range when no edge (a, b), a < b, has a < i <= b.  Host list of ints."""
    e = edges.long().reshape(-1, 2)
    d = torch.zeros(n + 1, dtype=torch.long)
    if e.numel():
        lo, hi = e.min(1)[0], e.max(1)[0]
        d.index_add_(0, lo + 1, torch.ones_like(lo))
        d.index_add_(0, hi + 1, -torch.ones_like(hi))
    cover = torch.cumsum(d, 0)[:n]
    return torch.nonzero(cover == 0).flatten().tolist()


def gcn_block_starts(edges, n, limit=GCN_HOP2_MAX_ROWS):
    """The block table of `edges` over n vertices as a host list [0, ..., n]: consecutive closed ranges
    (gcn_closed_ranges) merged left to right while a block keeps at most `limit` rows.  None when a closed range alone
    has more."""
    closed = gcn_closed_ranges(edges, n) + [n]
    starts = [0]
    for i in range(1, len(closed)):
        if closed[i] - closed[i - 1] > limit:
            return None
        if closed[i] - starts[-1] > limit:
            starts.append(closed[i - 1])
    return starts + [n]


def gcn_blocks(faces, n, device):
    """The block table of a face topology for gcn_aggregate2: int32 [nblocks + 1] starts on `device` of index ranges of at
    most GCN_HOP2_MAX_ROWS vertices that cover [0, n) and that no edge crosses, or None when the mesh has no such table
    (gcn_aggregate2 then takes two one-hop launches).  Built on the host once per (face content, n, device), like
    gcn_graph: a repeated step does no host work, no device read and no synchronisation."""
    key = (faces_fingerprint(faces), int(n), str(torch.device(device)))
    if key not in _GCN_BLOCKS:
        if len(_GCN_BLOCKS) > 64:
            _GCN_BLOCKS.clear()
        edges = gcn_edges(faces)
        if edges.numel() and int(edges.max()) >= n:
            raise ValueError('faces index vertex %d of a %d-vertex mesh' % (int(edges.max()), n))
        starts = gcn_block_starts(edges, int(n))
        _GCN_BLOCKS[key] = None if starts is None else torch.tensor(starts, dtype=torch.int32).to(device)
    return _GCN_BLOCKS[key]


def _gcn_aggregate2_check(h, u, bias, graph, blocks):
    """The contract of gcn_aggregate2, from shapes alone: ValueError before any launch."""
    if h.dim() != 3 or min(h.shape) < 1:
        raise ValueError('gcn_aggregate2: h must be [B,N,C], got %r' % (tuple(h.shape),))
    B, N, C = (int(s) for s in h.shape)
    if graph.row_ptr.numel() != N + 1:
        raise ValueError('gcn_aggregate2: the graph has %d vertices, h has %d' % (graph.row_ptr.numel() - 1, N))
    for name, v in (('u', u), ('bias', bias)):
        if v is not None and tuple(v.shape) != (C,):
            raise ValueError('gcn_aggregate2: %s must be [C] with C = %d, got %r' % (name, C, tuple(v.shape)))
    if blocks is not None and (blocks.dim() != 1 or blocks.dtype != torch.int32 or not 2 <= blocks.numel() <= N + 1):
        raise ValueError('gcn_aggregate2: blocks must be int32 [nblocks + 1] with 1 <= nblocks <= N = %d (ops.gcn_blocks), '
                         'got %s %r' % (N, blocks.dtype, tuple(blocks.shape)))
    return B, N, C


class GcnAggregate2Function(Function):
    """y [B,N,C] = A_hat (A_hat h + u) + bias (ReLU'd when relu): two propagations of GcnAggregateFunction back to back,
    bit-equal to them.  With a block table (ops.gcn_blocks) both hops of a block run in LDS in one launch and the
    intermediate never reaches memory; with blocks = None they are two one-hop launches through a scratch buffer.  Backward:
    dh = A_hat A_hat (g * [y > 0]) by the same launch on the masked gradient, du = the column sum of its intermediate (per
    block in row order, then the blocks in order), dbias = the column sum of the masked gradient.  No atomics; only y is
    saved, and only when relu."""

    @staticmethod
    def forward(ctx, h, u, bias, row_ptr, col, w, blocks, relu=False):
        h = _f32c(h)
        B, N, C = h.shape
        uu = _f32c(u) if u is not None else None
        bb = _f32c(bias) if bias is not None else None
        y = torch.empty_like(h)
        if blocks is not None:
            _lib.call('vpn_gcn_aggregate2', h, None, row_ptr, col, w, blocks, blocks.numel() - 1, uu, bb, B, N, C,
                      int(bool(relu)), y, None, _lib.stream())
        else:
            t = torch.empty_like(h)
            _lib.call('vpn_gcn_aggregate', h, row_ptr, col, w, uu, None, B, N, C, 0, t, _lib.stream())
            _lib.call('vpn_gcn_aggregate', t, row_ptr, col, w, bb, None, B, N, C, int(bool(relu)), y, _lib.stream())
        ctx.save_for_backward(row_ptr, col, w, blocks, y if relu else None)
        ctx.meta = (B, N, C, u is not None, bias is not None)
        return y

    @staticmethod
    def backward(ctx, g):
        row_ptr, col, w, blocks, y = ctx.saved_tensors
        B, N, C, has_u, has_bias = ctx.meta
        g = _f32c(g)
        need_h, need_u = ctx.needs_input_grad[0], has_u and ctx.needs_input_grad[1]
        gh = gu = gb = None
        if (need_h or need_u) and blocks is not None:
            nb = blocks.numel() - 1
            gh = torch.empty_like(g)
            part = _workspace('vpn_gcn_aggregate2_workspace', B, nb, C, dev=g.device) if need_u else None
            _lib.call('vpn_gcn_aggregate2', g, y, row_ptr, col, w, blocks, nb, None, None, B, N, C, 0, gh, part, _lib.stream())
            if need_u:
                gu = _colsum(part, None, 1, B * nb, C, 0, C).reshape(C)
        elif need_h or need_u:
            t = torch.empty_like(g)
            _lib.call('vpn_gcn_aggregate', g, row_ptr, col, w, None, y, B, N, C, 0, t, _lib.stream())
            if need_h:
                gh = torch.empty_like(g)
                _lib.call('vpn_gcn_aggregate', t, row_ptr, col, w, None, None, B, N, C, 0, gh, _lib.stream())
            if need_u:
                gu = _colsum(t, None, 1, B * N, C, 0, C).reshape(C)
        if has_bias and ctx.needs_input_grad[2]:
            gb = _colsum(g, y, 1, B * N, C, 0, C).reshape(C)
        return gh if need_h else None, gu, gb, None, None, None, None, None


def gcn_aggregate2(h, u, bias, graph, blocks=None, relu=False):
    """A_hat (A_hat h + u) + bias, ReLU'd when relu (GcnAggregate2Function): h [B,N,C], u and bias [C] or None, graph a
    GcnGraph over N vertices, blocks the table ops.gcn_blocks gives for the same faces (None: two one-hop launches, the
    same bits).  Anything else raises ValueError before any launch."""
    _gcn_aggregate2_check(h, u, bias, graph, blocks)
    return GcnAggregate2Function.apply(h, u, bias, graph.row_ptr, graph.col, graph.w, blocks, relu)


def _gcn_project_check(x, theta):
    """The contract of gcn_project, from shapes alone: ValueError before any launch."""
    if theta.dim() != 2 or min(theta.shape) < 1:
        raise ValueError('gcn_project: theta must be [Ci,Co], got %r' % (tuple(theta.shape),))
    Ci, Co = int(theta.shape[0]), int(theta.shape[1])
    if Co > GCN_PROJECT_MAX_CO:
        raise ValueError('gcn_project: Co = %d output columns; at most %d (wider products are torch.matmul)'
                         % (Co, GCN_PROJECT_MAX_CO))
    if Ci > GCN_PROJECT_MAX_CI:
        raise ValueError('gcn_project: Ci = %d; at most %d' % (Ci, GCN_PROJECT_MAX_CI))
    if x.dim() < 1 or int(x.shape[-1]) != Ci or x.numel() == 0:
        raise ValueError('gcn_project: x must be [..., Ci] with Ci = %d and at least one row, got %r' % (Ci, tuple(x.shape)))
    return x.numel() // Ci, Ci, Co


class GcnProjectFunction(Function):
    """out [..., Co] = x [..., Ci] theta [Ci, Co] for Co <= 4: the memory-bound product no GEMM tile fits (conv5 . conv6
    of the collapsed GCN is 512 -> 3).  x is read once, every result is the fixed-order sum of a wave.  Backward: dx =
    g theta^T and dtheta = x^T g as 64-row partial sums added in chunk order, one launch plus the final sum; either is
    skipped when nobody needs it.  No atomics."""

    @staticmethod
    def forward(ctx, x, theta):
        R, Ci, Co = _gcn_project_check(x, theta)
        x, theta = _f32c(x), _f32c(theta)
        out = torch.empty(x.shape[:-1] + (Co,), dtype=torch.float32, device=x.device)
        _lib.call('vpn_gcn_project_fwd', x, theta, R, Ci, Co, out, _lib.stream())
        ctx.save_for_backward(x, theta)
        ctx.meta = (R, Ci, Co)
        return out

    @staticmethod
    def backward(ctx, g):
        x, theta = ctx.saved_tensors
        R, Ci, Co = ctx.meta
        g = _f32c(g)
        need_x, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gx = torch.empty_like(x) if need_x else None
        gt = torch.empty_like(theta) if need_t else None
        if need_x or need_t:
            ws = _workspace('vpn_gcn_project_bwd_workspace', R, Ci, Co, dev=g.device) if need_t else None
            _lib.call('vpn_gcn_project_bwd', g, x, theta, R, Ci, Co, ws, gx, gt, _lib.stream())
        return gx, gt


def gcn_project(x, theta):
    """x [..., Ci] @ theta [Ci, Co] -> [..., Co] for Co <= 4 and Ci <= 1024 (GcnProjectFunction).  Anything else raises
    ValueError before any launch."""
    return GcnProjectFunction.apply(x, theta)


# ---- mesh regularisers (csrc/meshreg.hip): edge length, uniform Laplacian, normal consistency

MESHREG_TERMS = {'edge': _H['VPN_MESHREG_EDGE'], 'lap': _H['VPN_MESHREG_LAP'], 'normal': _H['VPN_MESHREG_NORMAL']}
MESHREG_MAX_ITEMS = _H['VPN_MESHREG_MAX_ITEMS']
_MESH_TOPOLOGIES = {}


class MeshTopology:
    """What the regularisers need of one face topology over n vertices, int32 tables on one device:

        faces [F,3]; edges [E,2] (ops.gcn_edges: unique, a < b, sorted); nbr_ptr [n+1] / nbr [2E]: the neighbours of a vertex,
        ascending; adj [F,3]: across edge j = (corner j, corner (j + 1) % 3) of face f the other face g of the pair as
        2 g + (s < 0), or -1; vf_ptr [n+1] / vf: per vertex 4 f + corner for every face with a pair it is a corner of,
        ascending.

    An edge with exactly two incident faces is one pair (f, g, s), f < g, s = +1 when the two traverse it in opposite
    directions (consistent winding), else -1; a face with a repeated index gives its edges and is incident to nothing.
    `pairs` [P,3] int64 (host, sorted), E, F, n_pairs, n_boundary (edges of one face), n_nonmanifold (of three or more) and
    n_flipped (pairs with s = -1) are host values."""

    def __init__(self, n, device, tables, pairs, n_boundary, n_nonmanifold):
        self.n, self.device, self.pairs = n, device, pairs
        self.host = tables
        for k, v in tables.items():
            setattr(self, k, v.to(device))
        self.E, self.F, self.n_pairs = int(tables['edges'].shape[0]), int(tables['faces'].shape[0]), int(pairs.shape[0])
        self.n_boundary, self.n_nonmanifold = n_boundary, n_nonmanifold
        self.n_flipped = int((pairs[:, 2] < 0).sum())


def _csr(rows, values, n):
    """(ptr [n+1] int32, values int32 ordered by (row, value)) of host int64 rows / values."""
    order = torch.argsort(rows * (int(values.max()) + 1 if values.numel() else 1) + values)
    ptr = torch.zeros(n + 1, dtype=torch.long)
    ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return ptr.int(), values[order].int()


def _unique_runs(sorted_keys):
    """(values, first index, length) of the runs of equal values of a sorted host vector."""
    if sorted_keys.numel() == 0:
        z = torch.zeros(0, dtype=torch.long)
        return z, z, z
    values, count = torch.unique_consecutive(sorted_keys, return_counts=True)
    return values, torch.cumsum(count, 0) - count, count


def mesh_topology(faces, n, device):
    """The MeshTopology of a face tensor [F,3] over n vertices on `device`, built on the host once per (face content, n,
    device) (keyed by ops.faces_fingerprint, like ops.gcn_graph): a repeated step does no host work and no synchronisation.
    An index outside [0, n) raises ValueError."""
    key = (faces_fingerprint(faces), int(n), str(torch.device(device)))
    hit = _MESH_TOPOLOGIES.get(key)
    if hit is not None:
        return hit
    n = int(n)
    f = faces.detach().cpu().long().reshape(-1, 3)
    F = int(f.shape[0])
    if F and (int(f.max()) >= n or int(f.min()) < 0):
        raise ValueError('faces index vertex %d of a %d-vertex mesh' % (int(f.max()) if int(f.max()) >= n else int(f.min()), n))
    edges = gcn_edges(f)
    E = int(edges.shape[0])
    nbr_ptr, nbr = _csr(torch.cat([edges[:, 0], edges[:, 1]]), torch.cat([edges[:, 1], edges[:, 0]]), n)
    # the directed edges (face, slot) of the faces that count, grouped by their undirected edge
    live = torch.nonzero((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])).flatten()
    fid = live.repeat_interleave(3)
    slot = torch.arange(3).repeat(live.numel())
    a, b = f[fid, slot], f[fid, (slot + 1) % 3]
    ekey = torch.minimum(a, b) * n + torch.maximum(a, b)
    order = torch.argsort(ekey, stable=True)                       # fid ascends already: within an edge the faces stay in order
    ekey, fid, slot, fwd = ekey[order], fid[order], slot[order], (a < b)[order]
    _, start, count = _unique_runs(ekey)
    n_boundary, n_nonmanifold = int((count == 1).sum()), int((count >= 3).sum())
    first = start[count == 2]
    pf, pg = fid[first], fid[first + 1]
    ps = torch.where(fwd[first] != fwd[first + 1], 1, -1)
    adj = torch.full((F, 3), -1, dtype=torch.long)
    adj[pf, slot[first]] = 2 * pg + (ps < 0).long()
    adj[pg, slot[first + 1]] = 2 * pf + (ps < 0).long()
    pairs = torch.stack([pf, pg, ps], 1) if first.numel() else torch.zeros((0, 3), dtype=torch.long)
    if pairs.shape[0]:
        pairs = pairs[torch.argsort(pf * F + pg)]
    paired = torch.nonzero((adj >= 0).any(1)).flatten()
    pid = paired.repeat_interleave(3)
    corner = torch.arange(3).repeat(paired.numel())
    vf_ptr, vf = _csr(f[pid, corner], 4 * pid + corner, n)
    tables = dict(faces=f.int().contiguous(), edges=edges.int().contiguous(), nbr_ptr=nbr_ptr, nbr=nbr, adj=adj.int(),
                  vf_ptr=vf_ptr, vf=vf)
    if len(_MESH_TOPOLOGIES) > 64:
        _MESH_TOPOLOGIES.clear()
    hit = _MESH_TOPOLOGIES[key] = MeshTopology(n, torch.device(device), tables, pairs, n_boundary, n_nonmanifold)
    return hit


def meshreg_terms_mask(terms):
    """The `terms` bit mask of vpn_meshreg_* of an iterable of names out of 'edge', 'lap', 'normal'."""
    if isinstance(terms, str):
        terms = (terms,)
    mask = 0
    for t in terms:
        if t not in MESHREG_TERMS:
            raise ValueError('mesh_regularizers: unknown term %r (terms are %s)' % (t, ', '.join(MESHREG_TERMS)))
        mask |= MESHREG_TERMS[t]
    return mask


def _meshreg_check(verts, faces, edge_target):
    """The contract of mesh_regularizers, from shapes and dtypes alone: ValueError before any launch."""
    if not isinstance(verts, torch.Tensor) or verts.dim() != 3 or verts.shape[2] != 3 or min(verts.shape) < 1:
        raise ValueError('mesh_regularizers: verts must be [B,V,3], got %r' % (tuple(getattr(verts, 'shape', ())),))
    if verts.dtype != torch.float32:
        raise ValueError('mesh_regularizers: verts must be float32, got %s' % verts.dtype)
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError('mesh_regularizers: faces must be [F,3], one topology for the batch, got %r'
                         % (tuple(getattr(faces, 'shape', ())),))
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError('mesh_regularizers: faces must be int32 or int64, got %s' % faces.dtype)
    if not (isinstance(edge_target, (int, float)) and 0.0 <= float(edge_target) < math.inf):
        raise ValueError('mesh_regularizers: edge_target must be a finite number >= 0, got %r' % (edge_target,))
    B, V = int(verts.shape[0]), int(verts.shape[1])
    if B > 65535 or max(V, int(faces.shape[0])) > MESHREG_MAX_ITEMS:
        raise ValueError('mesh_regularizers: at most 65535 samples and %d vertices or faces, got B = %d, V = %d, F = %d'
                         % (MESHREG_MAX_ITEMS, B, V, int(faces.shape[0])))
    return B, V


class MeshRegFunction(Function):
    """out [3] = (edge, lap, normal) of verts [B,V,3] over a MeshTopology (see vpn_meshreg_fwd in include/vpn_hip.h for the
    definitions): two launches forward, one gather launch backward, no atomics, bit-equal from run to run.  The gradient goes
    to verts only and is first order (once_differentiable); the upstream gradient [3] stays on the device, so weights
    applied in torch never cross to the host.  When verts needs no gradient nothing is saved and nothing runs backward."""

    @staticmethod
    def forward(ctx, verts, topo, edge_target, terms):
        if verts.dim() != 3 or tuple(verts.shape[1:]) != (topo.n, 3) or verts.shape[0] < 1 or verts.dtype != torch.float32:
            raise ValueError('MeshRegFunction: verts must be float32 [B,%d,3] for this topology, got %s %r'
                             % (topo.n, verts.dtype, tuple(verts.shape)))
        if not 0 <= int(terms) <= 7 or not 0.0 <= float(edge_target) < math.inf:
            raise ValueError('MeshRegFunction: terms is a mask of 0..7 and edge_target a finite number >= 0, got %r, %r'
                             % (terms, edge_target))
        verts = _f32c(verts)
        B, V = int(verts.shape[0]), int(verts.shape[1])
        dev = verts.device
        need = ctx.needs_input_grad[0]
        delta = torch.empty_like(verts) if need and terms & MESHREG_TERMS['lap'] else None
        normals = torch.empty((B, topo.F, 3), dtype=torch.float32, device=dev) if need and terms & MESHREG_TERMS['normal'] else None
        ws = _workspace('vpn_meshreg_workspace', B, V, topo.E, topo.F, dev=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        _lib.call('vpn_meshreg_fwd', verts, topo.faces, topo.edges, topo.nbr_ptr, topo.nbr, topo.adj, B, V, topo.E, topo.F,
                  topo.n_pairs, float(edge_target), terms, ws, delta, normals, out, _lib.stream())
        if need:
            ctx.save_for_backward(verts, delta, normals)
            ctx.meta = (topo, float(edge_target), terms)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        verts, delta, normals = ctx.saved_tensors
        topo, edge_target, terms = ctx.meta
        B, V = int(verts.shape[0]), int(verts.shape[1])
        dverts = torch.empty_like(verts)
        _lib.call('vpn_meshreg_bwd', _f32c(g), verts, delta, normals, topo.faces, topo.nbr_ptr, topo.nbr, topo.vf_ptr, topo.vf,
                  topo.adj, B, V, topo.E, topo.F, topo.n_pairs, edge_target, terms, dverts, _lib.stream())
        return dverts, None, None, None


def mesh_regularizers(verts, faces, edge_target=0.0, terms=('edge', 'lap', 'normal')):
    """[3] = (edge, lap, normal) of verts [B,V,3] fp32 over faces [F,3], one topology for the batch (MeshRegFunction):

        edge    mean over (b, e) of (|v_a - v_b| - edge_target)^2 over the unique edges
        lap     mean over (b, i) of |mean of i's neighbours - v_i|^2 (uniform weights, squared: smooth at 0)
        normal  mean over (b, pair) of 1 - cos of the normals of two faces that share an edge

    A term absent from `terms` is not computed: its value is 0 and it has no gradient.  Weight the three in torch.  To hold
    a deformation to the SHAPE it started from rather than to flatness, pass the offsets: the Laplacian is linear, so
    mesh_regularizers(pred - verts, faces, terms=('lap',))[1] is the mean of |delta(pred) - delta(verts)|^2.  The topology
    tables are built once per face content (ops.mesh_topology).  Anything outside the contract raises ValueError before
    any launch; CPU tensors have no path."""
    mask = meshreg_terms_mask(terms)
    _, V = _meshreg_check(verts, faces, edge_target)
    topo = mesh_topology(faces, V, verts.device)
    return MeshRegFunction.apply(verts, topo, float(edge_target), mask)


# ---- point-to-surface distance (csrc/pointmesh.hip): points to triangles, both ways

POINTMESH_MAX_ITEMS = _H['VPN_POINTMESH_MAX_ITEMS']
_MESH_INCIDENCES = {}


class MeshIncidence:
    """Which (face, corner) every vertex of one face list over n vertices is, int32 tables on one device: faces [F,3];
    vf_ptr [n+1] / vf [3F]: per vertex 4 f + corner of EVERY face it is a corner of (a face with a repeated index counts
    once per corner; MeshTopology.vf lists only faces with a pair), ascending.  `host` keeps the host copies."""

    def __init__(self, n, device, tables):
        self.n, self.device, self.host = n, device, tables
        for k, v in tables.items():
            setattr(self, k, v.to(device))
        self.F = int(tables['faces'].shape[0])


def mesh_incidence(faces, n, device):
    """The MeshIncidence of a face tensor [F,3] over n vertices on `device`, built on the host once per (face content, n,
    device) (keyed by ops.faces_fingerprint, like ops.mesh_topology): a repeated step does no host work and no
    synchronisation.  An index outside [0, n) raises ValueError."""
    key = (faces_fingerprint(faces), int(n), str(torch.device(device)))
    hit = _MESH_INCIDENCES.get(key)
    if hit is not None:
        return hit
    n = int(n)
    f = faces.detach().cpu().long().reshape(-1, 3)
    F = int(f.shape[0])
    if F and (int(f.max()) >= n or int(f.min()) < 0):
        raise ValueError('faces index vertex %d of a %d-vertex mesh' % (int(f.max()) if int(f.max()) >= n else int(f.min()), n))
    fid = torch.arange(F).repeat_interleave(3)
    corner = torch.arange(3).repeat(F)
    vf_ptr, vf = _csr(f.reshape(-1), 4 * fid + corner, n)
    tables = dict(faces=f.int().contiguous(), vf_ptr=vf_ptr, vf=vf)
    if len(_MESH_INCIDENCES) > 64:
        _MESH_INCIDENCES.clear()
    hit = _MESH_INCIDENCES[key] = MeshIncidence(n, torch.device(device), tables)
    return hit


def _pointmesh_check(name, points, verts, faces):
    """The contract of point_mesh_distance / point_mesh_nearest, from shapes and dtypes alone: ValueError before any launch."""
    for what, t, dim in (('points', points, 'P'), ('verts', verts, 'V')):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != 3 or min(t.shape) < 1:
            raise ValueError('%s: %s must be [B,%s,3], got %r' % (name, what, dim, tuple(getattr(t, 'shape', ()))))
        if t.dtype != torch.float32:
            raise ValueError('%s: %s must be float32, got %s' % (name, what, t.dtype))
    if points.shape[0] != verts.shape[0]:
        raise ValueError('%s: points and verts must have one batch size, got %d and %d' % (name, points.shape[0], verts.shape[0]))
    if points.device != verts.device:
        raise ValueError('%s: points and verts must be on one device, got %s and %s' % (name, points.device, verts.device))
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError('%s: faces must be [F,3], one topology for the batch, got %r' % (name, tuple(getattr(faces, 'shape', ()))))
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError('%s: faces must be int32 or int64, got %s' % (name, faces.dtype))
    B, P, V, F = int(points.shape[0]), int(points.shape[1]), int(verts.shape[1]), int(faces.shape[0])
    if B > 65535 or max(P, V, F) > POINTMESH_MAX_ITEMS:
        raise ValueError('%s: at most 65535 samples and %d points, vertices or faces, got B = %d, P = %d, V = %d, F = %d'
                         % (name, POINTMESH_MAX_ITEMS, B, P, V, F))
    return B, P, V, F


def _pointmesh_fwd(points, verts, inc, per_query, want_out):
    """One vpn_pointmesh_fwd: (dist_p, face_of_point, dist_f, point_of_face) or Nones, and out [2] or None."""
    B, P, V, dev = int(points.shape[0]), int(points.shape[1]), int(verts.shape[1]), points.device
    ws = _workspace('vpn_pointmesh_workspace', B, P, V, inc.F, dev=dev)
    dist_p = dist_f = fop = pof = None
    if per_query & 1:
        fop = torch.empty((B, P), dtype=torch.int32, device=dev)
        pof = torch.empty((B, inc.F), dtype=torch.int32, device=dev)
    if per_query & 2:
        dist_p = torch.empty((B, P), dtype=torch.float32, device=dev)
        dist_f = torch.empty((B, inc.F), dtype=torch.float32, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev) if want_out else None
    _lib.call('vpn_pointmesh_fwd', points, verts, inc.faces, B, P, V, inc.F, ws, ws.numel() * 4, dist_p, fop, dist_f, pof, out,
              _lib.stream())
    return (dist_p, fop, dist_f, pof), out


class PointMeshFunction(Function):
    """out [2] = (mean over (b, i) of dist_p, mean over (b, f) of dist_f) of points [B,P,3] against the triangles of verts
    [B,V,3] over a MeshIncidence (see vpn_pointmesh_fwd in include/vpn_hip.h for the definitions): four launches forward,
    at most three backward, no atomics, bit-equal from run to run.  The gradient goes to points and to verts, each only when
    needed, and is first order (once_differentiable); the upstream gradient [2] stays on the device.  Only the two index
    tensors are saved; when neither input needs a gradient nothing is saved and the indices are not written."""

    @staticmethod
    def forward(ctx, points, verts, inc):
        if (points.dim() != 3 or verts.dim() != 3 or points.shape[2] != 3 or tuple(verts.shape[1:]) != (inc.n, 3)
                or points.shape[0] != verts.shape[0] or min(points.shape) < 1 or points.dtype != torch.float32
                or verts.dtype != torch.float32):
            raise ValueError('PointMeshFunction: points must be float32 [B,P,3] and verts float32 [B,%d,3] for this incidence, '
                             'got %s %r and %s %r' % (inc.n, points.dtype, tuple(points.shape), verts.dtype, tuple(verts.shape)))
        points, verts = _f32c(points), _f32c(verts)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        (_, fop, _, pof), out = _pointmesh_fwd(points, verts, inc, 1 if need else 0, True)
        if need:
            ctx.save_for_backward(points, verts, fop, pof)
            ctx.inc = inc
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        need_p, need_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_p or need_v):
            return None, None, None
        points, verts, fop, pof = ctx.saved_tensors
        inc = ctx.inc
        B, P, V = int(points.shape[0]), int(points.shape[1]), int(verts.shape[1])
        dpoints = torch.empty_like(points) if need_p else None
        dverts = torch.empty_like(verts) if need_v else None
        ws = _workspace('vpn_pointmesh_workspace', B, P, V, inc.F, dev=points.device) if need_v else None
        _lib.call('vpn_pointmesh_bwd', _f32c(g), points, verts, inc.faces, fop, pof, inc.vf_ptr, inc.vf, B, P, V, inc.F, ws,
                  ws.numel() * 4 if need_v else 0, dpoints, dverts, _lib.stream())
        return dpoints, dverts, None


def point_mesh_distance(points, verts, faces):
    """[2] = (point term, face term) of points [B,P,3] fp32 against the surface of verts [B,V,3] fp32 over faces [F,3], one
    topology for the batch (PointMeshFunction; the point_mesh_face_distance of PyTorch3D, squared distances):

        point term  mean over (b, i) of the squared distance from point i to its nearest triangle
        face term   mean over (b, f) of the squared distance from triangle f to its nearest point

    A triangle without area is the segment or point it degenerates to.  Weight the two in torch.  Differentiable to points
    and to verts.  The incidence table is built once per face content (ops.mesh_incidence).  Anything outside the
    contract raises ValueError before any launch; CPU tensors have no path."""
    _, _, V, _ = _pointmesh_check('point_mesh_distance', points, verts, faces)
    inc = mesh_incidence(faces, V, verts.device)
    return PointMeshFunction.apply(points, verts, inc)


def point_mesh_nearest(points, verts, faces):
    """(dist_p [B,P], face_of_point [B,P] int32, dist_f [B,F], point_of_face [B,F] int32): per point the squared distance to
    and the index of its nearest triangle, per triangle of its nearest point, the lowest index on ties (the forward of
    point_mesh_distance).  No autograd node: for tests, evaluation scripts and visual debugging."""
    _, _, V, _ = _pointmesh_check('point_mesh_nearest', points, verts, faces)
    inc = mesh_incidence(faces, V, verts.device)
    with torch.no_grad():
        per_query, _ = _pointmesh_fwd(_f32c(points.detach()), _f32c(verts.detach()), inc, 3, False)
    return per_query


# ---- the batch augmentation stage (csrc/augment.hip).  Plain functions: the augmented tensors are data, nothing here is
# differentiable and no output requires grad.

def _augment_is_data(*tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise RuntimeError('augmentation arguments are dataset values here (train.py:232-237); gradients with respect '
                               'to them are not implemented')


def partner_indices(indices, B, device):
    """The partner of each sample as the contiguous int32 device tensor the kernels read.  A host tensor or list is
    checked against [0, B) here and uploaded from pinned memory without blocking (no synchronisation); a device tensor
    is converted at most (the kernels read an entry outside [0, B) as the sample itself)."""
    if isinstance(indices, torch.Tensor) and indices.is_cuda:
        assert indices.numel() == B
        return indices.reshape(B).to(torch.int32).contiguous()
    host = torch.as_tensor(indices).reshape(-1).to(torch.int32)
    if host.numel() != B or (B and (int(host.min()) < 0 or int(host.max()) >= B)):
        raise ValueError('indices must name %d partners in [0, %d)' % (B, B))
    return host.pin_memory().to(device, non_blocking=True)


def cutmix_points(points, indices, cut, seed, sample_base=0, n_out=None):
    """vpn_cutmix_points: points [B,N,3], indices [B] int32 on the device (None: each sample with itself), cut a float or
    a [B] fp32 device tensor -> (out [B,n_out,3], src [B,n_out] int32, count [B] int32); n_out defaults to N."""
    _augment_is_data(points, cut)
    points = _f32c(points.detach())
    B, N, _ = points.shape
    n_out = N if n_out is None else int(n_out)
    dev = points.device
    cut_t = None
    if isinstance(cut, torch.Tensor):
        cut_t = _f32c(cut.detach()).reshape(-1)
        assert cut_t.numel() == B
        cut = 0.0
    out = torch.empty((B, n_out, 3), dtype=torch.float32, device=dev)
    src = torch.empty((B, n_out), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.call('vpn_cutmix_points', points, indices, cut_t, float(cut), int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_base), B, N,
              n_out, out, src, count, _lib.stream())
    return out, src, count


def cutmix_images(rgbs, silhouettes, indices, cut_index):
    """vpn_cutmix_images: both images in one launch, out of place (silhouettes may be None)."""
    _augment_is_data(rgbs, silhouettes)
    rgbs = _f32c(rgbs.detach())
    B, Ca, H, W = rgbs.shape
    out_a = torch.empty_like(rgbs)
    Cb, out_b = 0, None
    if silhouettes is not None:
        silhouettes = _f32c(silhouettes.detach())
        assert silhouettes.size(0) == B and silhouettes.shape[2:] == rgbs.shape[2:]
        Cb = silhouettes.size(1)
        out_b = torch.empty_like(silhouettes)
    _lib.call('vpn_cutmix_images', rgbs, silhouettes, indices, B, Ca, Cb, H, W, int(cut_index), out_a, out_b, _lib.stream())
    return out_a, out_b


def mixup_points(points, indices, ratio, eps=0.005, iters=100, max_group=None):
    """point_mixup.py:24-40 for the whole batch: gather of the partner clouds, ONE auction over the B pairs, the
    interpolation through its assignment -> (mixed [B,n,3], dist [B,n], assignment [B,n] int32)."""
    _augment_is_data(points)
    points = _f32c(points.detach())
    B, n, _ = points.shape
    dev = points.device
    partner = torch.empty_like(points)
    _lib.call('vpn_mixup_gather', points, indices, B, n, partner, _lib.stream())
    dist, assignment, _ = _auction(points, partner, eps, iters, _emd_group(max_group), _lib.stream())
    ratio = float(ratio)
    mixed = torch.empty_like(points)
    # (1 - r) and r as torch rounds the two Python doubles of point_mixup.py:36 to fp32
    _lib.call('vpn_mixup_lerp', points, partner, assignment, B, n, 1.0 - ratio, ratio, mixed, _lib.stream())
    return mixed, dist, assignment


# ---- cloud -> mesh of one topology (csrc/reconstruct.hip): what point_mixup.py:43-55 does through open3d
# ball pivoting and V-HACD on the host, replaced by a clustering and support polytopes on the device.  Data, like the rest
# of the augmentation stage.

def cluster_points(points, hull_num, iters=8):
    """vpn_cluster_points: points [B,n,3] -> (labels [B,n] int32, centres [B,H,3], counts [B,H] int32): farthest-point
    seeds and `iters` Lloyd rounds with exact integer means, one workgroup per sample (include/vpn_hip.h)."""
    _augment_is_data(points)
    points = _f32c(points.detach())
    if points.dim() != 3 or points.size(2) != 3:
        raise ValueError('points must be [B,n,3], got %s' % (tuple(points.shape),))
    B, n, _ = points.shape
    H = int(hull_num)
    dev = points.device
    labels = torch.empty((B, n), dtype=torch.int32, device=dev)
    centres = torch.empty((B, H, 3), dtype=torch.float32, device=dev)
    counts = torch.empty((B, H), dtype=torch.int32, device=dev)
    _lib.call('vpn_cluster_points', points, B, n, H, int(iters), labels, centres, counts, _lib.stream())
    return labels, centres, counts


def support_hulls(points, labels, centres, dirs):
    """vpn_support_hulls: points [B,n,3], labels [B,n] int32, centres [B,H,3], dirs [D,3] -> (verts [B,H*D,3], support
    [B,H*D] int32): vertex (h,d) is the member of cluster h farthest along dirs[d] (include/vpn_hip.h)."""
    _augment_is_data(points, centres, dirs)
    if (points.dim() != 3 or points.size(2) != 3 or centres.dim() != 3 or centres.size(2) != 3 or centres.size(0) != points.size(0)
            or dirs.dim() != 2 or dirs.size(1) != 3 or labels.dtype != torch.int32 or tuple(labels.shape) != tuple(points.shape[:2])):
        raise ValueError('support_hulls: points [B,n,3], labels [B,n] int32, centres [B,H,3], dirs [D,3] expected, got %s %s %s %s %s'
                         % (tuple(points.shape), labels.dtype, tuple(labels.shape), tuple(centres.shape), tuple(dirs.shape)))
    points, centres, dirs = _f32c(points.detach()), _f32c(centres.detach()), _f32c(dirs.detach())
    B, n, _ = points.shape
    H, D = centres.size(1), dirs.size(0)
    dev = points.device
    verts = torch.empty((B, H * D, 3), dtype=torch.float32, device=dev)
    support = torch.empty((B, H * D), dtype=torch.int32, device=dev)
    _lib.call('vpn_support_hulls', points, labels.contiguous(), centres, dirs, B, n, H, D, verts, support, _lib.stream())
    return verts, support


_HULL_TEMPLATES = {}


def hull_template(hull_num, device, template=None):
    """(dirs [D,3] float32, faces [H*Ft,3] int32) of `hull_num` hulls on `device`: the template's vertices, normalised,
    and its faces repeated with a per-hull vertex offset.  template: (vertices [D,3], faces [Ft,3]) host tensors, default
    meshing.uv_sphere().  Uploaded once per (template, hull_num, device) through pinned memory without blocking
    (const_tensor style): later calls, also inside a HIP-graph capture, touch neither the host nor the copy engine."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    H = int(hull_num)
    if template is None:
        tkey = 'uv_sphere'
    else:
        tv, tf = (torch.as_tensor(t).detach().cpu().contiguous() for t in template)
        tkey = (tuple(tv.shape), hash(tv.numpy().tobytes()), tuple(tf.shape), hash(tf.numpy().tobytes()))
    key = (tkey, H, str(device))
    hit = _HULL_TEMPLATES.get(key)
    if hit is None:
        if template is None:
            from .modules.meshing import uv_sphere
            tv, tf = uv_sphere()
        tv = tv.to(torch.float32)
        if tv.dim() != 2 or tv.size(1) != 3 or tf.dim() != 2 or tf.size(1) != 3:
            raise ValueError('template must be (vertices [D,3], faces [Ft,3])')
        D = tv.size(0)
        if tf.numel() and (int(tf.min()) < 0 or int(tf.max()) >= D):
            raise ValueError('template faces index outside its %d vertices' % D)
        dirs = tv / tv.norm(dim=1, keepdim=True)
        faces = torch.cat([tf.long() + h * D for h in range(H)]).to(torch.int32)
        if len(_HULL_TEMPLATES) > 64:
            _HULL_TEMPLATES.clear()
        up = (lambda t: t.contiguous().pin_memory().to(device, non_blocking=True)) if device.type == 'cuda' else (lambda t: t.contiguous())
        hit = (up(dirs), up(faces))
        faces_remember(hit[1], ('hulls', tkey, H))        # the content key without a device read (mesh_batches, gcn_graph)
        _HULL_TEMPLATES[key] = hit
    return hit


def hull_meshes(points, hull_num, iters=8, template=None):
    """Cloud -> mesh of one topology for the whole batch, two launches, no host synchronisation: points [B,n,3] ->
    (verts [B,H*D,3], faces [H*Ft,3] int32 shared by the samples, labels [B,n] int32, support [B,H*D] int32).  Hull h of
    sample b is the template (default meshing.uv_sphere(): D = 128, Ft = 252) with vertex d moved to the member of cluster
    h farthest along the template's direction d: an inner approximation of the cluster's convex hull with every vertex on
    it.  Faces between coinciding vertices have zero area; the raster and the sampler ignore them."""
    _augment_is_data(points)
    dirs, faces = hull_template(hull_num, points.device, template)
    labels, centres, _counts = cluster_points(points, hull_num, iters)
    verts, support = support_hulls(points, labels, centres, dirs)
    return verts, faces, labels, support


def sample_meshes(verts, faces, n, seed, mesh_base=0):
    """n area-weighted uniform surface points on each of B meshes of one topology as data (vpn_mesh_sample_fwd, one launch
    pair, no autograd node): verts [B,P,3], faces [F,3] int32 -> (points [B,n,3], face index [B,n] int32, barycentric weights
    [B,n,3]); points[b,i] = sum_k bary[b,i,k] * verts[b, faces[face[b,i], k]].  Draws: Philox(seed; mesh_base + b, point)."""
    _augment_is_data(verts)
    verts = _f32c(verts.detach())
    B, P, _ = verts.shape
    F = faces.shape[0]
    assert faces.dtype == torch.int32 and faces.is_cuda and faces.is_contiguous()
    dev = verts.device
    n = int(n)
    cdf = torch.empty((B, F), dtype=torch.float32, device=dev)
    points = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    fidx = torch.empty((B, n), dtype=torch.int32, device=dev)
    bary = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    _lib.call('vpn_mesh_sample_fwd', verts, faces, None, int(seed) & 0xFFFFFFFFFFFFFFFF, int(mesh_base), B, P, F, n, cdf, points,
              fidx, bary, _lib.stream())
    return points, fidx, bary


# ---- the middle of the ACD-mix stage (csrc/acdmix.hip): acd.py:31-77,114-119 and the merge of
# generate.py:140-148, the boolean union replaced by a sampled union surface.  Data, like the rest of the augmentation stage.

def _draw_tensor(name, value, shape, dtype, dev):
    """A draw of the stage as the contiguous device tensor the kernels read: a device tensor is checked and converted at
    most; host values are uploaded from pinned memory without blocking."""
    if isinstance(value, torch.Tensor) and value.is_cuda:
        _augment_is_data(value)
        if tuple(value.shape) != tuple(shape):
            raise ValueError('%s must be %s, got %s' % (name, tuple(shape), tuple(value.shape)))
        return value.detach().to(dtype).contiguous()
    host = torch.as_tensor(value).detach().to(dtype)
    if tuple(host.shape) != tuple(shape):
        raise ValueError('%s must be %s, got %s' % (name, tuple(shape), tuple(host.shape)))
    host = host.contiguous()
    return host.pin_memory().to(dev, non_blocking=True) if torch.device(dev).type == 'cuda' else host


def hull_augment(verts, group, coin, u_num, scale, turn, shift, u_hull):
    """vpn_hull_augment: verts [S,G,D,3], group [G] (the object of each hull, 0 .. O-1), the draws per (sample, object)
    coin / u_num / scale / turn / shift [S,O] and the keys u_hull [S,G] (host values or device tensors) -> (out [S,G,D,3],
    keep [S,G] int32): cut-out, scale, quarter turn about z, shift along y (include/vpn_hip.h)."""
    _augment_is_data(verts)
    if verts.dim() != 4 or verts.size(3) != 3:
        raise ValueError('verts must be [S,G,D,3], got %s' % (tuple(verts.shape),))
    verts = _f32c(verts.detach())
    S, G, D, _ = verts.shape
    dev = verts.device
    group = _draw_tensor('group', group, (G,), torch.int32, dev)
    coin_t = torch.as_tensor(coin)
    if coin_t.dim() != 2 or coin_t.size(0) != S:
        raise ValueError('coin must be [S,O] with S = %d, got %s' % (S, tuple(coin_t.shape)))
    O = coin_t.size(1)
    coin, turn = (_draw_tensor(n, v, (S, O), torch.int32, dev) for n, v in (('coin', coin_t), ('turn', turn)))
    u_num, scale, shift = (_draw_tensor(n, v, (S, O), torch.float32, dev) for n, v in (('u_num', u_num), ('scale', scale), ('shift', shift)))
    u_hull = _draw_tensor('u_hull', u_hull, (S, G), torch.float32, dev)
    out = torch.empty_like(verts)
    keep = torch.empty((S, G), dtype=torch.int32, device=dev)
    _lib.call('vpn_hull_augment', verts, group, coin, u_num, scale, turn, shift, u_hull, S, G, D, O, out, keep, _lib.stream())
    return out, keep


def union_surface(verts, keep, dirs, cand, cand_hull, n_out, margin=1e-3):
    """vpn_union_surface: verts [S,G,D,3], keep [S,G] int32, dirs [D,3], candidates cand [S,nc,3] with the hull each was
    drawn on, cand_hull [S,nc] int32 -> (support [S,G,D], outside [S,nc] int32, points [S,n_out,3], src [S,n_out] int32,
    count [S] int32): the candidates that lie inside no other kept hull, in candidate order, repeated cyclically up to
    n_out (include/vpn_hip.h)."""
    _augment_is_data(verts, dirs, cand)
    if (verts.dim() != 4 or verts.size(3) != 3 or dirs.dim() != 2 or tuple(dirs.shape) != (verts.size(2), 3) or cand.dim() != 3
            or cand.size(2) != 3 or cand.size(0) != verts.size(0) or keep.dtype != torch.int32 or tuple(keep.shape) != tuple(verts.shape[:2])
            or cand_hull.dtype != torch.int32 or tuple(cand_hull.shape) != tuple(cand.shape[:2])):
        raise ValueError('union_surface: verts [S,G,D,3], keep [S,G] int32, dirs [D,3], cand [S,nc,3], cand_hull [S,nc] int32 expected, '
                         'got %s %s %s %s %s %s %s' % (tuple(verts.shape), keep.dtype, tuple(keep.shape), tuple(dirs.shape),
                                                     tuple(cand.shape), cand_hull.dtype, tuple(cand_hull.shape)))
    verts, dirs, cand = _f32c(verts.detach()), _f32c(dirs.detach()), _f32c(cand.detach())
    S, G, D, _ = verts.shape
    nc, n_out = cand.size(1), int(n_out)
    dev = verts.device
    support = torch.empty((S, G, D), dtype=torch.float32, device=dev)
    outside = torch.empty((S, nc), dtype=torch.int32, device=dev)
    points = torch.empty((S, n_out, 3), dtype=torch.float32, device=dev)
    src = torch.empty((S, n_out), dtype=torch.int32, device=dev)
    count = torch.empty((S,), dtype=torch.int32, device=dev)
    _lib.call('vpn_union_surface', verts, keep.contiguous(), dirs, cand, cand_hull.contiguous(), S, G, D, nc, n_out, float(margin),
              support, outside, points, src, count, _lib.stream())
    return support, outside, points, src, count


def acd_mix_points(hulls1, hulls2, coin, u_num, scale, turn, shift, u_hull, n_out, seed, mesh_base=0, *, n_cand=None,
                   margin=1e-3, template=None):
    """The hulls of two objects -> a cloud on the surface of their augmented union (generate.py:140-146): hulls1 / hulls2
    [S,H,D,3] (ops.hull_meshes' vertices of each object, D the template's), the draws of hull_augment with O = 2 and G = 2 H
    (object 1's hulls first).  Three steps, four launches, no host synchronisation: hull_augment; n_cand (default 2 n_out)
    area-weighted candidates on the merged hulls by sample_meshes (Philox(seed; mesh_base + s, point); the hull of a
    candidate is its face // Ft); union_surface.  -> (points [S,n_out,3], count [S] int32, parts), parts a dict: hulls
    (augmented, [S,G,D,3]), keep, faces, dirs, cand, cand_hull, support, outside, src."""
    _augment_is_data(hulls1, hulls2)
    if hulls1.dim() != 4 or hulls1.size(3) != 3 or tuple(hulls1.shape) != tuple(hulls2.shape):
        raise ValueError('hulls1 and hulls2 must both be [S,H,D,3], got %s and %s' % (tuple(hulls1.shape), tuple(hulls2.shape)))
    S, H, D, _ = hulls1.shape
    G = 2 * H
    dev = hulls1.device
    dirs, faces = hull_template(G, dev, template)
    if dirs.size(0) != D:
        raise ValueError('the hulls have %d vertices each, the template %d' % (D, dirs.size(0)))
    group = const_tensor((0,) * H + (1,) * H, torch.int32, dev)
    merged = torch.cat([_f32c(hulls1.detach()), _f32c(hulls2.detach())], 1)
    hulls, keep = hull_augment(merged, group, coin, u_num, scale, turn, shift, u_hull)
    n_out = int(n_out)
    nc = 2 * n_out if n_cand is None else int(n_cand)
    cand, face_idx, _bary = sample_meshes(hulls.reshape(S, G * D, 3), faces, nc, seed, mesh_base)
    cand_hull = torch.div(face_idx, faces.size(0) // G, rounding_mode='floor')
    support, outside, points, src, count = union_surface(hulls, keep, dirs, cand, cand_hull, n_out, margin)
    return points, count, dict(hulls=hulls, keep=keep, faces=faces, dirs=dirs, cand=cand, cand_hull=cand_hull, support=support,
                               outside=outside, src=src)


# ---- the evaluation stage (csrc/evaluate.hip; test.py:68-135, test_gcn.py:115-178).  Plain functions: nothing is
# differentiable, the metrics are reported values.

def eval_state(C, device):
    """A zeroed state of the evaluation stage for C classes (include/vpn_hip.h, vpn_eval_accumulate): one float64 tensor of
    5 + 3 C elements, the last 2 + C of which hold int64 bit patterns (eval_state_fields splits it)."""
    nbytes = _lib.lib().vpn_eval_state_size(int(C))
    if nbytes == 0:
        raise ValueError('the evaluation state needs at least one class')
    return torch.zeros((nbytes // 8,), dtype=torch.float64, device=device)


def eval_state_fields(state, C):
    """Views of a state tensor (any device): (sums float64 [3 + 2 C], counts int64 [2 + C])."""
    if state.dtype != torch.float64 or state.numel() != 5 + 3 * C:
        raise ValueError('not an evaluation state of %d classes' % C)
    return state[:3 + 2 * C], state[3 + 2 * C:].view(torch.int64)


def eval_step(predict_points, gt_points, class_index, state, C, *, emd=True, eps=0.005, iters=50, w1=None, w2=None,
              cd_scale=1.0, max_group=None):
    """One evaluation batch (test_gcn.py:142-152; emd=False: test.py:101-108): the Chamfer scan on the current stream, the
    auction beside it on the side stream (EMD_SIDE_STREAM, the group rule of the training step), joined in front of ONE
    vpn_eval_accumulate launch that writes the per-sample metrics and adds the batch to `state` (eval_state).
    class_index: [B] int32 on the device.  No host synchronisation.  -> (cd_b [B], emd_b [B] or None)."""
    from . import config
    p, g = _f32c(predict_points.detach()), _f32c(gt_points.detach())
    B, N, _ = p.shape
    M = g.shape[1]
    if emd and N != M:
        raise ValueError('the EMD metric needs as many predicted as ground-truth points (emd_module.py:36): %d vs %d' % (N, M))
    if g.shape[0] != B or class_index.numel() != B:
        raise ValueError('predicted points, ground-truth points and class indices must agree on the batch size')
    if not (class_index.is_cuda and class_index.dtype == torch.int32):
        raise ValueError('class_index must be an int32 tensor on the device')
    eval_state_fields(state, C)
    dev = p.device
    w1 = config.CD_W1 if w1 is None else w1
    w2 = config.CD_W2 if w2 is None else w2
    emd_dist = _assignment = _ews = side = None
    if emd:
        # launched first, so that its workgroups are placed while the CUs are empty (include/vpn_hip.h, vpn_emd_fwd)
        side = _fork_side(dev) if EMD_SIDE_STREAM else None
        emd_dist, _assignment, _ews = _auction(p, g, eps, iters, _emd_group(max_group),       # alive until the join below
                               ctypes.c_void_p(side.cuda_stream) if side is not None else _lib.stream())
    d1, _, d2, _ = chamfer_nn(p, g)
    if side is not None:
        torch.cuda.current_stream().wait_stream(side)
    cd_b = torch.empty((B,), dtype=torch.float32, device=dev)
    emd_b = torch.empty((B,), dtype=torch.float32, device=dev) if emd else None
    _lib.call('vpn_eval_accumulate', d1, d2, emd_dist, class_index.contiguous(), B, N, M, int(C), float(w1), float(w2),
              float(cd_scale), state, cd_b, emd_b, _lib.stream())
    return cd_b, emd_b


# ---- surface evaluation (csrc/surfeval.hip): Chamfer-L2 / -L1, precision / recall / F-score at distance
# thresholds and normal consistency on points sampled from the predicted surface.  Plain functions: reported values.

SURFEVAL_MAX_THRESHOLDS = _H['VPN_SURFEVAL_MAX_THRESHOLDS']
SURFEVAL_MAX_ITEMS = _H['VPN_SURFEVAL_MAX_ITEMS']


def surfeval_width(T):
    """Columns of a per-sample row: acc2 comp2 acc1 comp1 nc1 nc2, then precision, recall and F-score at each threshold."""
    T = int(T)
    if not 1 <= T <= SURFEVAL_MAX_THRESHOLDS:
        raise ValueError('surface evaluation takes 1 .. %d thresholds, got %d' % (SURFEVAL_MAX_THRESHOLDS, T))
    return 6 + 3 * T


def surfeval_state(C, T, device):
    """A zeroed state of the surface evaluation for C classes and T thresholds (include/vpn_hip.h, vpn_surfeval_accumulate):
    one float64 tensor of (1 + C) W + 3 + C elements, W = 6 + 3 T, the last 3 + C of which hold int64 bit patterns
    (surfeval_state_fields splits it)."""
    surfeval_width(T)
    nbytes = _lib.lib().vpn_surfeval_state_size(int(C), int(T))
    if nbytes == 0:
        raise ValueError('the surface evaluation state needs 1 .. %d classes, got %d' % (SURFEVAL_MAX_ITEMS, int(C)))
    return torch.zeros((nbytes // 8,), dtype=torch.float64, device=device)


def surfeval_state_fields(state, C, T):
    """Views of a state tensor (any device): (sums float64 [(1 + C) W]: total[W] then class_sum[C][W]; counts int64 [3 + C]:
    n_samples, n_batches, n_invalid, class_n[C])."""
    nd = (1 + int(C)) * surfeval_width(T)
    if not isinstance(state, torch.Tensor) or state.dtype != torch.float64 or state.dim() != 1 or state.numel() != nd + 3 + C:
        raise ValueError('not a surface evaluation state of %d classes and %d thresholds' % (C, T))
    return state[:nd], state[nd:].view(torch.int64)


def _normals_check(name, verts, faces, fidx, vdim):
    """Shapes and dtypes of the three tensors of a normals call: ValueError before any launch."""
    want = '[B,P,3]' if vdim == 3 else '[sumP,3]'
    if not isinstance(verts, torch.Tensor) or verts.dim() != vdim or verts.shape[-1] != 3 or min(verts.shape) < 1:
        raise ValueError('%s: verts must be %s, got %r' % (name, want, tuple(getattr(verts, 'shape', ()))))
    if verts.dtype != torch.float32:
        raise ValueError('%s: verts must be float32, got %s' % (name, verts.dtype))
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError('%s: faces must be [F,3], got %r' % (name, tuple(getattr(faces, 'shape', ()))))
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError('%s: faces must be int32 or int64, got %s' % (name, faces.dtype))
    if not isinstance(fidx, torch.Tensor) or fidx.dim() < 2 or min(fidx.shape) < 1:
        raise ValueError('%s: fidx must be [B,n], got %r' % (name, tuple(getattr(fidx, 'shape', ()))))
    if fidx.dtype != torch.int32:
        raise ValueError('%s: fidx must be int32 (what the samplers return), got %s' % (name, fidx.dtype))
    if max(verts.shape[-2], faces.shape[0], fidx.shape[-1]) > SURFEVAL_MAX_ITEMS:
        raise ValueError('%s: at most %d vertices, faces or points' % (name, SURFEVAL_MAX_ITEMS))


def _normals_launch(name, verts, faces, vert_offset, face_offset, fidx2, xforms, sets):
    if not verts.is_cuda:
        raise RuntimeError('vpn_amd operators run on the GPU only (got a %s tensor); there is no CPU path' % verts.device.type)
    dev = verts.device
    B, n = fidx2.shape
    if not fidx2.is_cuda:
        raise ValueError('%s: fidx must be on the device' % name)
    if xforms is not None:
        xforms = _draw_tensor('xforms', xforms, (B, 3, 4), torch.float32, dev)
    out = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    _lib.call('vpn_face_normals_at', verts.detach().contiguous(), faces_i32(faces, dev), vert_offset, face_offset,
              fidx2.contiguous(), xforms, B, n, verts.shape[-2], faces.shape[0], int(sets), out, _lib.stream())
    return out


@torch.no_grad()
def face_normals_at(verts, faces, fidx, xforms=None):
    """The unit normal of the face every sampled point lies on (vpn_face_normals_at, the batched layout): verts [B,P,3]
    fp32, ONE faces [F,3] for the batch (int32 or int64, host or device), fidx [B,n] int32 as sample_meshes returns it ->
    normals [B,n,3].  xforms [B,3,4]: affine rows applied to the corners first; the normal of the mapped triangle needs no
    inverse-transpose.  A map of negative determinant (a reflection) flips the sign, which the normal-consistency metric,
    taking |dot|, does not see.  A face without area, a face index outside [0,F) or a vertex index outside [0,P) gives
    (0,0,0).  One launch, no host synchronisation; everything is validated before it."""
    _normals_check('face_normals_at', verts, faces, fidx, 3)
    if fidx.dim() != 2 or fidx.shape[0] != verts.shape[0]:
        raise ValueError('face_normals_at: fidx must be [B,n] with B = %d, got %r' % (verts.shape[0], tuple(fidx.shape)))
    if verts.shape[0] > 65535:
        raise ValueError('face_normals_at: at most 65535 samples, got %d' % verts.shape[0])
    return _normals_launch('face_normals_at', verts, faces, None, None, fidx, xforms, 1)


@torch.no_grad()
def ragged_face_normals(verts, faces, vert_offset, face_offset, fidx, sets=1, xforms=None):
    """face_normals_at for the packed meshes of a MeshBatch (the ragged layout): verts [sumP,3] fp32, faces [sumF,3] with
    MESH-LOCAL vertex indices, vert_offset / face_offset [S+1] int32 on the device, fidx [S,sets,n] (or [S sets,n]) int32
    mesh-local as ragged_sample(..., return_faces=True) returns it -> normals of the same leading shape + [3].  xforms
    [S,sets,3,4] (or [S sets,3,4]): the map of every (mesh, set), as ragged_sample takes it."""
    _normals_check('ragged_face_normals', verts, faces, fidx, 2)
    sets = int(sets)
    for what, t in (('vert_offset', vert_offset), ('face_offset', face_offset)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or t.numel() < 2:
            raise ValueError('ragged_face_normals: %s must be an int32 tensor of S + 1 entries' % what)
    S = vert_offset.numel() - 1
    if face_offset.numel() != S + 1:
        raise ValueError('ragged_face_normals: the two offset tables must have S + 1 entries each')
    if sets < 1:
        raise ValueError('ragged_face_normals: sets must be positive, got %d' % sets)
    lead = tuple(fidx.shape[:-1])
    if lead not in ((S, sets), (S * sets,)):
        raise ValueError('ragged_face_normals: fidx must be [S,sets,n] = [%d,%d,n], got %r' % (S, sets, tuple(fidx.shape)))
    if S * sets > 65535:
        raise ValueError('ragged_face_normals: at most 65535 samples, got %d' % (S * sets))
    if isinstance(xforms, torch.Tensor) and xforms.dim() == 4:
        if tuple(xforms.shape) != (S, sets, 3, 4):
            raise ValueError('xforms must be %r, got %r' % ((S, sets, 3, 4), tuple(xforms.shape)))
        xforms = xforms.reshape(S * sets, 3, 4)
    if verts.is_cuda and not (vert_offset.is_cuda and face_offset.is_cuda):
        raise ValueError('ragged_face_normals: the offset tables must be on the device')
    out = _normals_launch('ragged_face_normals', verts, faces, vert_offset.contiguous(), face_offset.contiguous(),
                          fidx.reshape(S * sets, fidx.shape[-1]), xforms, sets)
    return out.reshape(lead + (fidx.shape[-1], 3))


@torch.no_grad()
def surfeval_step(predict_points, gt_points, class_index, state, C, thr2, predict_normals=None, gt_normals=None):
    """One batch of the surface evaluation: the nearest-neighbour scan both ways (chamfer_nn, mode 'auto'), then
    vpn_surfeval_accumulate (two launches), which writes the per-sample rows and adds the batch to `state`
    (surfeval_state).  predict_points [B,N,3], gt_points [B,M,3] (N and M may differ); class_index [B] int32 on the device;
    thr2 [T] fp32 on the device: SQUARED distance thresholds; predict_normals [B,N,3] and gt_normals [B,M,3]: unit normals,
    both or neither.  No host synchronisation; everything is validated before a launch.  -> per_sample [B, 6 + 3 T]."""
    for what, t in (('predict_points', predict_points), ('gt_points', gt_points)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != 3 or min(t.shape) < 1:
            raise ValueError('surfeval_step: %s must be [B,n,3], got %r' % (what, tuple(getattr(t, 'shape', ()))))
    B, N, M = predict_points.shape[0], predict_points.shape[1], gt_points.shape[1]
    if gt_points.shape[0] != B or not isinstance(class_index, torch.Tensor) or class_index.numel() != B:
        raise ValueError('predicted points, ground-truth points and class indices must agree on the batch size')
    if B > 65535 or max(N, M) > SURFEVAL_MAX_ITEMS:
        raise ValueError('surfeval_step: at most 65535 samples of %d points, got B = %d, N = %d, M = %d'
                         % (SURFEVAL_MAX_ITEMS, B, N, M))
    if not isinstance(thr2, torch.Tensor) or thr2.dtype != torch.float32 or thr2.dim() != 1:
        raise ValueError('thr2 must be a float32 tensor [T] of squared thresholds')
    T = thr2.numel()
    surfeval_state_fields(state, C, T)
    if (predict_normals is None) != (gt_normals is None):
        raise ValueError('surfeval_step: normals of the prediction and of the ground truth come together or not at all')
    for what, t, pts in (('predict_normals', predict_normals, predict_points), ('gt_normals', gt_normals, gt_points)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.shape == pts.shape and t.dtype == torch.float32):
            raise ValueError('surfeval_step: %s must be float32 %r' % (what, tuple(pts.shape)))
    if class_index.dtype != torch.int32:
        raise ValueError('class_index must be an int32 tensor on the device')
    p, g = _f32c(predict_points.detach()), _f32c(gt_points.detach())
    dev = p.device
    for what, t in (('class_index', class_index), ('thr2', thr2), ('state', state), ('predict_normals', predict_normals),
                    ('gt_normals', gt_normals)):
        if t is not None and t.device != dev:
            raise ValueError('surfeval_step: %s must be on %s, got %s' % (what, dev, t.device))
    if not state.is_contiguous():
        raise ValueError('surfeval_step: the state must be contiguous')
    d1, i1, d2, i2 = chamfer_nn(p, g)
    per_sample = torch.empty((B, 6 + 3 * T), dtype=torch.float32, device=dev)
    _lib.call('vpn_surfeval_accumulate', d1, i1, d2, i2, None if predict_normals is None else predict_normals.detach().contiguous(),
              None if gt_normals is None else gt_normals.detach().contiguous(), thr2.contiguous(), class_index.reshape(-1).contiguous(),
              B, N, M, T, int(C), state, per_sample, _lib.stream())
    return per_sample


# ---- volumetric evaluation (csrc/occupancy.hip): occupancy of a primitive assembly and of a triangle mesh at
# query points, volumetric IoU per sample and its bookkeeping.  Plain functions: reported values, nothing is differentiable.

OCCUPANCY_MAX_ITEMS = _H['VPN_OCCUPANCY_MAX_ITEMS']
VOLIOU_WIDTH = _H['VPN_VOLIOU_WIDTH']
VOLIOU_COLUMNS = ('iou', 'precision', 'recall', 'vol_pred', 'vol_gt')


def grid_queries(R, lo=-0.5, hi=0.5, device=None):
    """The R^3 cell centres of the cube [lo, hi]^3 as fp32 [R^3,3]: index (iz R + iy) R + ix, coordinate lo + (i + 0.5) (hi -
    lo) / R formed in float64 and rounded once.  device None: a host tensor."""
    R, lo, hi = int(R), float(lo), float(hi)
    if R < 1 or R ** 3 > OCCUPANCY_MAX_ITEMS:
        raise ValueError('grid_queries: the resolution must be 1 .. %d, got %d' % (int(round(OCCUPANCY_MAX_ITEMS ** (1 / 3))), R))
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError('grid_queries: bounds must be finite with lo < hi, got (%r, %r)' % (lo, hi))
    c = lo + (torch.arange(R, dtype=torch.float64) + 0.5) * (hi - lo) / R
    z, y, x = torch.meshgrid(c, c, c, indexing='ij')
    q = torch.stack([x, y, z], -1).reshape(-1, 3).float().contiguous()
    if device is None or torch.device(device).type != 'cuda':
        return q
    return q.pin_memory().to(device, non_blocking=True)


def _queries_check(name, queries, B, dev):
    """queries fp32 [Q,3] (shared by the batch) or [B,Q,3] on `dev` -> (contiguous tensor, shared flag, Q)."""
    if (not isinstance(queries, torch.Tensor) or queries.dim() not in (2, 3) or queries.shape[-1] != 3 or min(queries.shape) < 1
            or queries.dtype != torch.float32):
        raise ValueError('%s: queries must be float32 [Q,3] or [B,Q,3], got %s %r'
                         % (name, getattr(queries, 'dtype', None), tuple(getattr(queries, 'shape', ()))))
    if queries.dim() == 3 and queries.shape[0] != B:
        raise ValueError('%s: queries [B,Q,3] must have B = %d, got %d' % (name, B, queries.shape[0]))
    Q = int(queries.shape[-2])
    if B > 65535 or Q > OCCUPANCY_MAX_ITEMS:
        raise ValueError('%s: at most 65535 samples of %d queries, got B = %d, Q = %d' % (name, OCCUPANCY_MAX_ITEMS, B, Q))
    if queries.device != dev:
        raise ValueError('%s: queries must be on %s, got %s' % (name, dev, queries.device))
    return queries.detach().contiguous(), int(queries.dim() == 2), Q


def _gpu_only(t):
    if not t.is_cuda:
        raise RuntimeError('vpn_amd operators run on the GPU only (got a %s tensor); there is no CPU path' % t.device.type)


def _prims_shapes(name, params, kinds, queries):
    """The inputs of a call that asks a primitive assembly about query points: ValueError from shapes and dtypes alone ->
    (B, K, Q, contiguous queries, shared flag).  Nothing here needs the GPU."""
    if (not isinstance(params, torch.Tensor) or params.dim() != 3 or params.shape[2] != PARAM_STRIDE or min(params.shape) < 1
            or params.dtype != torch.float32):
        raise ValueError('%s: params must be float32 [B,K,%d], got %s %r'
                         % (name, PARAM_STRIDE, getattr(params, 'dtype', None), tuple(getattr(params, 'shape', ()))))
    B, K = int(params.shape[0]), int(params.shape[1])
    if K > _H['VPN_MAX_PRIMS']:
        raise ValueError('%s: at most %d primitives, got %d' % (name, _H['VPN_MAX_PRIMS'], K))
    n_kinds = kinds.numel() if isinstance(kinds, torch.Tensor) else len(kinds)
    if n_kinds != K:
        raise ValueError('%s: %d kinds for %d primitives' % (name, n_kinds, K))
    if not isinstance(kinds, torch.Tensor):
        _check_kinds(tuple(int(k) for k in kinds))
    q, shared, Q = _queries_check(name, queries, B, params.device)
    return B, K, Q, q, shared


def _prims_check(name, params, kinds, queries):
    """_prims_shapes, then the GPU -> (B, K, Q, contiguous queries, shared flag, kinds on the device)."""
    B, K, Q, q, shared = _prims_shapes(name, params, kinds, queries)
    _gpu_only(params)
    return B, K, Q, q, shared, kinds_tensor(kinds, params.device)


@torch.no_grad()
def primitive_occupancy(params, kinds, queries, owner=False):
    """Occupancy of the union of K primitives at query points (vpn_occupancy_prims, one launch): params [B,K,10] fp32 (v, q, t
    as the sampler reads them), kinds [K] (a list or a device tensor), queries fp32 [Q,3] shared by the batch or [B,Q,3] ->
    occ uint8 [B,Q] (1 inside); owner=True: (occ, owner int32 [B,Q]), the lowest primitive that holds the point, -1 for
    none.  A point is inside primitive k iff m <= 1 with x~ = R^T (x - t) / v and m = x~.x~ (sphere) or max |x~_i| (cuboid);
    a NaN is outside.  No host synchronisation; everything is validated before the launch."""
    B, K, Q, q, shared, kt = _prims_check('primitive_occupancy', params, kinds, queries)
    dev = params.device
    occ = torch.empty((B, Q), dtype=torch.uint8, device=dev)
    own = torch.empty((B, Q), dtype=torch.int32, device=dev) if owner else None
    _lib.call('vpn_occupancy_prims', params.detach().contiguous(), kt, q, shared, B, K, Q, occ, own, _lib.stream())
    return (occ, own) if owner else occ


def winding_plan(B, Q, max_faces):
    """(slices, faces per slice) of the winding scan for B samples of Q queries against meshes of at most max_faces faces
    (vpn_winding_plan): a function of the three numbers alone."""
    slice_faces = ctypes.c_int(0)
    slices = _lib.lib().vpn_winding_plan(int(B), int(Q), int(max_faces), ctypes.byref(slice_faces))
    if slices < 0:
        raise ValueError('winding_plan: rejected shape B = %d, Q = %d, max_faces = %d' % (B, Q, max_faces))
    return slices, slice_faces.value


def _winding_launch(name, verts, faces, vert_offset, face_offset, max_faces, queries, xforms, B, want_w, want_occ):
    dev = verts.device
    q, shared, Q = _queries_check(name, queries, B, dev)
    if xforms is not None and tuple(getattr(xforms, 'shape', ())) != (B, 3, 4):
        raise ValueError('%s: xforms must be %r, got %r' % (name, (B, 3, 4), tuple(getattr(xforms, 'shape', ()))))
    _gpu_only(verts)
    P, F =int(verts.shape[-2]), int(faces.shape[0])
    if xforms is not None:
        xforms = _draw_tensor('xforms', xforms, (B, 3, 4), torch.float32, dev)
    ragged = int(vert_offset is not None)
    ws = _workspace('vpn_winding_workspace', B, Q, F, ragged, int(max_faces), dev=dev, dtype=torch.float64)
    w = torch.empty((B, Q), dtype=torch.float32, device=dev) if want_w else None
    occ = torch.empty((B, Q), dtype=torch.uint8, device=dev) if want_occ else None
    _lib.call('vpn_winding_number', verts.detach().contiguous(), faces_i32(faces, dev), vert_offset, face_offset, xforms, q, shared,
              B, Q, P, F, int(max_faces), ws, ws.numel() * 8, w, occ, _lib.stream())
    return w, occ


def _winding_batched(name, verts, faces, queries, xforms, want_w, want_occ):
    if (not isinstance(verts, torch.Tensor) or verts.dim() != 3 or verts.shape[2] != 3 or min(verts.shape) < 1
            or verts.dtype != torch.float32):
        raise ValueError('%s: verts must be float32 [B,P,3], got %s %r'
                         % (name, getattr(verts, 'dtype', None), tuple(getattr(verts, 'shape', ()))))
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError('%s: faces must be [F,3], one topology for the batch, got %r' % (name, tuple(getattr(faces, 'shape', ()))))
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError('%s: faces must be int32 or int64, got %s' % (name, faces.dtype))
    if max(verts.shape[1], faces.shape[0]) > OCCUPANCY_MAX_ITEMS:
        raise ValueError('%s: at most %d vertices or faces' % (name, OCCUPANCY_MAX_ITEMS))
    return _winding_launch(name, verts, faces, None, None, faces.shape[0], queries, xforms, int(verts.shape[0]), want_w, want_occ)


def _winding_ragged(name, batch, queries, xforms, want_w, want_occ):
    """batch: a MeshBatch on the device, or (verts [sumP,3], faces [sumF,3] mesh-local, vert_offset [S+1], face_offset [S+1],
    max_faces) with the largest face count of a mesh as a host number."""
    if hasattr(batch, 'face_counts'):
        if batch.verts is None:
            raise RuntimeError('vpn_amd operators run on the GPU only: pack the MeshBatch with a device; there is no CPU path')
        verts, faces, vert_offset, face_offset, max_faces = (batch.verts, batch.faces, batch.vert_offset, batch.face_offset,
                                                             max(batch.face_counts))
    else:
        try:
            verts, faces, vert_offset, face_offset, max_faces = batch
        except (TypeError, ValueError):
            raise ValueError('%s: a MeshBatch or (verts, faces, vert_offset, face_offset, max_faces) expected' % name)
    if (not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] < 1
            or verts.dtype != torch.float32):
        raise ValueError('%s: verts must be float32 [sumP,3], got %s %r'
                         % (name, getattr(verts, 'dtype', None), tuple(getattr(verts, 'shape', ()))))
    if (not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1
            or faces.dtype not in (torch.int32, torch.int64)):
        raise ValueError('%s: faces must be int32 or int64 [sumF,3], got %r' % (name, tuple(getattr(faces, 'shape', ()))))
    for what, t in (('vert_offset', vert_offset), ('face_offset', face_offset)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or t.numel() < 2:
            raise ValueError('%s: %s must be an int32 tensor of S + 1 entries' % (name, what))
    S = vert_offset.numel() - 1
    if face_offset.numel() != S + 1:
        raise ValueError('%s: the two offset tables must have S + 1 entries each' % name)
    max_faces = int(max_faces)
    if not 1 <= max_faces <= faces.shape[0]:
        raise ValueError('%s: max_faces must be 1 .. %d (the largest face count of a mesh), got %d' % (name, faces.shape[0], max_faces))
    if max(verts.shape[0], faces.shape[0]) > OCCUPANCY_MAX_ITEMS:
        raise ValueError('%s: at most %d vertices or faces' % (name, OCCUPANCY_MAX_ITEMS))
    if verts.is_cuda and not (vert_offset.is_cuda and face_offset.is_cuda):
        raise ValueError('%s: the offset tables must be on the device' % name)
    return _winding_launch(name, verts, faces, vert_offset.contiguous(), face_offset.contiguous(), max_faces, queries, xforms, S,
                           want_w, want_occ)


@torch.no_grad()
def winding_number(verts, faces, queries, xforms=None):
    """The generalized winding number of the meshes verts [B,P,3] fp32 over ONE faces [F,3] (int32 or int64, host or device) at
    queries fp32 [Q,3] (shared) or [B,Q,3] -> w fp32 [B,Q] (vpn_winding_number, the batched layout): 1 inside a closed
    outward-oriented surface, 0 outside, 2 where two closed components overlap, a fraction near a hole.  xforms [B,3,4]:
    affine rows applied to the corners first; a reflection negates w.  A face of no area, a query on a face's plane or on a
    vertex and a face with a vertex index outside [0,P) add exactly 0; a coordinate that is not finite gives NaN.  Three
    launches, no host synchronisation; everything is validated before them."""
    return _winding_batched('winding_number', verts, faces, queries, xforms, True, False)[0]


@torch.no_grad()
def ragged_winding_number(batch_or_arrays, queries, xforms=None):
    """winding_number for the packed meshes of a MeshBatch (or the arrays (verts [sumP,3], faces [sumF,3] mesh-local,
    vert_offset, face_offset [S+1] int32 on the device, max_faces)): sample b is mesh b, queries [Q,3] or [S,Q,3], xforms
    [S,3,4] -> w [S,Q].  The grid follows from the face counts the host knows: nothing is read back."""
    return _winding_ragged('ragged_winding_number', batch_or_arrays, queries, xforms, True, False)[0]


@torch.no_grad()
def mesh_occupancy(verts_or_batch, faces, queries, xforms=None):
    """Occupancy of triangle meshes at query points: uint8 [B,Q], 1 where the winding number (as fp32) exceeds 0.5; NaN is
    outside.  Batched layout: mesh_occupancy(verts [B,P,3], faces [F,3], queries); ragged layout: mesh_occupancy(batch, None,
    queries) with a MeshBatch or the arrays ragged_winding_number takes."""
    if faces is None:
        return _winding_ragged('mesh_occupancy', verts_or_batch, queries, xforms, False, True)[1]
    return _winding_batched('mesh_occupancy', verts_or_batch, faces, queries, xforms, False, True)[1]


def voliou_state(C, device):
    """A zeroed state of the volumetric evaluation for C classes (include/vpn_hip.h, vpn_voliou_accumulate): one float64 tensor
    of (1 + C) 5 + 4 + C elements, the last 4 + C of which hold int64 bit patterns (voliou_state_fields splits it)."""
    nbytes = _lib.lib().vpn_voliou_state_size(int(C))
    if nbytes == 0:
        raise ValueError('the volumetric evaluation state needs 1 .. %d classes, got %d' % (OCCUPANCY_MAX_ITEMS, int(C)))
    return torch.zeros((nbytes // 8,), dtype=torch.float64, device=device)


def voliou_state_fields(state, C):
    """Views of a state tensor (any device): (sums float64 [(1 + C) 5]: total[5] then class_sum[C][5]; counts int64 [4 + C]:
    n_samples, n_batches, n_empty, n_invalid, class_n[C])."""
    nd = (1 + int(C)) * VOLIOU_WIDTH
    if not isinstance(state, torch.Tensor) or state.dtype != torch.float64 or state.dim() != 1 or state.numel() != nd + 4 + C:
        raise ValueError('not a volumetric evaluation state of %d classes' % C)
    return state[:nd], state[nd:].view(torch.int64)


@torch.no_grad()
def voliou_step(occ_pred, occ_gt, class_index, state, C):
    """One batch of the volumetric evaluation (vpn_voliou_accumulate, two launches): occ_pred, occ_gt uint8 [B,Q] on the
    device (non-zero = inside), class_index [B] int32 on the device, state from voliou_state.  Writes the per-sample rows
    and adds the batch to `state`.  No host synchronisation; everything is validated before a launch.
    -> (rows fp32 [B,5] = iou, precision, recall, vol_pred, vol_gt; counts int32 [B,4] = and, or, prediction, ground truth)."""
    for what, t in (('occ_pred', occ_pred), ('occ_gt', occ_gt)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or min(t.shape) < 1 or t.dtype != torch.uint8:
            raise ValueError('voliou_step: %s must be uint8 [B,Q], got %s %r'
                             % (what, getattr(t, 'dtype', None), tuple(getattr(t, 'shape', ()))))
    if occ_pred.shape != occ_gt.shape:
        raise ValueError('voliou_step: occ_pred and occ_gt must have one shape, got %r and %r'
                         % (tuple(occ_pred.shape), tuple(occ_gt.shape)))
    B, Q = int(occ_pred.shape[0]), int(occ_pred.shape[1])
    if not isinstance(class_index, torch.Tensor) or class_index.numel() != B:
        raise ValueError('voliou_step: occupancies and class indices must agree on the batch size')
    if class_index.dtype != torch.int32:
        raise ValueError('class_index must be an int32 tensor on the device')
    if B > 65535 or Q > OCCUPANCY_MAX_ITEMS:
        raise ValueError('voliou_step: at most 65535 samples of %d queries, got B = %d, Q = %d' % (OCCUPANCY_MAX_ITEMS, B, Q))
    voliou_state_fields(state, C)
    _gpu_only(occ_pred)
    dev = occ_pred.device
    for what, t in (('occ_gt', occ_gt), ('class_index', class_index), ('state', state)):
        if t.device != dev:
            raise ValueError('voliou_step: %s must be on %s, got %s' % (what, dev, t.device))
    if not state.is_contiguous():
        raise ValueError('voliou_step: the state must be contiguous')
    rows = torch.empty((B, VOLIOU_WIDTH), dtype=torch.float32, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    _lib.call('vpn_voliou_accumulate', occ_pred.contiguous(), occ_gt.contiguous(), class_index.reshape(-1).contiguous(), B, Q, int(C),
              state, rows, counts, _lib.stream())
    return rows, counts


# ---- outer-surface extraction (csrc/isosurface.hip): the implicit field of a primitive assembly, surface nets
# on a lattice, and the padded mesh batch the ragged operators take.  Plain functions: nothing is differentiable.

@torch.no_grad()
def primitive_field(params, kinds, queries):
    """The implicit field of the union of K primitives at query points (vpn_primitive_field, one launch): params, kinds and
    queries as primitive_occupancy takes them -> f fp32 [B,Q] = min_k (m_k - 1), negative inside, with m_k as
    primitive_occupancy forms it: (f <= 0) equals its result bit for bit.  A primitive whose m_k is a NaN is skipped; +inf
    where no primitive is left.  No host synchronisation; everything is validated before the launch."""
    B, K, Q, q, shared, kt = _prims_check('primitive_field', params, kinds, queries)
    f = torch.empty((B, Q), dtype=torch.float32, device=params.device)
    _lib.call('vpn_primitive_field', params.detach().contiguous(), kt, q, shared, B, K, Q, f, _lib.stream())
    return f


# ---- the occupancy loss (csrc/occloss.hip): the soft union of the primitives against occupancy labels and
# an overlap penalty, differentiable to the parameters

def occloss_plan(B, Q):
    """(slices, queries per slice) of the occupancy loss's backward for B samples of Q queries (vpn_occloss_plan): a function
    of the two numbers alone."""
    slice_queries = ctypes.c_int(0)
    slices = _lib.lib().vpn_occloss_plan(int(B), int(Q), ctypes.byref(slice_queries))
    if slices < 0:
        raise ValueError('occloss_plan: rejected shape B = %d, Q = %d' % (B, Q))
    return slices, slice_queries.value


def _occloss_check(name, params, kinds, queries, labels, tau, need_labels):
    """The contract of primitive_occupancy_loss / primitive_soft_occupancy, from shapes, dtypes and devices alone: ValueError
    before any launch -> (B, K, Q, contiguous queries, shared flag, kinds on the device, contiguous labels or None, tau)."""
    tau = float(tau)
    if not (math.isfinite(tau) and tau > 0.0):
        raise ValueError('%s: tau must be finite and > 0, got %r' % (name, tau))
    B, K, Q, q, shared = _prims_shapes(name, params, kinds, queries)
    if need_labels:
        if (not isinstance(labels, torch.Tensor) or tuple(labels.shape) != (B, Q) or labels.dtype not in (torch.uint8, torch.float32)):
            raise ValueError('%s: labels must be uint8 or float32 [%d,%d], got %s %r'
                             % (name, B, Q, getattr(labels, 'dtype', None), tuple(getattr(labels, 'shape', ()))))
        if labels.device != params.device:
            raise ValueError('%s: labels must be on %s, got %s' % (name, params.device, labels.device))
        labels = labels.detach().contiguous()
    if not params.is_cuda:
        raise ValueError('%s: vpn_amd operators run on the GPU only (got %s tensors); there is no CPU path' % (name, params.device.type))
    return B, K, Q, q, shared, kinds_tensor(kinds, params.device), labels, tau


class OccupancyLossFunction(Function):
    """(out [2], n_skipped int32 [1]) of vpn_occloss_fwd: out = (mean soft-union cross-entropy, mean overlap penalty) of params
    [B,K,10] with kinds [K] at queries [Q,3] (shared != 0) or [B,Q,3] against labels uint8 or fp32 [B,Q] (see include/vpn_hip.h
    for the definitions): two launches forward, two backward, no atomics, bit-equal from run to run.  The gradient goes to
    params alone and is first order (once_differentiable); the upstream gradient [2] stays on the device.  Only the logit and
    the overlap sum per query are saved, and only when params needs a gradient; otherwise they are not written."""

    @staticmethod
    def forward(ctx, params, kt, q, shared, labels, tau):
        if (params.dim() != 3 or params.shape[2] != PARAM_STRIDE or params.dtype != torch.float32 or kt.numel() != params.shape[1]
                or tuple(labels.shape) != (params.shape[0], q.shape[-2]) or labels.dtype not in (torch.uint8, torch.float32)):
            raise ValueError('OccupancyLossFunction: params must be float32 [B,K,%d] with K kinds and labels uint8 or float32 [B,Q], '
                             'got %r, %d kinds, %s %r' % (PARAM_STRIDE, tuple(params.shape), kt.numel(), labels.dtype, tuple(labels.shape)))
        params, q, labels = _f32c(params), _f32c(q), labels.contiguous()
        B, K, Q, dev = int(params.shape[0]), int(params.shape[1]), int(q.shape[-2]), params.device
        need = ctx.needs_input_grad[0]
        lse = torch.empty((B, Q), dtype=torch.float32, device=dev) if need else None
        s = torch.empty((B, Q), dtype=torch.float32, device=dev) if need else None
        out = torch.empty(2, dtype=torch.float32, device=dev)
        n_skipped = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _workspace('vpn_occloss_workspace', B, K, Q, dev=dev)
        _lib.call('vpn_occloss_fwd', params, kt, q, int(shared), labels, int(labels.dtype == torch.uint8), B, K, Q, float(tau), ws,
                  ws.numel() * 4, lse, s, out, n_skipped, _lib.stream())
        if need:
            ctx.save_for_backward(params, kt, q, labels, lse, s)
            ctx.shared, ctx.tau = int(shared), float(tau)
        ctx.mark_non_differentiable(n_skipped)
        return out, n_skipped

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_skipped):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        params, kt, q, labels, lse, s = ctx.saved_tensors
        B, K, Q = int(params.shape[0]), int(params.shape[1]), int(q.shape[-2])
        dparams = torch.empty_like(params)
        ws = _workspace('vpn_occloss_workspace', B, K, Q, dev=params.device)
        _lib.call('vpn_occloss_bwd', _f32c(g), params, kt, q, ctx.shared, labels, int(labels.dtype == torch.uint8), lse, s, B, K, Q,
                  ctx.tau, ws, ws.numel() * 4, dparams, _lib.stream())
        return dparams, None, None, None, None, None


def primitive_occupancy_loss(params, kinds, queries, labels, tau=0.05, return_skipped=False):
    """[2] = (occupancy term, overlap term) of the union of K primitives against occupancy labels (OccupancyLossFunction):
    params [B,K,10] fp32, kinds [K] (a list or a device tensor), queries fp32 [Q,3] shared by the batch or [B,Q,3], labels
    uint8 [B,Q] (what primitive_occupancy and mesh_occupancy return) or fp32 [B,Q] in [0,1].

        occupancy term  mean over (b, i) of softplus(l) - y l, the cross-entropy of sigmoid(l) against the label, with
                        l = logsumexp_k z_k the logit of the soft union and z_k = (1 - m_k) / tau, m_k as primitive_field forms it
        overlap term    mean over (b, i) of relu(sum_k sigmoid(z_k) - 1)^2: a point claimed by more than one primitive

    A query with a coordinate that is not finite, a NaN label or no finite logit adds nothing to either term or to the gradient
    and is counted; the divisor stays B Q.  Weight the two in torch.  Differentiable to params.  return_skipped=True: (the [2],
    the count int32 [1] on the device).  Anything outside the contract raises ValueError before any launch; host tensors have
    no path."""
    B, K, Q, q, shared, kt, labels, tau = _occloss_check('primitive_occupancy_loss', params, kinds, queries, labels, tau, True)
    out, n_skipped = OccupancyLossFunction.apply(params, kt, q, shared, labels, tau)
    return (out, n_skipped) if return_skipped else out


@torch.no_grad()
def primitive_soft_occupancy(params, kinds, queries, tau):
    """(logit [B,Q], overlap_sum [B,Q]) of the soft union: l = logsumexp_k z_k and s = sum_k sigmoid(z_k) per query (the
    forward of primitive_occupancy_loss without labels, one launch); sigmoid(logit) is the soft occupancy.  -inf where no
    primitive has a finite m_k.  No autograd node: for tests and debugging."""
    B, K, Q, q, shared, kt, _, tau = _occloss_check('primitive_soft_occupancy', params, kinds, queries, None, tau, False)
    lse = torch.empty((B, Q), dtype=torch.float32, device=params.device)
    s = torch.empty((B, Q), dtype=torch.float32, device=params.device)
    _lib.call('vpn_occloss_fwd', params.detach().contiguous(), kt, q, shared, None, 0, B, K, Q, tau, None, 0, lse, s, None, None,
              _lib.stream())
    return lse, s


def _triple(name, value, cast):
    try:
        out = tuple(cast(x) for x in value) if isinstance(value, (tuple, list)) else (cast(value),) * 3
    except (TypeError, ValueError):
        out = ()
    if len(out) != 3:
        raise ValueError('lattice: %s must be one number or three (x, y, z), got %r' % (name, value))
    return out


def lattice(dims, lo=-0.5, hi=0.5, device=None):
    """The lattice of an extraction: dims = N or (Nx, Ny, Nz) nodes at the cell centres of the box [lo, hi] (numbers, or one
    per axis) -> (cx [Nx], cy [Ny], cz [Nz], queries [Nz Ny Nx, 3]) fp32, node (iz Ny + iy) Nx + ix, coordinate lo + (i + 0.5)
    (hi - lo) / N formed in float64 and rounded once: lattice(R, lo, hi) holds grid_queries(R, lo, hi) bit for bit.
    device None: host tensors."""
    dims, lo, hi = _triple('dims', dims, int), _triple('lo', lo, float), _triple('hi', hi, float)
    if min(dims) < 2 or dims[0] * dims[1] * dims[2] > OCCUPANCY_MAX_ITEMS:
        raise ValueError('lattice: every dimension must be at least 2 and their product at most %d, got %r' % (OCCUPANCY_MAX_ITEMS, dims))
    if not all(math.isfinite(a) and math.isfinite(b) and a < b for a, b in zip(lo, hi)):
        raise ValueError('lattice: bounds must be finite with lo < hi, got (%r, %r)' % (lo, hi))
    c = [lo[a] + (torch.arange(dims[a], dtype=torch.float64) + 0.5) * (hi[a] - lo[a]) / dims[a] for a in range(3)]
    z, y, x = torch.meshgrid(c[2], c[1], c[0], indexing='ij')
    out = [t.float().contiguous() for t in c] + [torch.stack([x, y, z], -1).reshape(-1, 3).float().contiguous()]
    if device is None or torch.device(device).type != 'cuda':
        return tuple(out)
    return tuple(t.pin_memory().to(device, non_blocking=True) for t in out)


_PADDED_TABLES = {}


def _padded_tables(B, max_verts, max_faces, device):
    """The offset and chunk tables of B meshes of max_verts vertices and max_faces faces each: known on the host from the
    capacities alone, uploaded once per (shape, device)."""
    key = (B, max_verts, max_faces, str(torch.device(device)))
    hit = _PADDED_TABLES.get(key)
    if hit is None:
        chunk = _H['VPN_RAGGED_CHUNK']
        rows, chunk_offset = [], [0]
        for b in range(B):
            rows += [(b, b * max_faces + start, min(chunk, max_faces - start)) for start in range(0, max_faces, chunk)]
            chunk_offset.append(len(rows))
        host = [torch.arange(B + 1, dtype=torch.int64) * max_verts, torch.arange(B + 1, dtype=torch.int64) * max_faces,
                torch.tensor(chunk_offset), torch.tensor(rows)]
        host = [t.to(torch.int32).contiguous() for t in host]
        if torch.device(device).type == 'cuda':
            host = [t.pin_memory().to(device, non_blocking=True) for t in host]
        if len(_PADDED_TABLES) > 64:
            _PADDED_TABLES.clear()
        hit = _PADDED_TABLES[key] = tuple(host)
    return hit


class PaddedMeshArrays(collections.namedtuple('PaddedMeshArrays', ('verts', 'faces', 'vert_offset', 'face_offset', 'chunk_offset',
                                                                   'chunks'))):
    """The six arrays of a MeshBatch for B meshes of one capacity each (IsoSurface.arrays): ragged_sample(*arrays, n) and
    ragged_winding_number(arrays, queries) take it as it is; the counts are the capacities, which the host knows."""
    __slots__ = ()

    @property
    def num_meshes(self):
        return self.vert_offset.numel() - 1

    @property
    def vert_counts(self):
        return [self.verts.shape[0] // self.num_meshes] * self.num_meshes

    @property
    def face_counts(self):
        return [self.faces.shape[0] // self.num_meshes] * self.num_meshes


class IsoSurface:
    """What isosurface returns: verts fp32 [B,max_verts,3], faces int32 [B,max_faces,3] (mesh-local, wound counter-clockwise
    seen from outside), counts int32 [B,4] = (n_verts, n_faces, n_open, overflow) on the device, dims = (Nx, Ny, Nz).  Rows
    past the counts are padding: vertices (0,0,0) and faces (0,0,0), which have no area, so the ragged sampler never draws
    them and they add nothing to a winding number.  A sample that overflowed its capacity is all padding."""

    def __init__(self, verts, faces, counts, dims):
        self.verts, self.faces, self.counts, self.dims = verts, faces, counts, tuple(dims)

    def __len__(self):
        return self.verts.shape[0]

    def arrays(self):
        """The padded layout as the six arrays of a MeshBatch (PaddedMeshArrays): mesh b owns max_verts vertices and max_faces
        faces.  The tables follow from the capacities and are cached per shape: no read-back, so the ragged operators take
        the result inside a captured graph (after one call outside it has filled the cache)."""
        B, max_verts, max_faces = self.verts.shape[0], self.verts.shape[1], self.faces.shape[1]
        return PaddedMeshArrays(self.verts.reshape(-1, 3), self.faces.reshape(-1, 3),
                                *_padded_tables(B, max_verts, max_faces, self.verts.device))

    def host_counts(self):
        """counts as a list of B rows: the ONE device-to-host copy."""
        return self.counts.cpu().tolist()

    def to_mesh_batch(self, device=None):
        """The trimmed meshes as a MeshBatch (one device-to-host copy of counts, then of the rows that count).  A sample
        without faces (empty, or overflowed) cannot be packed: ValueError names it."""
        from .modules.dataset import MeshBatch
        return MeshBatch.pack([(m.vertices, m.faces) for m in self.meshes()], self.verts.device if device is None else device)

    def meshes(self):
        """The trimmed meshes as a list of B TriangleMesh on the host (faces int64), for save_mesh: one device-to-host copy of
        counts, then of the arrays.  An empty or overflowed sample gives a mesh without vertices and faces."""
        from .modules.meshing import TriangleMesh
        counts, verts, faces = self.host_counts(), self.verts.cpu(), self.faces.cpu()
        out = []
        for b, (nv, nf, _open, overflow) in enumerate(counts):
            nv, nf = (0, 0) if overflow else (nv, nf)
            out.append(TriangleMesh(verts[b, :nv].clone(), faces[b, :nf].long()))
        return out


@torch.no_grad()
def isosurface(field, coords, level=0.0, max_verts=None, max_faces=None):
    """Surface nets of a field on a lattice (vpn_isosurface, four launches): field fp32 [B,Nz,Ny,Nx] on the device, coords =
    (cx [Nx], cy [Ny], cz [Nz]) fp32 on the device, strictly increasing (ops.lattice) -> IsoSurface: ONE mesh per sample, the
    boundary of {field <= level}, closed when the set stays inside the lattice (counts[:, 2] = 0), faces wound
    counter-clockwise seen from outside.  Capacities default to 8 N^2 vertices and 16 N^2 faces per sample with N the
    largest dimension; a sample that needs more is flagged (counts[:, 3]) and left empty.  Include/vpn_hip.h has the
    definition.  No host synchronisation; everything is validated before the first launch."""
    if not isinstance(field, torch.Tensor) or field.dim() != 4 or field.dtype != torch.float32 or min(field.shape) < 1:
        raise ValueError('isosurface: field must be float32 [B,Nz,Ny,Nx], got %s %r'
                         % (getattr(field, 'dtype', None), tuple(getattr(field, 'shape', ()))))
    B, Nz, Ny, Nx = (int(x) for x in field.shape)
    if min(Nx, Ny, Nz) < 2:
        raise ValueError('isosurface: every lattice dimension must be at least 2, got (Nx, Ny, Nz) = %r' % ((Nx, Ny, Nz),))
    if B > 65535 or Nx * Ny * Nz > OCCUPANCY_MAX_ITEMS:
        raise ValueError('isosurface: at most 65535 samples of %d nodes, got B = %d, %d nodes' % (OCCUPANCY_MAX_ITEMS, B, Nx * Ny * Nz))
    try:
        cx, cy, cz = coords
    except (TypeError, ValueError):
        raise ValueError('isosurface: coords must be (cx, cy, cz)')
    for what, t, n in (('cx', cx, Nx), ('cy', cy, Ny), ('cz', cz, Nz)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (n,):
            raise ValueError('isosurface: %s must be float32 [%d], got %s %r'
                             % (what, n, getattr(t, 'dtype', None), tuple(getattr(t, 'shape', ()))))
        if t.device != field.device:
            raise ValueError('isosurface: %s must be on %s, got %s' % (what, field.device, t.device))
    level = float(level)
    if not math.isfinite(level):
        raise ValueError('isosurface: the level must be finite, got %r' % level)
    N = max(Nx, Ny, Nz)
    max_verts = 8 * N * N if max_verts is None else int(max_verts)
    max_faces = 16 * N * N if max_faces is None else int(max_faces)
    if not (1 <= max_verts <= OCCUPANCY_MAX_ITEMS and 1 <= max_faces <= OCCUPANCY_MAX_ITEMS):
        raise ValueError('isosurface: capacities must be 1 .. %d, got max_verts = %d, max_faces = %d'
                         % (OCCUPANCY_MAX_ITEMS, max_verts, max_faces))
    _gpu_only(field)
    dev = field.device
    ws = _workspace('vpn_isosurface_workspace', B, Nx, Ny, Nz, dev=dev, dtype=torch.float64)
    verts = torch.empty((B, max_verts, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((B, max_faces, 3), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 4), dtype=torch.int32, device=dev)
    _lib.call('vpn_isosurface', field.detach().contiguous(), cx.contiguous(), cy.contiguous(), cz.contiguous(), level, B, Nx, Ny, Nz,
              max_verts, max_faces, ws, ws.numel() * 8, verts, faces, counts, _lib.stream())
    return IsoSurface(verts, faces, counts, (Nx, Ny, Nz))


@torch.no_grad()
def mesh_signed_distance(verts, faces, queries):
    """The signed distance to triangle meshes at query points: verts [B,P,3] fp32 over ONE faces [F,3], queries fp32 [Q,3]
    (shared) or [B,Q,3] -> fp32 [B,Q]: the distance to the nearest triangle (the square root of point_mesh_nearest's dist_p),
    negative where mesh_occupancy says inside (winding number above 0.5, so overlapping closed components count as one
    solid).  The field whose zero level re-meshes a refined mesh without its interior faces.  The two operators do the work;
    they are combined by four small elementwise torch launches (root, compare, negate, select), not by a kernel of this
    library, and a shared query set is copied B times first because point_mesh_nearest reads [B,Q,3]."""
    occ = mesh_occupancy(verts, faces, queries)
    B = verts.shape[0]
    points = queries if queries.dim() == 3 else queries[None].expand(B, -1, -1)
    dist = point_mesh_nearest(points.contiguous(), verts, faces)[0].sqrt()
    return torch.where(occ != 0, -dist, dist)


# ---- the visualisation stage (csrc/visualize.hip; modules/visualize/render.py:13-24).  Plain functions: a picture has no
# gradient.

_CONSTS = {}


def const_tensor(values, dtype, device):
    """Device tensor of a host tuple of numbers, one per (values, dtype, device): view lists, frame offsets and default
    palettes are the same call after call.  Uploaded once through pinned memory without blocking; a later call -- also one
    inside a HIP-graph capture -- finds the tensor and touches neither the host nor the copy engine."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (values, dtype, str(device))
    t = _CONSTS.get(key)
    if t is None:
        if len(_CONSTS) > 512:
            _CONSTS.clear()
        t = torch.tensor(values, dtype=dtype)
        t = t.pin_memory().to(device, non_blocking=True) if device.type == 'cuda' else t
        _CONSTS[key] = t
    return t


def _vis_target(S, V, H, W, dev, out, pitch, view_offset):
    """(frame buffer, its size in bytes, pitch, offsets or None, what to return) of a render call, validated on the host."""
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError('image size must be positive, got %d x %d' % (H, W))
    if out is None:
        if pitch is not None or view_offset is not None:
            raise ValueError('pitch and view_offset describe a frame buffer: pass it as out=')
        out = torch.empty((S, V, H, W, 3), dtype=torch.uint8, device=dev)
        return out, out.numel(), W * 3, None
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.is_contiguous()):
        raise ValueError('out must be a contiguous uint8 tensor')
    if out.device != dev:
        raise ValueError('out lives on %s, the scene on %s' % (out.device, dev))
    pitch = W * 3 if pitch is None else int(pitch)
    if pitch < W * 3:
        raise ValueError('pitch %d is shorter than a row of %d pixels' % (pitch, W))
    nbytes = out.numel()
    if view_offset is None:
        if S * V * H * pitch > nbytes:
            raise ValueError('out holds %d bytes, %d views of %d rows at pitch %d need %d' % (nbytes, S * V, H, pitch, S * V * H * pitch))
        return out, nbytes, pitch, None
    if isinstance(view_offset, torch.Tensor):
        if not (view_offset.dtype == torch.int64 and view_offset.numel() == S * V and view_offset.device == dev):
            raise ValueError('view_offset must hold S * V = %d int64 byte offsets on the device' % (S * V))
        return out, nbytes, pitch, view_offset.contiguous()         # device data: the kernel skips a view that would leave `out`
    offs = tuple(int(o) for o in view_offset)
    if len(offs) != S * V:
        raise ValueError('%d view offsets for S * V = %d views' % (len(offs), S * V))
    for o in offs:
        if o < 0 or o + (H - 1) * pitch + W * 3 > nbytes:
            raise ValueError('view offset %d puts a %d x %d view outside the %d bytes of out' % (o, H, W, nbytes))
    return out, nbytes, pitch, const_tensor(offs, torch.int64, dev)


def _vis_common(cams, S, dev, ambient, background):
    if not (isinstance(cams, torch.Tensor) and cams.dim() == 3 and cams.size(0) == S and cams.size(2) == 3 and cams.size(1) > 0):
        raise ValueError('cams must be [S, V, 3] = (dist, elev, azim) with S = %d, got %s' % (S, tuple(getattr(cams, 'shape', ()))))
    if cams.dtype != torch.float32 or cams.device != dev:
        raise ValueError('cams must be a float32 tensor on %s' % dev)
    ambient = float(ambient)
    if not 0.0 <= ambient <= 1.0:
        raise ValueError('ambient must lie in [0, 1], got %r' % ambient)
    bg = tuple(float(c) for c in background)
    if len(bg) != 3:
        raise ValueError('background is an RGB triple')
    return cams.contiguous(), ambient, bg


def _vis_f32(name, t, shape_ok, want):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not shape_ok(t):
        raise ValueError('%s must be a float32 tensor of shape %s, got %s %s' % (name, want, getattr(t, 'dtype', type(t).__name__),
                                                                               tuple(getattr(t, 'shape', ()))))
    return t.detach().contiguous()


def _vis_on_device(dev, **tensors):
    if dev.type != 'cuda':
        raise ValueError('the scene lives on the %s: the renderer runs on the GPU only, there is no CPU path' % dev.type)
    for name, t in tensors.items():
        if t.device != dev:
            raise ValueError('%s lives on %s, the scene on %s' % (name, t.device, dev))


@torch.no_grad()
def vis_primitives(params, kinds, cams, palette, H, W, *, ambient=1.0, background=(0.0, 0.0, 0.0), out=None, pitch=None,
                   view_offset=None):
    """Colour render of primitives (csrc/visualize.hip, vis_primitives_kernel): params [S,K,10], kinds (list or int32 device
    tensor [K]), cams [S,V,3] = (dist, elev, azim), palette [>= K,3] -> uint8 [S,V,H,W,3]; all views of all samples in ONE
    launch on the current stream, no host synchronisation.
    out / pitch / view_offset: write into a frame buffer instead (uint8, contiguous): pixel (row, col) of view (s, v) goes to
    byte view_offset[s * V + v] + row * pitch + col * 3 of it; offsets as a host sequence are checked here, as a device
    int64 tensor by the kernel.  Returns `out` then.  Everything is validated (ValueError) before the launch."""
    params = _vis_f32('params', params, lambda t: t.dim() == 3 and t.size(2) == PARAM_STRIDE and t.size(0) > 0 and t.size(1) > 0, '[S,K,10]')
    S, K, _ = params.shape
    dev = params.device
    if K > _H['VPN_VIS_MAX_PRIMS']:
        raise ValueError('K = %d primitives: the renderer stages at most %d (VPN_VIS_MAX_PRIMS)' % (K, _H['VPN_VIS_MAX_PRIMS']))
    if len(kinds) != K:
        raise ValueError('%d kinds for K = %d primitives' % (len(kinds), K))
    palette = _vis_f32('palette', palette, lambda t: t.dim() == 2 and t.size(1) == 3, '[>= K,3]')
    if palette.shape[0] < K:
        raise ValueError('the palette has %d colours for K = %d primitives' % (palette.shape[0], K))
    _vis_on_device(dev, palette=palette)
    kinds = kinds_tensor(kinds, dev)
    cams, ambient, bg = _vis_common(cams, S, dev, ambient, background)
    V = cams.size(1)
    out, nbytes, pitch, offs = _vis_target(S, V, H, W, dev, out, pitch, view_offset)
    _lib.call('vpn_vis_primitives', params, kinds, cams, palette, S, K, V, int(H), int(W), ambient, bg[0], bg[1], bg[2], out,
              nbytes, pitch, offs, _lib.stream())
    return out


@torch.no_grad()
def vis_mesh(verts, faces, colors, cams, H, W, *, ambient=1.0, background=(0.0, 0.0, 0.0), out=None, pitch=None, view_offset=None):
    """Colour render of triangle meshes of one topology (vis_project_kernel + vis_mesh_kernel): verts [S,P,3], faces [F,3]
    int32 on the device, colors [S,P,3], cams [S,V,3] -> uint8 [S,V,H,W,3]; two launches for all views of all samples, no
    host synchronisation.  out / pitch / view_offset as in vis_primitives."""
    verts = _vis_f32('verts', verts, lambda t: t.dim() == 3 and t.size(2) == 3 and t.size(0) > 0 and t.size(1) > 0, '[S,P,3]')
    S, P, _ = verts.shape
    dev = verts.device
    colors = _vis_f32('colors', colors, lambda t: tuple(t.shape) == (S, P, 3), '[S,P,3] = %s' % ((S, P, 3),))
    if not (isinstance(faces, torch.Tensor) and faces.dtype == torch.int32 and faces.dim() == 2 and faces.size(1) == 3
            and faces.size(0) > 0):
        raise ValueError('faces must be an int32 tensor [F,3] (ops.faces_i32 makes one)')
    _vis_on_device(dev, colors=colors, faces=faces)
    cams, ambient, bg = _vis_common(cams, S, dev, ambient, background)
    V = cams.size(1)
    out, nbytes, pitch, offs = _vis_target(S, V, H, W, dev, out, pitch, view_offset)
    ws = _workspace('vpn_vis_mesh_workspace', S, V, P, dev=dev)
    _lib.call('vpn_vis_mesh', verts, faces.contiguous(), colors, cams, S, P, faces.size(0), V, int(H), int(W), ambient, bg[0], bg[1],
              bg[2], ws, out, nbytes, pitch, offs, _lib.stream())
    return out


def _phong_const(name, value, shape, dev):
    """light / material of a render call on the device: a host sequence is uploaded once (const_tensor), a tensor is checked."""
    if isinstance(value, torch.Tensor):
        if value.dtype != torch.float32 or tuple(value.shape) != shape:
            raise ValueError('%s must be a float32 tensor of shape %s, got %s %s' % (name, shape, value.dtype, tuple(value.shape)))
        if value.device != dev:
            raise ValueError('%s lives on %s, the scene on %s' % (name, value.device, dev))
        return value.detach().contiguous()
    flat = tuple(float(x) for x in torch.as_tensor(value, dtype=torch.float64).reshape(-1).tolist())
    n = 1
    for d in shape:
        n *= d
    if len(flat) != n:
        raise ValueError('%s must hold %d numbers (shape %s), got %d' % (name, n, shape, len(flat)))
    return const_tensor(flat, torch.float32, dev).reshape(shape)


@torch.no_grad()
def phong_mesh(verts, faces, uv, texture, cams, H, W, *, light, material, shininess, out=None):
    """Textured, lit render of triangle meshes of one topology (csrc/phong.hip, phong_project_kernel + phong_mesh_kernel;
    DESIGN.md 4.11): verts [S,P,3], faces [F,3] int32 on the device, uv [S,P,2], texture [S,3,TH,TW], cams [S,V,3] = (dist,
    elev, azim) -> float32 rgb [S,V,H,W,3] in [0,1], background (0,0,0); two launches for all views of all scenes on the
    current stream, no host synchronisation.
    light: 3 numbers, a direction in the camera basis (right, up, fwd); material: 3 x 3 numbers, rows ambient, diffuse,
    specular; host sequences (uploaded once and cached) or float32 device tensors.  shininess: the specular exponent, a
    number >= 0.  out: a contiguous float32 [S,V,H,W,3] tensor to write into.  Everything is validated (ValueError) before the
    launch."""
    verts = _vis_f32('verts', verts, lambda t: t.dim() == 3 and t.size(2) == 3 and t.size(0) > 0 and t.size(1) > 0, '[S,P,3]')
    S, P, _ = verts.shape
    dev = verts.device
    uv = _vis_f32('uv', uv, lambda t: tuple(t.shape) == (S, P, 2), '[S,P,2] = %s' % ((S, P, 2),))
    texture = _vis_f32('texture', texture, lambda t: t.dim() == 4 and t.size(0) == S and t.size(1) == 3 and t.size(2) > 0 and t.size(3) > 0,
                       '[S,3,TH,TW] with S = %d' % S)
    if not (isinstance(faces, torch.Tensor) and faces.dtype == torch.int32 and faces.dim() == 2 and faces.size(1) == 3
            and faces.size(0) > 0):
        raise ValueError('faces must be an int32 tensor [F,3] (ops.faces_i32 makes one)')
    cams, _, _ = _vis_common(cams, S, dev, 1.0, (0.0, 0.0, 0.0))
    _vis_on_device(dev, uv=uv, texture=texture, faces=faces)
    V = cams.size(1)
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError('image size must be positive, got %d x %d' % (H, W))
    shininess = float(shininess)
    if not shininess >= 0.0:
        raise ValueError('shininess must be >= 0, got %r' % shininess)
    light = _phong_const('light', light, (3,), dev)
    material = _phong_const('material', material, (3, 3), dev)
    if out is None:
        out = torch.empty((S, V, H, W, 3), dtype=torch.float32, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (S, V, H, W, 3)
              and out.device == dev):
        raise ValueError('out must be a contiguous float32 tensor of shape %s on %s' % ((S, V, H, W, 3), dev))
    ws = _workspace('vpn_phong_mesh_workspace', S, V, P, dev=dev)
    _lib.call('vpn_phong_mesh', verts, faces.contiguous(), uv, texture, cams, light, material, shininess, S, P, faces.size(0), V,
              texture.size(2), texture.size(3), H, W, ws, out, _lib.stream())
    return out


# ---- the image input stage (csrc/input.hip): dataset.py:15-19,115-139 of the reference -- Resize,
# ColorJitter, ToTensor, the rotation, the rgb / silhouette split, Normalize -- bit-exact to PIL.  Data, no backward.

INPUT_JITTER, INPUT_ROTATE, INPUT_NORMALIZE = _H['VPN_INPUT_JITTER'], _H['VPN_INPUT_ROTATE'], _H['VPN_INPUT_NORMALIZE']
INPUT_TILE_ROWS = _H['VPN_INPUT_TILE_ROWS']         # output rows per tile of the resize kernel
_INPUT_TABLES = {}


def input_filter_table(in_size, out_size):
    """PIL's coefficients of Image.resize(BILINEAR) along one axis, in float64 as precompute_coeffs builds them and in
    22-bit fixed point as normalize_coeffs_8bpc rounds them: (bounds [out,2] int32 = first tap, tap count; coeffs
    [out,ksize] int32).  The triangle filter's support is max(in / out, 1) source pixels either side."""
    in_size, out_size = int(in_size), int(out_size)
    scale = float(in_size) / out_size
    fscale = max(scale, 1.0)
    support, ss = 1.0 * fscale, 1.0 / fscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = torch.zeros((out_size, 2), dtype=torch.int32)
    coeffs = torch.zeros((out_size, ksize), dtype=torch.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        bounds[xx, 0], bounds[xx, 1] = xmin, n
        for x in range(n):
            coeffs[xx, x] = int(0.5 + (w[x] / ww if ww != 0.0 else w[x]) * (1 << 22))
    return bounds, coeffs


def input_tables(Hs, Ws, H, W, device):
    """(tables, ksh, ksv, max_rows) of vpn_prepare_images for one (source size, output size): the horizontal and the vertical
    filter table as one int32 device tensor hb | hk | vb | vk, and the most source rows 8 consecutive output rows need.
    Built once per (Hs, Ws, H, W, device) and uploaded through pinned memory without blocking."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    key = (int(Hs), int(Ws), int(H), int(W), str(device))
    hit = _INPUT_TABLES.get(key)
    if hit is None:
        if len(_INPUT_TABLES) > 64:
            _INPUT_TABLES.clear()
        hb, hk = input_filter_table(Ws, W)
        vb, vk = input_filter_table(Hs, H)
        ends = vb[:, 0] + vb[:, 1]
        max_rows = max(int(ends[min(y + INPUT_TILE_ROWS, H) - 1]) - int(vb[y, 0]) for y in range(0, H, INPUT_TILE_ROWS))
        host = torch.cat([hb.reshape(-1), hk.reshape(-1), vb.reshape(-1), vk.reshape(-1)]).contiguous()
        t = host.pin_memory().to(device, non_blocking=True) if device.type == 'cuda' else host
        hit = (t, hk.size(1), vk.size(1), max_rows)
        _INPUT_TABLES[key] = hit
    return hit


@torch.no_grad()
def prepare_images(rgba_u8, H, W, *, jitter=True, rotate=False, normalize=False, factors=None, order=None, angles=None,
                   seed=0, seed_dev=None, sample_base=0, return_intermediate=False):
    """vpn_prepare_images: rgba_u8 [B,Hs,Ws,4] uint8 on the device -> (rgb [B,3,H,W], silhouette [B,1,H,W], angles [B]) fp32;
    return_intermediate appends the resized 8-bit image [B,H,W,4].  factors [B,3] fp32, order [B,3] int32, angles [B] fp32
    (degrees): the draws, host values or device tensors; one that is None is drawn in the kernel from (seed + *seed_dev,
    sample_base + b).  Three launches on the current stream, no host synchronisation; everything is validated (ValueError)
    before the launch."""
    if not (isinstance(rgba_u8, torch.Tensor) and rgba_u8.dtype == torch.uint8 and rgba_u8.dim() == 4 and rgba_u8.size(3) == 4
            and rgba_u8.numel() > 0):
        raise ValueError('rgba_u8 must be a uint8 tensor [B,Hs,Ws,4] (np.asarray(Image.open(p)) per image)')
    if not rgba_u8.is_cuda:
        raise RuntimeError('vpn_amd operators run on the GPU only (got a %s tensor); there is no CPU path' % rgba_u8.device.type)
    rgba_u8 = rgba_u8.contiguous()
    B, Hs, Ws, _ = rgba_u8.shape
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError('output size must be positive, got %d x %d' % (H, W))
    dev = rgba_u8.device
    if not jitter and (factors is not None or order is not None):
        raise ValueError('factors / order are the draws of the colour jitter: give them with jitter=True')
    if not rotate and angles is not None:
        raise ValueError('angles are the draws of the rotation: give them with rotate=True')
    if factors is not None:
        factors = _draw_tensor('factors', factors, (B, 3), torch.float32, dev)
    if order is not None:
        if not (isinstance(order, torch.Tensor) and order.is_cuda):          # host values are checked here, device ones in the kernel
            host = torch.as_tensor(order).reshape(-1, 3)
            if any(sorted(int(v) for v in row) != [0, 1, 2] for row in host):
                raise ValueError('every row of order must be a permutation of 0 (brightness), 1 (contrast), 2 (saturation)')
        order = _draw_tensor('order', order, (B, 3), torch.int32, dev)
    if angles is not None:
        angles = _draw_tensor('angles', angles, (B,), torch.float32, dev)
    seed_host, seed_ptr = int(seed) & 0xFFFFFFFFFFFFFFFF, None
    if seed_dev is not None:
        _, seed_ptr = _seed_args(seed_dev)
    tables, ksh, ksv, max_rows = input_tables(Hs, Ws, H, W, dev)
    flags = (INPUT_JITTER if jitter else 0) | (INPUT_ROTATE if rotate else 0) | (INPUT_NORMALIZE if normalize else 0)
    ws = _workspace('vpn_input_ws', B, dev=dev, dtype=torch.int64)
    inter = torch.empty((B, H, W, 4), dtype=torch.uint8, device=dev)
    rgb = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    sil = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    out_angles = torch.empty((B,), dtype=torch.float32, device=dev)
    _lib.call('vpn_prepare_images', rgba_u8, tables, ksh, ksv, max_rows, factors, order, angles, seed_host, seed_ptr,
              int(sample_base), B, Hs, Ws, H, W, flags, ws, ws.numel() * 8, inter, rgb, sil, out_angles, _lib.stream())
    return (rgb, sil, out_angles, inter) if return_intermediate else (rgb, sil, out_angles)


# ---- the ground-truth stage (csrc/gtpoints.hip): dataset.py:161-165 for a ragged batch of meshes.  Data: no
# autograd node.

RAGGED_MAX_SETS = _H['VPN_RAGGED_MAX_SETS']
RAGGED_LAUNCHES = 3          # chunk scan, chunk bases, sampling: whatever the number of meshes


@torch.no_grad()
def ragged_sample(verts, faces, vert_offset, face_offset, chunk_offset, chunks, n, *, sets=1, xforms=None, xform_mask=None, u=None,
                  seed=0, seed_dev=None, mesh_base=0, return_faces=False):
    """vpn_ragged_sample: the packed meshes of a MeshBatch (verts [sumP,3] fp32, faces [sumF,3] int32 mesh-local, vert_offset /
    face_offset / chunk_offset [S+1] int32, chunks [C,3] int32, all on the device) -> points [S,sets,n,3]; return_faces adds
    face [S,sets,n] int32 (mesh-local) and bary [S,sets,n,3].  xforms [S,sets,3,4]: the affine map of every (mesh, set), applied
    in the sets whose bit of xform_mask is set (default: all); u [S,sets,n,3]: explicit uniforms instead of the Philox draws of
    (seed + *seed_dev, mesh_base + s, set).  RAGGED_LAUNCHES launches on the current stream, no host synchronisation;
    everything is validated (ValueError) before the launch."""
    for name, t, dt in (('verts', verts, torch.float32), ('faces', faces, torch.int32), ('vert_offset', vert_offset, torch.int32),
                        ('face_offset', face_offset, torch.int32), ('chunk_offset', chunk_offset, torch.int32),
                        ('chunks', chunks, torch.int32)):
        if not (isinstance(t, torch.Tensor) and t.dtype == dt):
            raise ValueError('%s must be a %s tensor' % (name, dt))
        if not t.is_cuda:
            raise RuntimeError('vpn_amd operators run on the GPU only (got a %s tensor); there is no CPU path' % t.device.type)
        if not t.is_contiguous():
            raise ValueError('%s must be contiguous' % name)
    _augment_is_data(verts)
    S, T, n = vert_offset.numel() - 1, int(sets), int(n)
    sumP, sumF, C = verts.size(0), faces.size(0), chunks.size(0)
    if S < 1 or face_offset.numel() != S + 1 or chunk_offset.numel() != S + 1:
        raise ValueError('the three offset tables must have S + 1 entries for S >= 1 meshes')
    if verts.dim() != 2 or verts.size(1) != 3 or faces.dim() != 2 or faces.size(1) != 3 or chunks.dim() != 2 or chunks.size(1) != 3:
        raise ValueError('verts [sumP,3], faces [sumF,3] and chunks [C,3] expected')
    if sumP < 1 or sumF < 1 or C < 1 or C > sumF:
        raise ValueError('an empty batch: %d vertices, %d faces, %d chunks' % (sumP, sumF, C))
    if not 1 <= T <= RAGGED_MAX_SETS:
        raise ValueError('sets must be 1 .. %d, got %d' % (RAGGED_MAX_SETS, T))
    if n < 1:
        raise ValueError('n must be positive, got %d' % n)
    dev = verts.device
    if xforms is not None:
        xforms = _draw_tensor('xforms', xforms, (S, T, 3, 4), torch.float32, dev)
    mask = (1 << T) - 1 if xform_mask is None else int(xform_mask) & ((1 << T) - 1)
    if u is not None:
        u = _draw_tensor('u', u, (S, T, n, 3), torch.float32, dev)
    seed_host, seed_ptr = int(seed) & 0xFFFFFFFFFFFFFFFF, None
    if seed_dev is not None:
        _, seed_ptr = _seed_args(seed_dev)
    ws = _workspace('vpn_ragged_sample_workspace', sumF, C, S, dev=dev, dtype=torch.float64, floor=1)
    points = torch.empty((S, T, n, 3), dtype=torch.float32, device=dev)
    fidx = torch.empty((S, T, n), dtype=torch.int32, device=dev) if return_faces else None
    bary = torch.empty((S, T, n, 3), dtype=torch.float32, device=dev) if return_faces else None
    _lib.call('vpn_ragged_sample', verts, faces, vert_offset, face_offset, chunk_offset, chunks, xforms, mask, u, seed_host, seed_ptr,
              int(mesh_base), S, T, n, sumP, sumF, C, ws, ws.numel() * 8, points, fidx, bary, _lib.stream())
    return (points, fidx, bary) if return_faces else points


# ---- the optimiser stage (csrc/optim.hip): train.py:83-102 Adam(...) and :264 optimizer.step().  The
# parameters are updated in place: no autograd node.

ADAM_CHUNK = _H['VPN_ADAM_CHUNK']        # elements per workgroup of adam_step_kernel; the chunk table is cut with it


def adam_tables(entries):
    """The two tables of vpn_adam_step from `entries` = (p, g, m, v, n) per parameter, the first four as addresses (ints);
    an entry whose g is None (a parameter without a gradient) gets no rows.  Returns (segments, chunks): segments rows
    (p, g, m, v, n, vec) with vec = 1 where the four addresses are 16-byte aligned (the kernel then uses 16-byte accesses:
    a chunk starts a multiple of ADAM_CHUNK elements into the segment, so the alignment holds at every chunk's start),
    chunks rows (segment, first element), every segment tiled in order by chunks of ADAM_CHUNK elements; an empty segment
    keeps its row and gets no chunk.  Host arithmetic only: no GPU needed."""
    segments, chunks = [], []
    for p, g, m, v, n in entries:
        if g is None:
            continue
        vec = int(all(a % 16 == 0 for a in (p, g, m, v)))
        chunks.extend((len(segments), first) for first in range(0, int(n), ADAM_CHUNK))
        segments.append((int(p), int(g), int(m), int(v), int(n), vec))
    return segments, chunks


def adam_step(segments, num_segments, chunks, num_chunks, state, lr, lr_dev, beta1, beta2, eps, weight_decay, zero_grads=False):
    """vpn_adam_step on the current stream: segments / chunks are the DEVICE int64 tables of adam_tables (6 and 2 words a
    row), state the group's device block (VPN_ADAM_STATE_BYTES), lr_dev None or a one-element fp32 device tensor read
    instead of lr.  One launch, no host synchronisation; zero segments: nothing is launched."""
    hyper = (ctypes.c_double * 5)(lr, beta1, beta2, eps, weight_decay)
    _lib.call('vpn_adam_step', segments, int(num_segments), chunks, int(num_chunks), state, hyper, lr_dev, int(bool(zero_grads)),
              _lib.stream())


# ---- the trunk's norm / add / ReLU ring (csrc/trunknorm.hip): training-mode batch norm, the residual add
# and the ReLU of a ResNet-18 site as one op

TRUNKNORM_ONE_PASS_MAX = _H['VPN_BN_ONE_PASS_MAX']      # N = B H W up to here: one launch, the channel's slab stays in LDS
TRUNKNORM_SLICE = _H['VPN_BN_SLICE']                    # above it: two launches over slices of this many elements


def _bn_act_check(x, weight, bias, running_mean, running_var, num_batches_tracked, residual, training, momentum):
    """Everything BatchNormActFunction refuses, before any launch (and before the library is loaded)."""
    if x.dim() != 4:
        raise ValueError('batch_norm_act: x must be (B, C, H, W), got %d dimensions' % x.dim())
    C = x.shape[1]
    tensors = dict(x=x, weight=weight, bias=bias, running_mean=running_mean, running_var=running_var, residual=residual)
    for name, t in tensors.items():
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError('batch_norm_act: fp32 only (%s is %s)' % (name, t.dtype))
    if running_mean is None or running_var is None:
        raise NotImplementedError('batch_norm_act: track_running_stats=False (no running statistics) is not supported')
    if momentum is None:
        raise NotImplementedError('batch_norm_act: momentum=None (cumulative moving average) is not supported')
    if num_batches_tracked is not None and num_batches_tracked.dtype != torch.int64:
        raise ValueError('batch_norm_act: num_batches_tracked must be int64')
    for name in ('weight', 'bias', 'running_mean', 'running_var'):
        if tensors[name] is not None and tuple(tensors[name].shape) != (C,):
            raise ValueError('batch_norm_act: %s must have shape (%d,), got %s' % (name, C, tuple(tensors[name].shape)))
    if residual is not None and residual.shape != x.shape:
        raise ValueError('batch_norm_act: the residual has shape %s, x has %s' % (tuple(residual.shape), tuple(x.shape)))
    if x.numel() == 0:
        raise ValueError('batch_norm_act: empty input')
    if training and x.numel() // C == 1:
        raise ValueError('batch_norm_act: expected more than 1 value per channel when training, got input size %s'
                         % (tuple(x.shape),))
    for name, t in list(tensors.items()) + [('num_batches_tracked', num_batches_tracked)]:
        if t is not None and not t.is_cuda:
            raise ValueError('batch_norm_act runs on the GPU only (%s is a %s tensor); there is no CPU path' % (name, t.device.type))


def _bn_fwd_inputs(x, weight, bias, running_mean, running_var, num_batches_tracked, residual, training, momentum):
    """The prologue of the three forwards: _bn_act_check, then (x, residual, weight, bias) contiguous (channels_last and
    other strided inputs: NCHW first)."""
    _bn_act_check(x, weight, bias, running_mean, running_var, num_batches_tracked, residual, training, momentum)
    return tuple(None if t is None else t.contiguous() for t in (x, residual, weight, bias))


def _bn_fwd_stats(x, training, running_mean, running_var, workspace):
    """(save_mean, save_invstd, stats, ws, ws_bytes) of a forward over x.  Training: the two buffers the launch fills, which
    are also the `stats` the backward reads, and `ws`, the buffer of the library's `workspace` query (None: the caller knows
    that none is needed), None where that is empty.  Eval: no buffers, and the running statistics are the `stats`."""
    if not training:
        return None, None, (running_mean, running_var), None, 0
    B, C, H, W = x.shape
    save_mean = torch.empty((C,), dtype=torch.float32, device=x.device)
    save_invstd = torch.empty((C,), dtype=torch.float32, device=x.device)
    ws = None if workspace is None else _workspace(workspace, B, C, H, W, dev=x.device)
    if ws is not None and not ws.numel():
        ws = None
    return save_mean, save_invstd, (save_mean, save_invstd), ws, 0 if ws is None else ws.numel() * 4


def _bn_bwd_outputs(x, need_x, need_w, need_b):
    """(dx, dw, db) of the three backwards: an uninitialised buffer for each gradient that is needed, None for the others."""
    C = x.shape[1]
    dx = torch.empty_like(x) if need_x else None
    dw = torch.empty((C,), dtype=torch.float32, device=x.device) if need_w else None
    db = torch.empty((C,), dtype=torch.float32, device=x.device) if need_b else None
    return dx, dw, db


class BatchNormActFunction(Function):
    """y = relu?(batch_norm(x) + residual?) on csrc/trunknorm.hip.  apply(x, weight, bias, running_mean, running_var,
    num_batches_tracked, residual | None, training, momentum, eps, relu).  Training: batch statistics, the running statistics
    and the counter are updated in place on the device by the same launch; eval: the running statistics.  Gradients for x,
    weight, bias and residual; each is skipped when not needed."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, num_batches_tracked, residual, training, momentum, eps, relu):
        training, relu = bool(training), bool(relu)
        x, res, weight, bias = _bn_fwd_inputs(x, weight, bias, running_mean, running_var, num_batches_tracked, residual,
                                              training, momentum)
        B, C, H, W = x.shape
        y = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
        save_mean, save_invstd, stats, ws, ws_bytes = _bn_fwd_stats(x, training, running_mean, running_var, 'vpn_bn_act_workspace')
        _lib.call('vpn_bn_act_fwd', x, res, weight, bias, running_mean, running_var, num_batches_tracked, B, C, H, W,
                  int(training), float(momentum), float(eps), int(relu), y, save_mean, save_invstd, ws, ws_bytes, _lib.stream())
        ctx.save_for_backward(x, y if relu else None, weight, *stats)
        ctx.cfg = (training, float(eps), relu, residual is not None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        return _bn_ring_backward(ctx, 'act', grad_y, None)


def _bn_ring_backward(ctx, form, grad_y, grad_m):
    """The backward of BatchNormActFunction (form 'act', grad_m None) and BatchNormMeanFunction (form 'tail': grad_y or
    grad_m may be None, not both)."""
    x, y, weight, stat_a, stat_b = ctx.saved_tensors
    training, eps, relu, has_res = ctx.cfg
    need_x, need_w, need_b = ctx.needs_input_grad[:3]
    need_r = has_res and ctx.needs_input_grad[6]
    B, C, H, W = x.shape
    dy = None if grad_y is None else grad_y.contiguous()
    dm = None if grad_m is None else grad_m.contiguous()
    dx, dw, db = _bn_bwd_outputs(x, need_x, need_w, need_b)
    # without a ReLU and without a gradient of m the residual's gradient IS dy: returned as it is, nothing written
    dres = torch.empty_like(x) if need_r and (relu or dm is not None) else None
    if dx is not None or dw is not None or db is not None or dres is not None:
        ws = _workspace('vpn_bn_%s_workspace' % form, B, C, H, W, dev=x.device)
        upstream = (dy,) if form == 'act' else (dy, dm)
        _lib.call('vpn_bn_%s_bwd' % form, *upstream, x, y, weight, stat_a, stat_b, B, C, H, W, int(training), eps, int(relu), dx,
                  dres, dw, db, ws if ws.numel() else None, ws.numel() * 4, _lib.stream())
    if need_r and dres is None:
        dres = dy
    return dx, dw, db, None, None, None, dres, None, None, None, None


class BatchNormMeanFunction(Function):
    """(y, m) = (relu?(batch_norm(x) + residual?), y.mean((2, 3))) on the tt_ kernels of csrc/trunknorm.hip:
    the last norm site of the ResNet-18 trunk with the global average pool.  apply(x, weight, bias, running_mean, running_var,
    num_batches_tracked, residual | None, training, momentum, eps, relu) -> (y [B,C,H,W], m [B,C]), both differentiable.  y,
    the statistics and the counter are BatchNormActFunction's bit for bit, and what it saves is saved here (m is not needed
    backward).  Gradients for x, weight, bias and residual; each is skipped when not needed, and a gradient of y or m that
    autograd does not have is not read."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, num_batches_tracked, residual, training, momentum, eps, relu):
        training, relu = bool(training), bool(relu)
        x, res, weight, bias = _bn_fwd_inputs(x, weight, bias, running_mean, running_var, num_batches_tracked, residual,
                                              training, momentum)
        B, C, H, W = x.shape
        y = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
        m = torch.empty((B, C), dtype=torch.float32, device=x.device)
        save_mean, save_invstd, stats, ws, ws_bytes = _bn_fwd_stats(x, training, running_mean, running_var, 'vpn_bn_tail_workspace')
        _lib.call('vpn_bn_tail_fwd', x, res, weight, bias, running_mean, running_var, num_batches_tracked, B, C, H, W,
                  int(training), float(momentum), float(eps), int(relu), y, m, save_mean, save_invstd, ws, ws_bytes,
                  _lib.stream())
        ctx.save_for_backward(x, y if relu else None, weight, *stats)
        ctx.cfg = (training, float(eps), relu, residual is not None)
        ctx.set_materialize_grads(False)      # a gradient that does not exist arrives as None and travels as NULL
        return y, m

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, grad_m):
        if grad_y is None and grad_m is None:
            return (None,) * 11
        return _bn_ring_backward(ctx, 'tail', grad_y, grad_m)


def pool_out_size(H, W):
    """(PH, PW) of MaxPool2d(3, 2, 1): ((H - 1) // 2 + 1, (W - 1) // 2 + 1)."""
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


class BatchNormPoolFunction(Function):
    """p = max_pool2d(relu(batch_norm(x)), 3, 2, 1) on the tp_ kernels of csrc/trunknorm.hip: the stem of the
    ResNet-18 trunk.  apply(x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps).
    Training: batch statistics, the running statistics and the counter are updated in place on the device, bit-equal to
    BatchNormActFunction's.  The full-size activation is never written: x, p, the uint8 tap index of every window, weight and
    the two statistics are saved (in this order).  Gradients for x, weight and bias; each is skipped when not needed."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps):
        training = bool(training)
        x, _, weight, bias = _bn_fwd_inputs(x, weight, bias, running_mean, running_var, num_batches_tracked, None, training,
                                            momentum)
        B, C, H, W = x.shape
        PH, PW = pool_out_size(H, W)
        p = torch.empty((B, C, PH, PW), dtype=torch.float32, device=x.device)
        idx = torch.empty((B, C, PH, PW), dtype=torch.uint8, device=x.device)
        # the pool's query sizes the backward's workspace, needed at any N; forward only the split regime has one
        save_mean, save_invstd, stats, ws, ws_bytes = _bn_fwd_stats(
            x, training, running_mean, running_var, 'vpn_bn_pool_workspace' if B * H * W > TRUNKNORM_ONE_PASS_MAX else None)
        _lib.call('vpn_bn_pool_fwd', x, weight, bias, running_mean, running_var, num_batches_tracked, B, C, H, W, int(training),
                  float(momentum), float(eps), p, idx, save_mean, save_invstd, ws, ws_bytes, _lib.stream())
        ctx.save_for_backward(x, p, idx, weight, *stats)
        ctx.cfg = (training, float(eps))
        return p

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_p):
        x, p, idx, weight, stat_a, stat_b = ctx.saved_tensors
        training, eps = ctx.cfg
        B, C, H, W = x.shape
        dp = grad_p.contiguous()
        dx, dw, db = _bn_bwd_outputs(x, *ctx.needs_input_grad[:3])
        if dx is not None or dw is not None or db is not None:
            ws = _workspace('vpn_bn_pool_workspace', B, C, H, W, dev=x.device)
            _lib.call('vpn_bn_pool_bwd', dp, x, p, idx, weight, stat_a, stat_b, B, C, H, W, int(training), eps, dx, dw, db, ws,
                      ws.numel() * 4, _lib.stream())
        return dx, dw, db, None, None, None, None, None, None


# ---- the trunk's convolutions (csrc/trunkconv.hip, csrc/trunkstride.hip on the tile loop of csrc/vpn_conv_gemm.h; DESIGN.md
# 4.19, 4.20): nn.Conv2d(square kernel, no bias) reached through vpnet_one_resnet.py:45-57, forward and both gradients on the
# f32-input MFMA.  Conv3x3Function: kernel 3, stride 1, padding 1 inside torchvision's BasicBlock; Conv2dFunction: kernel 1, 3
# or 7, any stride and padding (the stem, the stride-2 3x3 and the 1x1 downsamples)

CONV_TILE, CONV_TILE_K = _H['VPN_CONV_TILE'], _H['VPN_CONV_TILE_K']                       # outputs / reduction elements of a workgroup's step
CONV_SPLIT_TARGET, CONV_MAX_SPLIT = _H['VPN_CONV_SPLIT_TARGET'], _H['VPN_CONV_MAX_SPLIT']   # fewer tiles than the target: K is split
CONV_FWD, CONV_DX, CONV_DW = _H['VPN_CONV_FWD'], _H['VPN_CONV_DX'], _H['VPN_CONV_DW']
CONV2D_KERNELS = (1, 3, 7)                # the kernel sizes csrc/trunkstride.hip instantiates


def conv2d_out_size(H, W, R, stride, padding):
    """(OH, OW) = ((H + 2 p - R) // stride + 1, likewise for W)."""
    return (H + 2 * padding - R) // stride + 1, (W + 2 * padding - R) // stride + 1


def conv2d_splits(B, C_in, C_out, H, W, R, stride, padding, product):
    """The host rule of include/vpn_hip.h restated: the slices S the reduction of `product` (CONV_FWD, CONV_DX, CONV_DW) is
    split into; 1: one launch, no workspace.  tests hold it to the library's vpn_conv2d_splits and vpn_conv3x3_splits."""
    OH, OW = conv2d_out_size(H, W, R, stride, padding)
    M, N, K = {CONV_FWD: (C_out, B * OH * OW, R * R * C_in), CONV_DX: (C_in, B * H * W, R * R * C_out),
               CONV_DW: (C_out, R * R * C_in, B * OH * OW)}[product]
    tiles = -(-M // CONV_TILE) * -(-N // CONV_TILE)
    if tiles >= CONV_SPLIT_TARGET:
        return 1
    return min(-(-CONV_SPLIT_TARGET // tiles), CONV_MAX_SPLIT, -(-K // CONV_TILE_K))


def conv3x3_splits(B, C_in, C_out, H, W, product):
    """conv2d_splits for kernel 3, stride 1, padding 1."""
    return conv2d_splits(B, C_in, C_out, H, W, 3, 1, 1, product)


def _conv_check(name, x, weight, kernel, kernel_ok):
    """What Conv3x3Function and Conv2dFunction both refuse about their tensors, before any launch (and before the library is
    loaded); `kernel`: the last two weight dimensions as the message names them, `kernel_ok`: the test they must pass."""
    if x.dim() != 4:
        raise ValueError('%s: x must be (B, C_in, H, W), got %d dimensions' % (name, x.dim()))
    if weight.dim() != 4 or not kernel_ok(tuple(weight.shape[2:])):
        raise ValueError('%s: weight must be (C_out, C_in, %s), got %s' % (name, kernel, tuple(weight.shape)))
    if weight.shape[1] != x.shape[1]:
        raise ValueError('%s: weight has %d input channels, x has %d (groups = 1 only)' % (name, weight.shape[1], x.shape[1]))
    for which, t in (('x', x), ('weight', weight)):
        if t.dtype != torch.float32:
            raise NotImplementedError('%s: fp32 only (%s is %s)' % (name, which, t.dtype))
    if x.numel() == 0 or weight.numel() == 0:
        raise ValueError('%s: empty input' % name)


def _conv_check_gpu(name, x, weight):
    """The last refusal of both functions: there is no CPU path."""
    for which, t in (('x', x), ('weight', weight)):
        if not t.is_cuda:
            raise ValueError('%s runs on the GPU only (%s is a %s tensor); there is no CPU path' % (name, which, t.device.type))


def _conv2d_check_args(x, weight, stride, padding):
    """What Conv2dFunction refuses wherever its tensors live: the shared checks, then what only a general convolution can
    get wrong."""
    _conv_check('conv2d', x, weight, 'R, R', lambda k: k[0] == k[1])
    R = weight.shape[2]
    if R not in CONV2D_KERNELS:
        raise NotImplementedError('conv2d: kernel size %d is not one of %s' % (R, CONV2D_KERNELS))
    if not isinstance(stride, int) or isinstance(stride, bool) or stride < 1:
        raise ValueError('conv2d: stride must be an int >= 1, got %r' % (stride,))
    if not isinstance(padding, int) or isinstance(padding, bool) or padding < 0:
        raise ValueError('conv2d: padding must be an int >= 0, got %r' % (padding,))
    if x.shape[2] + 2 * padding < R or x.shape[3] + 2 * padding < R:
        raise ValueError('conv2d: the padded image (%d + 2 x %d) x (%d + 2 x %d) is smaller than the %d x %d kernel' %
                         (x.shape[2], padding, x.shape[3], padding, R, R))


def _conv2d_check(x, weight, stride, padding):
    """Everything Conv2dFunction refuses."""
    _conv2d_check_args(x, weight, stride, padding)
    _conv_check_gpu('conv2d', x, weight)


# serves both entry families; it keeps the conv2d name and default because tests/test_trunkstride.py calls it that way
def _conv2d_ws(dims, products, dev, entry='conv2d'):
    """(workspace, bytes) of the mask `products` for the entry family `entry`, (None, 0) when no product is split."""
    ws = _workspace('vpn_%s_workspace' % entry, *dims, products, dev=dev)
    return (ws, ws.numel() * 4) if ws.numel() else (None, 0)


def _conv_forward(ctx, entry, x, weight, tail, out_hw):
    """y of entry family `entry` ('conv3x3', 'conv2d'); `tail`: the dimensions its entries take after (B, C_in, C_out, H, W)."""
    x, weight = x.contiguous(), weight.contiguous()
    B, Ci, H, W = x.shape
    Co = weight.shape[0]
    dims = (B, Ci, Co, H, W) + tail
    y = torch.empty((B, Co) + out_hw, dtype=torch.float32, device=x.device)
    ws, nbytes = _conv2d_ws(dims, CONV_FWD, x.device, entry)
    _lib.call('vpn_%s_fwd' % entry, x, weight, y, *dims, ws, nbytes, _lib.stream())
    ctx.save_for_backward(x, weight)
    ctx.dims = dims
    return y


def _conv_backward(ctx, entry, grad_y):
    """(dx, dw); each is None when not needed (a frozen trunk, an input that needs no gradient)."""
    x, weight = ctx.saved_tensors
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if not need_x and not need_w:
        return None, None
    dy = grad_y.contiguous()
    dx = torch.empty_like(x) if need_x else None
    dw = torch.empty_like(weight) if need_w else None
    ws, nbytes = _conv2d_ws(ctx.dims, (CONV_DX if need_x else 0) | (CONV_DW if need_w else 0), x.device, entry)
    _lib.call('vpn_%s_bwd' % entry, dy, x, weight, dx, dw, *ctx.dims, ws, nbytes, _lib.stream())
    return dx, dw


class Conv3x3Function(Function):
    """y = conv2d(x, weight, stride 1, padding 1) for a 3x3 kernel without bias on csrc/trunkconv.hip.  apply(x, weight):
    x (B, C_in, H, W), weight (C_out, C_in, 3, 3), fp32; strided and channels-last inputs are made NCHW-contiguous first.
    Gradients for x and weight; each is skipped when not needed (a frozen trunk, an input that needs no gradient)."""

    @staticmethod
    def forward(ctx, x, weight):
        _conv_check('conv3x3', x, weight, '3, 3', lambda k: k == (3, 3))
        _conv_check_gpu('conv3x3', x, weight)
        return _conv_forward(ctx, 'conv3x3', x, weight, (), tuple(x.shape[2:]))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        return _conv_backward(ctx, 'conv3x3', grad_y)


class Conv2dFunction(Function):
    """y = conv2d(x, weight, stride, padding) for a square kernel of 1, 3 or 7 without bias on csrc/trunkstride.hip.
    apply(x, weight, stride, padding): x (B, C_in, H, W), weight (C_out, C_in, R, R), fp32, stride >= 1 and padding >= 0
    ints; strided and channels-last inputs are made NCHW-contiguous first.  Gradients for x and weight; each is skipped
    when not needed (the stem's input, a frozen trunk)."""

    @staticmethod
    def forward(ctx, x, weight, stride, padding):
        _conv2d_check(x, weight, stride, padding)
        R = weight.shape[2]
        return _conv_forward(ctx, 'conv2d', x, weight, (R, stride, padding), conv2d_out_size(x.shape[2], x.shape[3], R, stride, padding))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        return _conv_backward(ctx, 'conv2d', grad_y) + (None, None)


# ---- the trunk's convolutions for eval-mode inference (csrc/trunkfold.hip): nn.Conv2d + nn.BatchNorm2d (eval)
# + add + ReLU reached through vpnet_one_resnet.py:45-57 as one op, the norm folded into the weights and a bias beforehand

def conv2d_bias_act(x, weight, bias=None, residual=None, stride=1, padding=0, relu=True):
    """relu?(conv2d(x, weight, stride, padding) + bias[c_out]? + residual?) on csrc/trunkfold.hip: Conv2dFunction's product
    (a square kernel of 1, 3 or 7, exact fp32 products, one summation order) with the bias, the residual add and the ReLU in
    its epilogue, in that order.  x (B, C_in, H, W), weight (C_out, C_in, R, R), bias (C_out,) or None, residual of the
    result's shape or None, all fp32 on one GPU; strided and channels-last inputs are made NCHW-contiguous first.  Inference
    only: it has no backward, and refuses an argument that requires grad while grad mode is on.  With bias=None,
    residual=None, relu=False it equals Conv2dFunction's forward bit for bit."""
    tensors = [('x', x), ('weight', weight), ('bias', bias), ('residual', residual)]
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for _n, t in tensors):
        raise RuntimeError('conv2d_bias_act is inference only (no backward): run it under torch.no_grad(), or use conv2d + '
                           'batch_norm_act, the differentiable form')
    _conv2d_check_args(x, weight, stride, padding)
    Co, R = weight.shape[0], weight.shape[2]
    if bias is not None:
        if bias.dtype != torch.float32:
            raise NotImplementedError('conv2d_bias_act: fp32 only (bias is %s)' % (bias.dtype,))
        if tuple(bias.shape) != (Co,):
            raise ValueError('conv2d_bias_act: bias must be (C_out,) = (%d,), got %s' % (Co, tuple(bias.shape)))
    if residual is not None and residual.dtype != torch.float32:
        raise NotImplementedError('conv2d_bias_act: fp32 only (residual is %s)' % (residual.dtype,))
    if not isinstance(relu, (bool, int)) or relu not in (0, 1):
        raise ValueError('conv2d_bias_act: relu must be True or False, got %r' % (relu,))
    out_shape = (x.shape[0], Co) + conv2d_out_size(x.shape[2], x.shape[3], R, stride, padding)
    if residual is not None and tuple(residual.shape) != out_shape:
        raise ValueError('conv2d_bias_act: residual must have the shape of the result %s, got %s' % (out_shape, tuple(residual.shape)))
    for which, t in tensors[1:]:
        if t is not None and t.device != x.device:
            raise ValueError('conv2d_bias_act: %s is on %s, x is on %s' % (which, t.device, x.device))
    _conv_check_gpu('conv2d_bias_act', x, weight)
    x, weight = x.contiguous(), weight.contiguous()
    bias = None if bias is None else bias.contiguous()
    residual = None if residual is None else residual.contiguous()
    B, Ci, H, W = x.shape
    dims = (B, Ci, Co, H, W, R, stride, padding)
    y = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    ws, nbytes = _conv2d_ws(dims, CONV_FWD, x.device)
    _lib.call('vpn_conv2d_bias_act_fwd', x, weight, bias, residual, y, *dims, int(relu), ws, nbytes, _lib.stream())
    return y
