"""Restatement of the image input stage (modules/dataset.py::prepare_images, csrc/input.hip) in numpy:
every pixel operation PIL performs for Resize(int) / ColorJitter / rotate(NEAREST) on an RGBA rendering, in the integer
or separately rounded fp32 arithmetic PIL uses, so that the result equals PIL's bit for bit (tests/test_input_cpu.py
holds it to that on every fixture case).  No PIL import here: the GPU tests compare the kernels with this file and with
the fixture PIL wrote (tools/make_golden_input.py)."""
import math

import numpy as np

PRECISION_BITS = 22                      # PIL's 8-bit resampling: 32 - 8 - 2
BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))     # lexicographic: index = the Philox draw
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
IN_STREAM = 0x80000001                   # Philox counter word 1 of the stage's draws (augment.hip uses 0x80000000)


def resized_hw(Hs, Ws, size):
    """Resize(int): the shorter side becomes `size`, the longer int(size * long / short)."""
    if Ws <= Hs:
        return int(size * Hs / Ws), int(size)
    return int(size), int(size * Ws / Hs)


def filter_table(in_size, out_size):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter over the whole axis:
    (bounds [out,2] int32 = first tap and tap count, coeffs [out,ksize] int32 = round(k * 2^22))."""
    scale = float(in_size) / out_size
    fscale = max(scale, 1.0)
    support = 1.0 * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / fscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(0.5 + k * (1 << PRECISION_BITS))      # triangle weights are never negative
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def premultiply(rgba):
    """PIL's RGBA -> RGBa: c * a / 255 rounded through MULDIV255."""
    a = rgba[..., 3:4].astype(np.uint32)
    t = rgba[..., :3].astype(np.uint32) * a + 128
    out = rgba.copy()
    out[..., :3] = ((t >> 8) + t) >> 8
    return out


def unpremultiply(rgba):
    """PIL's RGBa -> RGBA: min(255, 255 * c // a); alpha 0 and 255 copy."""
    a = rgba[..., 3:4].astype(np.uint32)
    c = rgba[..., :3].astype(np.uint32)
    q = np.minimum(255 * c // np.maximum(a, 1), 255)
    out = rgba.copy()
    out[..., :3] = np.where((a == 0) | (a == 255), c, q)
    return out


def _filter_axis(img, bounds, kk, axis):
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + img.shape[1:], np.uint8)
    for i in range(bounds.shape[0]):
        lo, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for t in range(n):
            acc += img[lo + t] * int(kk[i, t])
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(rgba, H, W):
    """Image.resize((W, H), BILINEAR) of one [Hs,Ws,4] uint8 RGBA image: premultiplied, filtered horizontally then
    vertically with an 8-bit rounding after each pass, un-premultiplied.  An unchanged size is a copy (PIL returns one
    before it premultiplies)."""
    Hs, Ws, _ = rgba.shape
    if (Hs, Ws) == (H, W):
        return rgba.copy()
    hb, hk = filter_table(Ws, W)
    vb, vk = filter_table(Hs, H)
    x = premultiply(rgba)
    x = _filter_axis(x, hb, hk, 1)
    x = _filter_axis(x, vb, vk, 0)
    return unpremultiply(x)


def luma(rgba):
    """PIL's RGB -> L."""
    c = rgba.astype(np.uint32)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16).astype(np.uint8)


def rounded_mean(L):
    """int(mean(L) + 0.5) in integers: (2 sum + n) // (2 n)."""
    s, n = int(L.astype(np.int64).sum()), int(L.size)
    return (2 * s + n) // (2 * n)


def blend(deg, img, f):
    """Image.blend(degenerate, image, f) on the three colour channels (alpha is the same in both): fp32
    in1 + f * (in2 - in1), each operation rounded, clipped when f lies outside [0, 1], truncated."""
    f = np.float32(f)
    d = deg.astype(np.int32)
    t = d.astype(np.float32) + f * (img.astype(np.int32) - d).astype(np.float32)
    assert t.dtype == np.float32
    if not (f >= 0 and f <= 1):
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.uint8)


def enhance(rgba, op, f):
    """ImageEnhance.Brightness / Contrast / Color (.enhance(f)) of one RGBA image; alpha is preserved."""
    rgb = rgba[..., :3]
    if op == BRIGHTNESS:
        deg = np.zeros_like(rgb)
    elif op == CONTRAST:
        deg = np.full_like(rgb, rounded_mean(luma(rgba)))
    else:
        deg = np.repeat(luma(rgba)[..., None], 3, -1)
    out = rgba.copy()
    out[..., :3] = blend(deg, rgb, f)
    return out


def jitter(rgba, factors, order):
    """ColorJitter's three enhancers with factors (brightness, contrast, saturation) in `order`."""
    for op in order:
        rgba = enhance(rgba, int(op), factors[int(op)])
    return rgba


def _fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def rotation_coefficients(angle, H, W):
    """The 16.16 fixed-point coefficients (a0, a1, a2, a3, a4, a5) of Image.rotate(angle, NEAREST) for an angle PIL
    does not turn into a transpose, and the six float64 values before rounding (for the fixture's tie check)."""
    a = -math.radians(float(angle) % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2, H / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    m[2] += m[0] * 0.5 + m[1] * 0.5
    m[5] += m[3] * 0.5 + m[4] * 0.5
    return tuple(_fix(v) for v in m), tuple(m)


def rotate(rgba, angle):
    """Image.rotate(angle, NEAREST, expand=False) of one [H,W,4] uint8 image; pixels from outside are 0."""
    H, W, _ = rgba.shape
    a = float(angle) % 360.0
    if a == 0:
        return rgba.copy()
    if a == 180:
        return rgba[::-1, ::-1].copy()
    if a == 90 and H == W:
        return np.rot90(rgba, 1).copy()
    if a == 270 and H == W:
        return np.rot90(rgba, 3).copy()
    (a0, a1, a2, a3, a4, a5), _ = rotation_coefficients(angle, H, W)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    xin = (a2 + x * a0 + y * a1) >> 16
    yin = (a5 + x * a3 + y * a4) >> 16
    ok = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = np.zeros_like(rgba)
    out[ok] = rgba[yin[ok], xin[ok]]
    return out


def to_outputs(rgba, normalize=False):
    """ToTensor, the split and the optional ImageNet normalisation: rgb [3,H,W], silhouette [1,H,W] fp32."""
    t = np.moveaxis(rgba, -1, 0).astype(np.float32) / np.float32(255)
    rgb, sil = t[:3], t[3:4]
    if normalize:
        mean = np.array(IMAGENET_MEAN, np.float32).reshape(3, 1, 1)
        std = np.array(IMAGENET_STD, np.float32).reshape(3, 1, 1)
        rgb = (rgb - mean) / std
    return rgb, sil


def prepare_images(rgba, size, factors=None, order=None, angles=None, normalize=False, return_stages=False):
    """The whole stage on a [B,Hs,Ws,4] uint8 batch with given draws (None: that operation is off) ->
    (rgb [B,3,H,W], silhouette [B,1,H,W], angles [B]) fp32; return_stages appends the 8-bit images after the resize,
    the jitter and the rotation."""
    B, Hs, Ws, _ = rgba.shape
    H, W = resized_hw(Hs, Ws, size)
    rs, js, ro, rgbs, sils = [], [], [], [], []
    for b in range(B):
        x = resize(rgba[b], H, W)
        rs.append(x)
        if factors is not None:
            x = jitter(x, np.asarray(factors[b], np.float32), order[b])
        js.append(x)
        if angles is not None:
            x = rotate(x, np.float32(angles[b]))
        ro.append(x)
        r, s = to_outputs(x, normalize)
        rgbs.append(r)
        sils.append(s)
    ang = np.zeros(B, np.float32) if angles is None else np.asarray(angles, np.float32)
    out = (np.stack(rgbs), np.stack(sils), ang)
    return out + (np.stack(rs), np.stack(js), np.stack(ro)) if return_stages else out


# ---- the in-kernel draws: Philox4x32-10 keyed on (seed, sample_base + b), counter (slot, IN_STREAM, b_lo, b_hi)

def _philox(c, k):
    c, k = [int(v) for v in c], [int(v) for v in k]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def draws(seed, sample_base, B):
    """(factors [B,3] fp32, order [B,3] int32, angles [B] fp32) as the kernel draws them: slot 0 gives the three factors
    0.6 + u * 0.8 (at most 1.4) and the angle u * 360 (360 itself wraps to 0), u = (word >> 8) * 2^-24; slot 1 gives the
    order, ORDERS[word * 6 >> 32] with Lemire's rejection over the four words."""
    seed &= 0xFFFFFFFFFFFFFFFF
    factors, order, angles = np.zeros((B, 3), np.float32), np.zeros((B, 3), np.int32), np.zeros(B, np.float32)
    for b in range(B):
        gb = (sample_base + b) & 0xFFFFFFFFFFFFFFFF
        key = (seed & 0xFFFFFFFF, seed >> 32)
        o = _philox((0, IN_STREAM, gb & 0xFFFFFFFF, gb >> 32), key)
        u = [np.float32(w >> 8) * np.float32(2.0 ** -24) for w in o]
        for i in range(3):
            factors[b, i] = min(np.float32(0.6) + u[i] * np.float32(0.8), np.float32(1.4))
        a = u[3] * np.float32(360.0)
        angles[b] = a if a < np.float32(360.0) else np.float32(0.0)
        o = _philox((1, IN_STREAM, gb & 0xFFFFFFFF, gb >> 32), key)
        reject, hi = (2 ** 32 - 6) % 6, 0
        for w in o:
            m = w * 6
            hi = m >> 32
            if (m & 0xFFFFFFFF) >= reject:
                break
        order[b] = ORDERS[hi]
    return factors, order, angles
