"""Writes tests/golden/g10_input.npz: the fixture of the image input stage, made by PIL alone.

    python tools/make_golden_input.py

Small RGBA source images, the draws (factors, orders, angles) and PIL's 8-bit result after each of the three operations of
the loader's transform: Image.resize(BILINEAR), ImageEnhance.Brightness / Contrast / Color in a given order, and
Image.rotate(NEAREST).  tests/test_input_cpu.py holds tests/input_ref.py to these bit for bit and regenerates the file;
tests/test_input.py holds the kernels to them.

General rotation angles are REJECTED when one of the six affine coefficients lies within 1e-6 of a 16.16 rounding tie
before it is rounded: the device computes sin / cos itself, a last-bit difference moves a coefficient by about 1e-9 units,
so the kept angles round to the same six integers on both sides and everything after that is integer arithmetic."""
import math
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'g10_input.npz')
ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
ENHANCERS = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)
FACTOR_LEVELS = (0.6, 1.0, 1.4)
FAST_ANGLES = (0.0, 90.0, 180.0, 270.0)
TIE_MARGIN = 1e-6
# name -> (Hs, Ws, size of Resize): the dataset's own 137^2 -> 128^2, a non-square reduction with tile tails, an enlargement
CASES = {'d137': (137, 137, 128), 'n41': (41, 37, 16), 'u9': (9, 9, 16)}


def resized_hw(Hs, Ws, size):
    return (int(size * Hs / Ws), size) if Ws <= Hs else (size, int(size * Ws / Hs))


def coefficients(angle, H, W):
    """The six float64 values Image.rotate / affine_fixed round to 16.16 (PIL/Image.py rotate, Geometry.c)."""
    a = -math.radians(float(angle) % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2, H / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2] + cx
    m[5] = m[3] * -cx + m[4] * -cy + m[5] + cy
    m[2] += m[0] * 0.5 + m[1] * 0.5
    m[5] += m[3] * 0.5 + m[4] * 0.5
    return m


def near_tie(angle, H, W):
    for v in coefficients(angle, H, W):
        t = v * 65536.0 + 0.5
        if abs(t - round(t)) < TIE_MARGIN:
            return True
    return False


def general_angles(rng, n, sizes):
    """n fp32 angles in (0, 360), none a transpose, none near a rounding tie at any of `sizes`."""
    out = []
    while len(out) < n:
        a = float(np.float32(rng.uniform(0.0, 360.0)))
        if a % 90.0 == 0.0 or any(near_tie(a, H, W) for H, W in sizes):
            continue
        out.append(a)
    return out


def source_images(rng, Hs, Ws, smooth):
    """[3,Hs,Ws,4] uint8: a partly transparent image, a fully opaque one, a fully transparent one (its colours kept)."""
    if smooth:         # a shaded disc on a transparent ground with a soft edge, like a rendering; compresses well
        y, x = np.mgrid[0:Hs, 0:Ws].astype(np.float64)
        r = np.hypot(y - Hs * 0.47, x - Ws * 0.53) / (0.38 * min(Hs, Ws))
        alpha = np.clip((1.08 - r) * 9.0, 0.0, 1.0)
        base = np.stack([0.5 + 0.5 * np.sin(x / 9.0), 0.5 + 0.5 * np.cos(y / 7.0), np.clip(1.0 - r, 0.0, 1.0)], -1)
        img = np.concatenate([base, alpha[..., None]], -1)
        imgs = np.stack([img, img[::-1, :, [2, 0, 1, 3]], img[:, ::-1, [1, 2, 0, 3]]])
        imgs[..., :3] = np.floor(imgs[..., :3] * 6.0) / 6.0          # flat bands: the file stays small
        imgs = np.floor(imgs * 255.0 + 0.5).astype(np.uint8)
    else:
        imgs = rng.integers(0, 256, (3, Hs, Ws, 4), dtype=np.uint8)
        imgs[0, ..., 3] = np.clip(rng.integers(-128, 384, (Hs, Ws)), 0, 255)       # many 0 and 255, the rest in between
    imgs[1, ..., 3] = 255
    imgs[2, ..., 3] = 0
    return imgs


def pil(a):
    return Image.fromarray(a, 'RGBA')


def jitter(im, factors, order):
    for op in order:
        im = ENHANCERS[op](im).enhance(float(factors[op]))
    return im


def rotate(im, angle):
    return im.rotate(float(angle), Image.NEAREST, False, None, fillcolor=(0, 0, 0, 0))


def build():
    rng = np.random.default_rng(20240610)
    sizes = [resized_hw(Hs, Ws, s) for Hs, Ws, s in CASES.values()]
    z = {'general_angles': np.array(general_angles(rng, 3, sizes), np.float32),
         'fast_angles': np.array(FAST_ANGLES, np.float32), 'orders': np.array(ORDERS, np.int32),
         'factor_levels': np.array(FACTOR_LEVELS, np.float32)}
    angles = list(FAST_ANGLES) + [float(a) for a in z['general_angles']]
    for name in sorted(CASES):
        Hs, Ws, size = CASES[name]
        H, W = resized_hw(Hs, Ws, size)
        src = source_images(rng, Hs, Ws, smooth=name == 'd137')
        B = src.shape[0]
        factors = rng.uniform(0.6, 1.4, (B, 3)).astype(np.float32)
        resized = [pil(src[b]).resize((W, H), Image.BILINEAR) for b in range(B)]
        z[name + '_src'], z[name + '_size'], z[name + '_factors'] = src, np.array([size, H, W], np.int32), factors
        z[name + '_resized'] = np.stack([np.asarray(r) for r in resized])
        if name == 'd137':        # the large case keeps one route per image: its own order, then its own general angle
            jit = [jitter(resized[b], factors[b], ORDERS[b]) for b in range(B)]
            z[name + '_jittered'] = np.stack([np.asarray(j) for j in jit])
            z[name + '_rotated'] = np.stack([np.asarray(rotate(jit[b], z['general_angles'][b])) for b in range(B)])
            continue
        # each enhancer alone at the three levels [3 ops, 3 levels, B,H,W,4]; all six orders at the drawn factors [6, B,H,W,4]
        z[name + '_single'] = np.stack([np.stack([np.stack([np.asarray(E(r).enhance(float(np.float32(f)))) for r in resized])
                                                  for f in FACTOR_LEVELS]) for E in ENHANCERS])
        jit = [[jitter(resized[b], factors[b], o) for b in range(B)] for o in ORDERS]
        z[name + '_jittered'] = np.stack([np.stack([np.asarray(j) for j in row]) for row in jit])
        # the rotation of what order b (image b's own) gave, by every angle [A, B,H,W,4]
        z[name + '_rotated'] = np.stack([np.stack([np.asarray(rotate(jit[b][b], a)) for b in range(B)]) for a in angles])
    return z


def main():
    z = build()
    np.savez_compressed(OUT, **z)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    sys.exit(main())
