"""Time the image input stage on one GPU against the loader it replaces: prepare_images (resize 137^2 -> 128^2, colour
jitter, rotation, normalisation; three launches a batch) at B = 64 and B = 256, and the same transform in PIL on 16 host
threads (Resize, the three ImageEnhance blends in a drawn order, ToTensor's division, rotate, the split: what
modules/dataset/dataset.py:15-19,115-139 does per sample on loader processes).  The host side starts from decoded images,
as the device side does; PNG decoding and the upload are on neither side.  Device events around every call after a
warm-up, wall clock around the thread pool; median and the 10th..90th percentile spread of each.

    python tools/time_input.py [--reps 30] [--threads 16] [--out profiles/input_time.txt]"""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vpn_amd  # noqa: E402

SRC, SIZE = 137, 128


def pil_sample(args):
    from PIL import Image, ImageEnhance
    arr, factors, order, angle = args
    im = Image.fromarray(arr, 'RGBA').resize((SIZE, SIZE), Image.BILINEAR)
    enh = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)
    for op in order:
        im = enh[op](im).enhance(float(factors[op]))
    im = im.rotate(float(angle), Image.NEAREST)
    t = torch.from_numpy(np.asarray(im)).permute(2, 0, 1).float().div(255)
    mean = torch.tensor(vpn_amd.modules.dataset.IMAGENET_MEAN).view(3, 1, 1)
    std = torch.tensor(vpn_amd.modules.dataset.IMAGENET_STD).view(3, 1, 1)
    return (t[:3] - mean) / std, t[3:]


def spread(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[len(ts) // 10], ts[(len(ts) * 9) // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    lines = ['image input stage: %d^2 -> %d^2 RGBA, jitter + rotate + normalize; %d reps' % (SRC, SIZE, args.reps)]
    pool = ThreadPoolExecutor(args.threads)
    for B in (64, 256):
        src = rng.integers(0, 256, (B, SRC, SRC, 4), dtype=np.uint8)
        dev = torch.from_numpy(src).cuda()
        step = torch.zeros(1, dtype=torch.int64, device='cuda')
        call = lambda: vpn_amd.prepare_images(dev, size=SIZE, rotate=True, normalize=True, seed=1, seed_dev=step)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        gpu = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            gpu.append(a.elapsed_time(b))
            step += 1
        draws = [(src[i], rng.uniform(0.6, 1.4, 3), rng.permutation(3), rng.uniform(0, 360)) for i in range(B)]
        list(pool.map(pil_sample, draws))
        host = []
        for _ in range(max(3, args.reps // 6)):
            t0 = time.perf_counter()
            list(pool.map(pil_sample, draws))
            host.append((time.perf_counter() - t0) * 1e3)
        g, h = spread(gpu), spread(host)
        lines.append('B = %3d  device %.3f ms (%.3f .. %.3f) = %.0f images/s | PIL on %d threads %.1f ms (%.1f .. %.1f) = %.0f images/s'
                     % (B, g[0], g[1], g[2], B / g[0] * 1e3, args.threads, h[0], h[1], h[2], B / h[0] * 1e3))
        with vpn_amd._lib.KernelProfile() as kp:
            call()
            torch.cuda.synchronize()
        for k, (n, ms) in sorted(kp.summary().items()):
            lines.append('         %-22s %d x %.4f ms' % (k, n, ms))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
