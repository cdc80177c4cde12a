#!/usr/bin/env python
"""Time of LPIPS (csrc/r2l_lpips.hip, one r2l_lpips call per stack; AlexNet trunk, seeded weights) at the two sizes the README
pipeline scores: the 25 test views of 400 x 400 a training run renders every --i_testset iterations, and 8 frames of 800 x 800.
Beside it the same formulas as F.conv2d / F.max_pool2d in float32 under PyTorch-ROCm on the same card (both images of all pairs in one
batch): the yardstick, since there was no LPIPS here before, and an independent check of the kernels' values at the timed sizes.  HIP
events; per variant several windows after warm-up, median and spread; the variants alternate inside a round.  In front of the timings
the parity figures of tests/test_lpips_gpu.py (its oracle, sizes and seeds).  Writes profiles/lpips_time.txt.

The bound the kernels are held to: the multiply-adds of the five convolutions of both images, 2 FLOP each, at the 157.3 TFLOP/s of
the fp32 MFMA (the patch matrices and feature maps move far fewer bytes than that takes).

    python tools/lpips_time.py [--windows 5] [--steps 5] [--out profiles/lpips_time.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd import metrics  # noqa: E402
import test_lpips_gpu as T  # noqa: E402  (the oracle, the seeded weights and frames)

MFMA_FP32_FLOPS = 157.3e12
TEST_PASS_MS = 747.2          # profiles/train_eval_time.txt


def conv_flops(H, W):
    """2 x the multiply-adds of the five convolutions of one image"""
    total, h, w = 0, H, W
    for k, (o, i, ks, stride, pad) in enumerate(T.CONVS):
        if k in (1, 2):
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
        total += 2 * h * w * o * i * ks * ks
    return total


class TorchLPIPS:
    """the formula in float32 torch on the device"""

    def __init__(self, weights, device):
        self.w, self.b, self.lin = ([t.to(device) for t in weights[5 * j:5 * j + 5]] for j in range(3))
        self.shift, self.scale = (torch.tensor(v, device=device).view(1, 3, 1, 1) for v in (T.SHIFT, T.SCALE))

    def __call__(self, a, b):
        n = len(a)
        x = (torch.cat([a, b]).permute(0, 3, 1, 2) - self.shift) / self.scale
        d = 0
        for k, (_, _, _, stride, pad) in enumerate(T.CONVS):
            if k in (1, 2):
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, self.w[k], self.b[k], stride=stride, padding=pad))
            nrm = x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10)
            d = d + (self.lin[k].view(1, -1, 1, 1) * (nrm[:n] - nrm[n:]) ** 2).sum(1).mean((1, 2))
        return d


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def images(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand(n, 3, size // 8 + 2, size // 8 + 2, generator=g), size=(size, size), mode='bilinear', align_corners=True)
    a = (base + 0.05 * torch.randn(n, 3, size, size, generator=g)).clamp(0, 1).permute(0, 2, 3, 1).contiguous() * 2 - 1
    return a.cuda(), (a + 0.06 * torch.randn(n, size, size, 3, generator=g)).clamp(-1, 1).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--sizes', type=str, default='25x400,8x800')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'lpips_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lpips_time.py measures on the GPU; none is visible')
    weights = T.seeded_weights()
    metric, ref = metrics.LPIPS(weights), TorchLPIPS(weights, 'cuda')
    lines = [f'LPIPS v0.1, AlexNet trunk, seeded weights: r2l_lpips (csrc/r2l_lpips.hip: patch gather + the fp32 MFMA layer, up to 8 pairs per pass) against the '
             f'same formulas as F.conv2d / F.max_pool2d in float32 under PyTorch-ROCm (all pairs in one batch); HIP events, {args.windows} windows of '
             f'{args.steps} calls after warm-up, the variants alternating; median [min .. max]']
    worst, hip = 0., []
    for j, (H, W) in enumerate(T.SIZES):          # the parity figures of tests/test_lpips_gpu.py
        a, b = T.frames(H, W, seed=10 + j)
        want = T.oracle(weights, a, b, torch.float64)
        worst = max(worst, T.rel(T.oracle(weights, a, b, torch.float32), want))
        _, d, layers = T.run(metric, a, b)
        hip.append(T.rel((d, layers), want))
    lines.append('parity with the float64 CPU oracle, worst relative error of d and every d_k at ' + ', '.join(f'{H} x {W}' for H, W in T.SIZES) +
                 f': float32 CPU oracle {worst:.3e}, r2l_lpips ' + ', '.join(f'{e:.3e}' for e in hip) + f', limit (8 x the oracle\'s) {8 * worst:.3e}')
    for spec in args.sizes.split(','):
        n, size = (int(v) for v in spec.split('x'))
        a, b = images(n, size, seed=size)
        variants = [('r2l_lpips', lambda: metric(a, b)), ('torch, F.conv2d', lambda: ref(a, b))]
        with torch.no_grad():
            for name, fn in variants:        # warm-up: code objects, the convolution library's choice of algorithm
                fn()
                fn()
                torch.cuda.synchronize()
                print(f'[{spec}] warmed up: {name}', file=sys.stderr, flush=True)
            mean = metric(a, b)
            gap = float(((metric.last_d - ref(a, b)).abs() / ref(a, b)).max())
            ms = {name: [] for name, _ in variants}
            for _ in range(args.windows):
                for name, fn in variants:
                    ms[name].append(window(fn, args.steps))
        flops = 2 * n * conv_flops(size, size)
        bound_ms = flops / MFMA_FP32_FLOPS * 1e3
        lines.append(f'{n} pairs of {size} x {size}: worst relative gap of d between r2l_lpips and torch = {gap:.2e}, mean LPIPS {mean:.6f}; '
                     f'{flops / 1e9:.1f} GFLOP in the convolutions')
        med = {}
        for name, _ in variants:
            v = sorted(ms[name])
            med[name] = float(np.median(v))
            lines.append(f'  {name}: {med[name]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}] = {med[name] / n:.4f} ms per pair')
        k = med['r2l_lpips']
        lines.append(f'  torch / r2l_lpips = {med["torch, F.conv2d"] / k:.2f} x; r2l_lpips runs at {flops / k / 1e9:.1f} TFLOP/s; bound (fp32 MFMA) {bound_ms:.3f} ms, '
                     f'reached {bound_ms / k * 100:.0f} %' +
                     (f'; the stack costs {k / TEST_PASS_MS * 100:.2f} % of the {TEST_PASS_MS} ms test pass of profiles/train_eval_time.txt' if size == 400 else ''))
    metric.close()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
