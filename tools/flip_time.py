#!/usr/bin/env python
"""Time of FLIP (csrc/r2l_flip.hip, one r2l_flip call per stack) at the two sizes the README pipeline scores: the 25 test views of
400 x 400 a training run renders every --i_testset iterations, and 8 frames of 800 x 800.  With and without the per-pixel map;
beside it the same formulas evaluated the way the reference writes them, fourteen dense 2-D single-channel F.conv2d per pair under
PyTorch-ROCm on the same card: the yardstick, since there was no FLIP here before.  That evaluation is written for this tool from
the formulas (dense filters from their 2-D definitions, not from flip_taps.py), so it is also an independent check of the kernels'
map at the timed sizes.  HIP events; per variant several windows after warm-up, median and spread; the variants alternate inside a
round.  Writes profiles/flip_time.txt.

The bound the kernels are held to: the larger of (a) the bytes one pair must move, 24 B read + 14 row-filtered float32 planes written
and read once + 4 B of map per pixel = 140 B, at the 6.3 TB/s a streaming copy reaches, and (b) the multiply-adds of the two 1-D
passes, 2 x (4 (2 r_c + 1) + 3 (2 r_f + 1)) + 2 x 4 ((2 r_c + 1) + (2 r_f + 1)) per pixel, at 39.3 T FMA/s: the fp32 vector peak of
157.3 TFLOP/s is reached with packed FMAs only, which this library is built without (csrc/Makefile, -fno-slp-vectorize).

    python tools/flip_time.py [--windows 5] [--steps 10] [--out profiles/flip_time.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd import _lib  # noqa: E402
from efficient_nerf_amd.flip_taps import FLIP_PPD, radii  # noqa: E402

HBM_BYTES_PER_S, FMA_PER_S = 6.3e12, 157.3e12 / 4
FRAME_MS, TEST_PASS_MS = 10.0, 747.2          # an 800 x 800 fp16_fp8 frame (README); profiles/train_eval_time.txt


# ---- the formulas with dense 2-D filters, in torch ------------------------------------------------------------------------------
def dense_filters(ppd, device):
    r_c, r_f = radii(ppd)
    y, x = np.meshgrid(np.arange(-r_c, r_c + 1), np.arange(-r_c, r_c + 1), indexing='ij')
    z = (x / ppd) ** 2 + (y / ppd) ** 2
    out = {}
    for name, (a1, b1, a2, b2) in (('A', (1, 0.0047, 0, 1e-5)), ('RG', (1, 0.0053, 0, 1e-5)), ('BY', (34.1, 0.04, 13.5, 0.025))):
        g = a1 * np.sqrt(np.pi / b1) * np.exp(-np.pi ** 2 * z / b1) + a2 * np.sqrt(np.pi / b2) * np.exp(-np.pi ** 2 * z / b2)
        out[name] = g / g.sum()
    sd = 0.5 * 0.082 * ppd
    y, x = np.meshgrid(np.arange(-r_f, r_f + 1), np.arange(-r_f, r_f + 1), indexing='ij')
    g = np.exp(-(x ** 2 + y ** 2) / (2 * sd * sd))
    for name, t in (('edge', -x * g), ('point', (x ** 2 / (sd * sd) - 1) * g)):
        out[name] = np.where(t < 0, t / -t[t < 0].sum(), t / t[t > 0].sum())
    return {k: torch.tensor(v, dtype=torch.float32, device=device)[None, None] for k, v in out.items()}, r_c, r_f


class TorchFlip:
    def __init__(self, ppd, device):
        self.f, self.r_c, self.r_f = dense_filters(ppd, device)
        m = torch.tensor([[10135552 / 24577794, 8788810 / 24577794, 4435075 / 24577794], [2613072 / 12288897, 8788810 / 12288897, 887015 / 12288897],
                          [1425312 / 73733382, 8788810 / 73733382, 70074185 / 73733382]], dtype=torch.float64)
        self.m, self.minv, self.ill = m.float().to(device), torch.inverse(m).float().to(device), m.sum(1).float().to(device).view(1, 3, 1, 1)
        green, blue = (self.hunt_lab(torch.tensor(c, device=device).view(1, 3, 1, 1)) for c in ([0., 1., 0.], [0., 0., 1.]))
        self.cmax = float(self.hyab(green, blue) ** 0.7)

    def mat(self, m, x):
        return torch.einsum('ij,njhw->nihw', m, x)

    def hunt_lab(self, rgb):
        v = self.mat(self.m, rgb) / self.ill
        v = torch.where(v > 0.00885, v ** (1 / 3), v / (3 * (6 / 29) ** 2) + 4 / 29)
        L = 116 * v[:, 1:2] - 16
        return torch.cat([L, 0.01 * L * (500 * (v[:, 0:1] - v[:, 1:2])), 0.01 * L * (200 * (v[:, 1:2] - v[:, 2:3]))], 1)

    @staticmethod
    def hyab(p, q):
        d = p - q
        return d[:, 0:1].abs() + torch.linalg.vector_norm(d[:, 1:3], dim=1, keepdim=True)

    @staticmethod
    def conv(x, w, r):
        return F.conv2d(F.pad(x, (r, r, r, r), mode='replicate'), w)

    def side(self, img):
        x = img.permute(0, 3, 1, 2).clamp(0, 1)
        lin = torch.where(x > 0.04045, ((x + 0.055) / 1.055) ** 2.4, x / 12.92)
        v = self.mat(self.m, lin) / self.ill
        opp = (116 * v[:, 1:2] - 16, 500 * (v[:, 0:1] - v[:, 1:2]), 200 * (v[:, 1:2] - v[:, 2:3]))
        a, rg, by = (self.conv(c, self.f[k], self.r_c) for c, k in zip(opp, ('A', 'RG', 'BY')))
        y = (a + 16) / 116
        rgb = self.mat(self.minv, torch.cat([y + rg / 500, y, y - by / 200], 1) * self.ill).clamp(0, 1)
        yn = (opp[0] + 16) / 116
        feats = []
        for k in ('edge', 'point'):
            fx, fy = self.conv(yn, self.f[k], self.r_f), self.conv(yn, self.f[k].transpose(2, 3), self.r_f)
            feats.append(torch.sqrt(fx * fx + fy * fy))
        return self.hunt_lab(rgb), feats[0], feats[1]

    def __call__(self, a, b):
        (la, ea, pa), (lb, eb, pb) = self.side(a), self.side(b)
        pw, pcc = self.hyab(la, lb) ** 0.7, 0.4 * self.cmax
        d_c = torch.where(pw < pcc, (0.95 / pcc) * pw, 0.95 + ((pw - pcc) / (self.cmax - pcc)) * 0.05)
        d_f = torch.sqrt((1 / np.sqrt(2)) * torch.maximum((ea - eb).abs(), (pb - pa).abs())).clamp(0, 1)
        return (d_c ** (1 - d_f))[:, 0]


# ---- timing ---------------------------------------------------------------------------------------------------------------------
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
    a = (base + 0.05 * torch.randn(n, 3, size, size, generator=g)).clamp(0, 1).permute(0, 2, 3, 1).contiguous()
    return a.cuda(), (a + 0.03 * torch.randn(n, size, size, 3, generator=g)).clamp(0, 1).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--torch_steps', type=int, default=2)
    ap.add_argument('--sizes', type=str, default='25x400,8x800')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'flip_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('flip_time.py measures on the GPU; none is visible')
    L = _lib.lib()
    ppd = FLIP_PPD
    r_c, r_f = radii(ppd)
    macs = 2 * (4 * (2 * r_c + 1) + 3 * (2 * r_f + 1)) + 2 * 4 * ((2 * r_c + 1) + (2 * r_f + 1))
    dense_macs = 2 * (3 * (2 * r_c + 1) ** 2 + 4 * (2 * r_f + 1) ** 2)
    lines = [f'FLIP of image pairs at pixels_per_degree {ppd:.2f} (radii {r_c} and {r_f}): r2l_flip (csrc/r2l_flip.hip, {macs} MAC per pixel in two 1-D '
             f'passes) against the same formulas with fourteen dense 2-D F.conv2d per pair under PyTorch-ROCm ({dense_macs} MAC per pixel); HIP events, '
             f'{args.windows} windows of {args.steps} calls ({args.torch_steps} for torch) after warm-up, the variants alternating; median [min .. max]']
    ref = TorchFlip(ppd, 'cuda')
    for spec in args.sizes.split(','):
        n, size = (int(v) for v in spec.split('x'))
        a, b = images(n, size, seed=size)
        need = L.r2l_flip_workspace_floats(size, size, ppd)
        ws = torch.empty(need, device='cuda')
        fmap, means = torch.empty(n, size, size, device='cuda'), torch.empty(n, device='cuda')

        def call(with_map):
            _lib.check(L.r2l_flip(_lib.dptr(a), _lib.dptr(b), n, size, size, 0., 1., 0., 0., 1., 0., ppd, _lib.dptr(fmap) if with_map else None,
                                  _lib.dptr(means), _lib.dptr(ws), need, _lib.current_stream()))

        variants = [('r2l_flip with the map', lambda: call(True), args.steps), ('r2l_flip, means only', lambda: call(False), args.steps),
                    ('torch, dense 2-D filters', lambda: ref(a, b), args.torch_steps)]
        with torch.no_grad():
            for name, fn, _ in variants:        # warm-up: code objects, the convolution library's choice of algorithm
                fn()
                fn()
                torch.cuda.synchronize()
                print(f'[{spec}] warmed up: {name}', file=sys.stderr, flush=True)
            torch.cuda.synchronize()
            call(True)
            gap = (fmap - ref(a, b)).abs().max().item()
            ms = {name: [] for name, _, _ in variants}
            for _ in range(args.windows):
                for name, fn, steps in variants:
                    ms[name].append(window(fn, steps))
        px = n * size * size
        bound_ms = max(px * 140 / HBM_BYTES_PER_S, px * macs / FMA_PER_S) * 1e3
        which = 'bytes' if px * 140 / HBM_BYTES_PER_S > px * macs / FMA_PER_S else 'multiply-adds'
        lines.append(f'{n} pairs of {size} x {size}: L_inf(r2l_flip map - torch map) = {gap:.2e}, mean FLIP {means.double().mean().item():.6f}')
        med = {}
        for name, _, _ in variants:
            v = sorted(ms[name])
            med[name] = float(np.median(v))
            lines.append(f'  {name}: {med[name]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}] = {med[name] / n:.4f} ms per pair')
        k = med['r2l_flip with the map']
        lines.append(f'  torch / r2l_flip = {med["torch, dense 2-D filters"] / k:.1f} x; bound ({which}: 140 B and {macs} MAC per pixel) {bound_ms:.3f} ms, reached '
                     f'{bound_ms / k * 100:.0f} %; a pair costs {k / n / FRAME_MS * 100:.2f} % of the {FRAME_MS:.0f} ms an 800 x 800 fp16_fp8 frame renders in'
                     + (f'; the stack costs {k / TEST_PASS_MS * 100:.2f} % of the {TEST_PASS_MS} ms test pass of profiles/train_eval_time.txt' if size == 400 else ''))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
