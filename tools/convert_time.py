#!/usr/bin/env python
"""Time of the real-image conversion (efficient-nerf_amd/convert_data.py, csrc/r2l_convert.hip) at the size of a Blender scene: 100
RGBA images of 800 x 800 at half resolution = 16,000,000 rays, 3,906 shards.  The kernel with HIP events after warm-up, on a random
permutation as its row order (what the converter gives it), with the bytes the algorithm needs and their share of the HBM peak;
beside it the host pieces of a conversion: the two numpy permutations, the copies to and from the device.  Synthetic images: the
kernel's time does not depend on their content.  Writes profiles/convert_time.txt.

    python tools/convert_time.py [--n_img 100] [--size 800] [--full_res] [--repeat 20] [--warmup 3] [--out profiles/convert_time.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd import convert_data as CD  # noqa: E402
from efficient_nerf_amd._lib import check, current_stream, dptr, lib  # noqa: E402

HBM_PEAK = 8.0e12       # bytes/s, the HBM3E specification of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n_img', type=int, default=100)
    ap.add_argument('--size', type=int, default=800)
    ap.add_argument('--full_res', action='store_true')
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'convert_time.txt'))
    a = ap.parse_args()
    half = not a.full_res
    rs = np.random.RandomState(0)
    imgs = rs.randint(0, 256, size=(a.n_img, a.size, a.size, 4), dtype=np.uint8)
    poses = rs.randn(a.n_img, 3, 4).astype(np.float32)
    H, W, focal = CD.output_grid(a.size, a.size, 0.6911, half)
    n = a.n_img * H * W
    t0 = time.time()
    order = CD.draw_order(n, 0)
    t_order = time.time() - t0
    rows = CD.saved_rows(n)
    torch.cuda.synchronize()
    t0 = time.time()
    im_d, po_d, od_d = torch.from_numpy(imgs).cuda(), torch.from_numpy(poses).cuda(), torch.from_numpy(order[:rows].copy()).cuda()
    torch.cuda.synchronize()
    t_h2d = time.time() - t0
    out = torch.empty((rows, 9), dtype=torch.float32, device='cuda')

    def launch():
        check(lib().r2l_rays_from_images(C.c_void_p(im_d.data_ptr()), a.n_img, a.size, a.size, 4, dptr(po_d), float(focal), 1 if half else 0,
                                         C.c_void_p(od_d.data_ptr()), rows, dptr(out), current_stream()))

    for _ in range(a.warmup):
        launch()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.repeat)]
    torch.cuda.synchronize()
    for s, e in ev:
        s.record()
        launch()
        e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in ev)
    med = ms[len(ms) // 2]
    t0 = time.time()
    host = out.cpu()
    t_d2h = time.time() - t0
    assert bool(torch.isfinite(host).all())
    # what the algorithm needs: every source pixel of the kept rows once (a permutation), the order, the output rows
    px_bytes = rows * (4 if half else 1) * 4
    need = px_bytes + rows * 8 + rows * 36
    lines = [f'r2l_rays_from_images, {a.n_img} RGBA images of {a.size} x {a.size}, {"half" if half else "full"} resolution: {n} rays, {rows} rows written '
             f'({rows // CD.SPLIT_SIZE} shards), row order = a random permutation; HIP events, {a.repeat} launches after {a.warmup} warm-up launches',
             f'kernel: median {med:.3f} ms (min {ms[0]:.3f}, max {ms[-1]:.3f}) = {rows / med * 1e3:.3e} rays/s',
             f'bytes the algorithm needs: {need / 1e6:.1f} MB = pixels {px_bytes / 1e6:.1f} (each source byte once, gathered {16 if half else 4} bytes '
             f'at a time) + order {rows * 8 / 1e6:.1f} + rows out {rows * 36 / 1e6:.1f}: {need / (med * 1e-3) / 1e12:.2f} TB/s = '
             f'{need / (med * 1e-3) / HBM_PEAK:.2f} of the {HBM_PEAK / 1e12:.1f} TB/s HBM peak (bound by memory: 27 flops per row)',
             f'host pieces of one conversion at this size: two np.random.permutation({n}) + their composition {t_order:.2f} s, images + poses + order '
             f'to the device {t_h2d:.2f} s ({(imgs.nbytes + rows * 8) / 1e6:.0f} MB, pageable), rows back {t_d2h:.2f} s ({rows * 36 / 1e6:.0f} MB); reading '
             f'the PNGs and writing the {rows // CD.SPLIT_SIZE} .npy files are not timed here']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
