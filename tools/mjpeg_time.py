#!/usr/bin/env python
"""Time of the Motion-JPEG encoder (csrc/r2l_mjpeg.hip) at the two sizes a video is written at: 40 frames of 800 x 800 (the Blender
path of --render_only) and 120 frames of 378 x 504 (an LLFF spiral), quality 90.  Timed with HIP events: the r2l_mjpeg_encode calls of a
stack alone (chunked as video.encode_jpeg chunks them, into buffers made once), and encode_jpeg as the front end calls it, with its
allocations and its copy of the finished bytes to the host.  Beside each, from the same run: the time the W256D88 student needs to
render that many frames of that size (fp16_fp8, one launch per frame), the time the host needs for to8b + write_png of the same frames
(what a run writes today; wall clock, once), and the bytes a frame takes.  Several windows after warm-up, median and spread.  The frames are
smooth colour fields with fine noise, not renders: the random-weight student's frames are nearly flat and would flatter the byte count.
Writes profiles/mjpeg_time.txt.

    python tools/mjpeg_time.py [--windows 5] [--steps 3] [--out profiles/mjpeg_time.txt]
"""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd import R2LEngine, _lib, video as V  # noqa: E402
from efficient_nerf_amd._lib import PREC_FP16_FP8  # noqa: E402
from efficient_nerf_amd.frontend import to8b, write_png  # noqa: E402
from oracle import r2l_oracle as O  # noqa: E402


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def frames_like_renders(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    base = F.interpolate(torch.rand(n, 3, H // 16 + 2, W // 16 + 2, generator=g), size=(H, W), mode='bilinear', align_corners=True)
    return (base + 0.02 * torch.randn(n, 3, H, W, generator=g)).clamp(0, 1).permute(0, 2, 3, 1).contiguous().cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--quality', type=int, default=90)
    ap.add_argument('--sizes', type=str, default='40x800x800,120x378x504')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'mjpeg_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('mjpeg_time.py measures on the GPU; none is visible')
    L = _lib.lib()
    q = args.quality
    lines = [f'Motion-JPEG at quality {q} (csrc/r2l_mjpeg.hip: baseline JPEG, 4:4:4, Annex K Huffman tables, entropy coding on the device); HIP events, '
             f'{args.windows} windows of {args.steps} passes after warm-up, the variants alternating; median [min .. max]']
    sd = O.make_r2l_state(seed=0)
    for spec in args.sizes.split(','):
        n, H, W = (int(v) for v in spec.split('x'))
        frames = frames_like_renders(n, H, W, seed=H)
        pitch, one = L.r2l_mjpeg_max_frame_bytes(H, W), L.r2l_mjpeg_workspace_bytes(1, H, W)
        per = V._frames_per_call(n, pitch, one)
        need = L.r2l_mjpeg_workspace_bytes(per, H, W)
        ws = torch.empty(need, dtype=torch.uint8, device='cuda')
        buf = torch.empty((per, pitch), dtype=torch.uint8, device='cuda')
        sizes = torch.empty(per, dtype=torch.int64, device='cuda')

        def calls():
            for i0 in range(0, n, per):
                nb = min(per, n - i0)
                _lib.check(L.r2l_mjpeg_encode(_lib.dptr(frames[i0:i0 + nb]), nb, H, W, q, C.c_void_p(ws.data_ptr()), need, C.c_void_p(buf.data_ptr()),
                                              pitch, C.c_void_p(sizes.data_ptr()), None, _lib.current_stream()))

        eng = R2LEngine(H, W, O.focal_from_angle(W), precision=PREC_FP16_FP8).load_state_dict(sd)
        poses = [p[:3, :4] for p in O.novel_poses(n)]
        out = torch.empty((H * W, 3), dtype=torch.float32, device='cuda')

        def render():
            for p in poses:
                eng.render(p, out=out)

        variants = [('r2l_mjpeg_encode, the stack', calls), ('video.encode_jpeg, bytes on the host', lambda: V.encode_jpeg(frames, q)),
                    ('the student renders the stack', render)]
        with torch.no_grad():
            for name, fn in variants:
                fn()
                torch.cuda.synchronize()
                print(f'[{spec}] warmed up: {name}', file=sys.stderr, flush=True)
            ms = {name: [] for name, _ in variants}
            for _ in range(args.windows):
                for name, fn in variants:
                    ms[name].append(window(fn, args.steps))
        eng.close()
        jpegs = V.encode_jpeg(frames, q)
        host = frames.cpu().numpy()
        with tempfile.TemporaryDirectory() as tmp:
            t_ = time.time()
            for k in range(n):
                write_png(os.path.join(tmp, f'{k:03d}.png'), to8b(host[k]))
            png_ms = (time.time() - t_) * 1e3
            png_bytes = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp))
            t_ = time.time()
            V.write_video(os.path.join(tmp, 'v.avi'), frames, fps=30, quality=q)
            torch.cuda.synchronize()
            avi_ms, avi_bytes = (time.time() - t_) * 1e3, os.path.getsize(os.path.join(tmp, 'v.avi'))
        raw = H * W * 12
        lines.append(f'{n} frames of {H} x {W} ({per} per library call, {need / 2 ** 20:.0f} MiB of workspace, slots of {pitch / 2 ** 20:.1f} MiB): '
                     f'{np.mean([len(j) for j in jpegs]) / 1e3:.1f} kB per frame [{min(map(len, jpegs)) / 1e3:.1f} .. {max(map(len, jpegs)) / 1e3:.1f}], '
                     f'{raw / np.mean([len(j) for j in jpegs]):.0f} x below the {raw / 1e6:.2f} MB of a float32 frame')
        med = {}
        for name, _ in variants:
            v = sorted(ms[name])
            med[name] = float(np.median(v))
            lines.append(f'  {name}: {med[name]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}] = {med[name] / n:.4f} ms per frame')
        k = med['r2l_mjpeg_encode, the stack']
        lines.append(f'  to8b + write_png of the same frames on the host, once, wall clock: {png_ms:.0f} ms = {png_ms / n:.2f} ms per frame, '
                     f'{png_bytes / n / 1e3:.1f} kB per frame')
        lines.append(f'  write_video (encode + copy + the AVI file), once, wall clock: {avi_ms:.0f} ms for a file of {avi_bytes / 1e6:.2f} MB')
        lines.append(f'  the encode calls cost {k / med["the student renders the stack"] * 100:.1f} % of rendering the frames; host PNGs / write_video = '
                     f'{png_ms / avi_ms:.1f} x; the kernels move at least {30 * H * W / 1e6:.2f} MB per frame (the float32 frame in, the int16 coefficients '
                     f'out once and in twice): {30 * H * W * n / (k * 1e-3) / 1e12:.2f} TB/s of that')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
