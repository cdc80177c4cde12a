#!/usr/bin/env python
"""Time of the PNG encoder (csrc/r2l_png.hip) at the two sizes still images are written at: 40 frames of 800 x 800 (the Blender path of
--render_only) and 120 frames of 378 x 504 (an LLFF spiral).  The frames are the shaded disc on white of tests/test_png_gpu.py, its centre
moving from frame to frame, with and without Gaussian noise of sigma 0.01 inside the disc.  Timed with HIP events, several windows after
warm-up, median and spread: the r2l_png_encode calls of a stack alone (chunked as png.encode_png chunks them, into buffers made once), and
encode_png as a caller sees it, with its allocations and its copy of the finished bytes to the host.  Beside each, from the same run: the
bytes a frame takes, the time the host needs for to8b + write_png of the same frames and its bytes (wall clock, once), the time the
W256D88 student needs to render that many frames of that size (fp16_fp8), and the wall clock of frontend.render_path with a savedir, with
and without png_device (the student's own frames, which random weights leave nearly flat: they say what the loop costs, not what a file
weighs).  Writes profiles/png_time.txt.

    python tools/png_time.py [--windows 5] [--steps 3] [--out profiles/png_time.txt]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd import R2LEngine, _lib, png as P  # noqa: E402
from efficient_nerf_amd._lib import PREC_FP16_FP8  # noqa: E402
from efficient_nerf_amd.frontend import render_path, to8b, write_png  # noqa: E402
from oracle import r2l_oracle as O  # noqa: E402


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def discs(n, H, W, sigma):
    """white, and inside a disc of radius 0.3 min(H, W) around (0.5 W + 0.1 W sin(k), 0.55 H) a shaded colour; noise of sigma inside the disc"""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    g = torch.Generator().manual_seed(H)
    out = torch.ones((n, H, W, 3), dtype=torch.float32)
    for k in range(n):
        d = torch.hypot(x - (0.5 + 0.1 * np.sin(k)) * W, y - 0.55 * H) / (0.3 * min(H, W))
        z = torch.sqrt(torch.clamp(1 - d * d, min=0))
        col = torch.stack([0.2 + 0.7 * z, 0.3 + 0.5 * z * (0.5 + 0.5 * torch.sin(x / 7)), 0.1 + 0.8 * z * (0.5 + 0.5 * torch.cos(y / 5))], -1)
        if sigma:
            col = col + sigma * torch.randn(col.shape, generator=g, dtype=torch.float64)
        out[k][d < 1] = col[d < 1].float()
    return out.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--sizes', type=str, default='40x800x800,120x378x504')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'png_time.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('png_time.py measures on the GPU; none is visible')
    L = _lib.lib()
    lines = [f'PNG on the device (csrc/r2l_png.hip: adaptive filters, run-length matches, dynamic Huffman codes per segment); HIP events, '
             f'{args.windows} windows of {args.steps} passes after warm-up, the variants alternating; median [min .. max]']
    sd = O.make_r2l_state(seed=0)
    for spec in args.sizes.split(','):
        n, H, W = (int(v) for v in spec.split('x'))
        rows, segs = P.layout(H, W)
        pitch = L.r2l_png_max_frame_bytes(H, W)
        enc = P.PNGEncoder(H, W, P._frames_per_call(n, pitch, L.r2l_png_workspace_bytes(1, H, W)), 'cuda')
        eng = R2LEngine(H, W, O.focal_from_angle(W), precision=PREC_FP16_FP8).load_state_dict(sd)
        poses = [p[:3, :4] for p in O.novel_poses(n)]
        out = torch.empty((H * W, 3), dtype=torch.float32, device='cuda')

        def render():
            for p in poses:
                eng.render(p, out=out)

        lines.append(f'{n} frames of {H} x {W}: segments of {rows} rows, {segs} per frame ({enc.n_max} frames per library call, '
                     f'{enc.need / 2 ** 20:.0f} MiB of workspace, slots of {pitch / 2 ** 20:.1f} MiB)')
        for label, sigma in (('disc', 0.), ('disc with noise', 0.01)):
            frames = discs(n, H, W, sigma)

            def calls():
                for i0 in range(0, n, enc.n_max):
                    enc.launch(frames[i0:i0 + enc.n_max])

            variants = [('r2l_png_encode, the stack', calls), ('png.encode_png, bytes on the host', lambda: P.encode_png(frames)),
                        ('the student renders as many frames', render)]
            with torch.no_grad():
                for name, fn in variants:
                    fn()
                    torch.cuda.synchronize()
                    print(f'[{spec} {label}] warmed up: {name}', file=sys.stderr, flush=True)
                ms = {name: [] for name, _ in variants}
                for _ in range(args.windows):
                    for name, fn in variants:
                        ms[name].append(window(fn, args.steps))
            files = P.encode_png(frames)
            host = frames.cpu().numpy()
            with tempfile.TemporaryDirectory() as tmp:
                t_ = time.time()
                for k in range(n):
                    write_png(os.path.join(tmp, f'{k:03d}.png'), to8b(host[k]))
                host_ms = (time.time() - t_) * 1e3
                host_bytes = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp))
            ours = float(np.mean([len(f) for f in files]))
            lines.append(f'  {label}: {ours / 1e3:.1f} kB per frame [{min(map(len, files)) / 1e3:.1f} .. {max(map(len, files)) / 1e3:.1f}] on the device, '
                         f'{host_bytes / n / 1e3:.1f} kB through to8b + write_png: {ours * n / host_bytes:.2f} x')
            med = {}
            for name, _ in variants:
                v = sorted(ms[name])
                med[name] = float(np.median(v))
                lines.append(f'    {name}: {med[name]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}] = {med[name] / n:.4f} ms per frame')
            lines.append(f'    to8b + write_png of the same frames on the host, once, wall clock: {host_ms:.0f} ms = {host_ms / n:.2f} ms per frame; the '
                         f'encode calls cost {med["r2l_png_encode, the stack"] / med["the student renders as many frames"] * 100:.1f} % of rendering as many '
                         f'frames, the host writer {host_ms / med["the student renders as many frames"] * 100:.0f} %')
        # the render loop of --render_only with its files, both ways, the student's own frames
        walls = {False: [], True: []}
        with torch.no_grad():
            for rep in range(3):
                for dev in (False, True):
                    with tempfile.TemporaryDirectory() as tmp:
                        st = {}
                        torch.cuda.synchronize()
                        t_ = time.time()
                        render_path(poses, (H, W, O.focal_from_angle(W)), 'R2L', eng, savedir=tmp, log=lambda *a: None, stats=st, png_device=dev)
                        walls[dev].append((time.time() - t_, st['render_loop_s']))
        for dev in (False, True):
            wall, loop = min(walls[dev])
            lines.append(f'  render_path with savedir, {"--png_device" if dev else "host PNGs (4 threads)"}: {wall * 1e3:.0f} ms wall clock until the last file '
                         f'is written, {loop * 1e3:.0f} ms of it the render loop (best of 3; the student\'s own frames)')
        eng.close()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
