#!/usr/bin/env python
"""Time of the PNG decoder (csrc/png_inflate.h, csrc/r2l_png_decode.hip behind png.decode_pngs) at the two sizes scenes are read at: 40
files of 800 x 800 RGBA (a Blender test split) and 120 files of 378 x 504 RGB (an LLFF scene at factor 8).  The pictures are the shaded
disc of tools/png_time.py with Gaussian noise of sigma 0.01 inside it, its centre moving from file to file; the RGBA ones carry the disc
as their alpha channel.  Three sets of files per size: written by the host writer (frontend.write_png: filter 0 on every row), with a
filter type chosen per row (the RGB set by the device encoder, png.encode_png; the RGBA set, which that encoder does not write, with the
same minimum-sum rule and zlib level 6 on the host), and with Paeth on every row (zlib level 6).

Per set, from the same run on the same files: the parent commit's loader (blender.read_png in a loop, wall clock, once; it takes
seconds per file where rows are filtered, so the loop stops after the file that passes --loop_budget_s, and the line says how many files
that was: the loop over those few is then set against decode_pngs over ALL the files), the host's zlib.decompress alone over the
batch (wall clock), the r2l_png_decode call alone on streams that are already on the device (HIP events) and png.decode_pngs as a
caller sees it, from the paths to the pixels on the device (wall clock, with the file reads, the chunk walk, the upload and the read of
the status); the last two as the median of several windows [min .. max].  The pixels of decode_pngs are compared with the loop's.
Writes profiles/png_read_time.txt.

    python tools/png_read_time.py [--sizes 800x800x4x40,378x504x3x120] [--windows 5] [--loop_budget_s 20] [--out profiles/png_read_time.txt]
"""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd import _lib, blender, png as P  # noqa: E402
from efficient_nerf_amd.frontend import to8b, write_png  # noqa: E402


def discs(n, H, W, ch, sigma=0.01):
    """uint8 [n, H, W, ch]: white, and inside a disc of radius 0.3 min(H, W) around (0.5 W + 0.1 W sin(k), 0.55 H) a shaded colour with noise"""
    y, x = np.mgrid[:H, :W].astype(np.float64)
    rng = np.random.default_rng(H)
    out = np.ones((n, H, W, ch), np.float32)
    for k in range(n):
        d = np.hypot(x - (0.5 + 0.1 * np.sin(k)) * W, y - 0.55 * H) / (0.3 * min(H, W))
        z = np.sqrt(np.clip(1 - d * d, 0, None))
        col = np.stack([0.2 + 0.7 * z, 0.3 + 0.5 * z * (0.5 + 0.5 * np.sin(x / 7)), 0.1 + 0.8 * z * (0.5 + 0.5 * np.cos(y / 5))], -1)
        col = col + sigma * rng.standard_normal(col.shape)
        inside = d < 1
        out[k, ..., :3][inside] = col[inside]
        if ch == 4:
            out[k, ..., 3] = inside
    return to8b(out)


def residuals(img):
    H, W, ch = img.shape
    x = img.reshape(H, W * ch).astype(np.int32)
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, ch:] = x[:, :-ch]
    b[1:] = x[:-1]
    c[1:, ch:] = x[:-1, :-ch]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]).astype(np.uint8)


def host_png(img, mode):
    """a PNG file with Paeth rows (mode 4) or the minimum-sum type per row (mode -1), zlib level 6"""
    import struct
    H, W, ch = img.shape
    r = residuals(img)
    choice = np.full(H, 4) if mode == 4 else np.argmin(np.abs(r.astype(np.int8).astype(np.int64)).sum(-1), 0)
    raw = np.concatenate([choice.astype(np.uint8)[:, None], r[choice, np.arange(H)]], 1).tobytes()

    def chunk(tag, body):
        return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body) & 0xffffffff)

    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, {3: 2, 4: 6}[ch], 0, 0, 0)) + chunk(b'IDAT', zlib.compress(raw, 6)) +
            chunk(b'IEND', b'')), choice


def spread(v):
    v = sorted(v)
    return f'{v[len(v) // 2]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}]', v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=str, default='800x800x4x40,378x504x3x120')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'png_read_time.txt'))
    ap.add_argument('--append', action='store_true', help='add to --out instead of starting it (one size per run)')
    ap.add_argument('--loop_budget_s', type=float, default=20., help='the parent\'s loop stops after the file that passes this many seconds (0: never)')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if not args.append:
        say('PNG on the way in (csrc/png_inflate.h, csrc/r2l_png_decode.hip: inflate by one wave per file through a 64 KiB window in LDS, the row filters '
            f'on a skewed wavefront of 64 rows); {args.windows} windows after warm-up, median [min .. max]; the disc with noise of sigma 0.01')
    for size in args.sizes.split(','):
        H, W, ch, n = (int(v) for v in size.split('x'))
        imgs = discs(n, H, W, ch)
        say(f'{n} files of {H} x {W} x {ch} ({H * (W * ch + 1) / 1e6:.2f} MB of filtered bytes each)')
        with tempfile.TemporaryDirectory() as tmp:
            sets = {}
            paths = [os.path.join(tmp, f'host_{k:03d}.png') for k in range(n)]
            for p, im in zip(paths, imgs):
                write_png(p, im)
            sets['host writer (filter 0, zlib 6)'] = paths
            name = 'device encoder (adaptive rows, run-length matches)' if ch == 3 else 'minimum-sum type per row as the device encoder chooses it, zlib 6 on the host'
            paths, types = [os.path.join(tmp, f'adaptive_{k:03d}.png') for k in range(n)], np.zeros(5, np.int64)
            if ch == 3:
                files = P.encode_png(torch.from_numpy(imgs.astype(np.float32) + 0.25).cuda() / 255., -1)
            else:
                files = []
                for im in imgs:
                    data, choice = host_png(im, -1)
                    files.append(data)
                    types += np.bincount(choice, minlength=5)
            for p, data in zip(paths, files):
                with open(p, 'wb') as f:
                    f.write(data)
            if ch == 4:
                name += f' (rows of type 0 .. 4: {types.tolist()})'
            sets[name] = paths
            paths = [os.path.join(tmp, f'paeth_{k:03d}.png') for k in range(n)]
            for p, im in zip(paths, imgs):
                with open(p, 'wb') as f:
                    f.write(host_png(im, 4)[0])
            sets['Paeth on every row, zlib 6'] = paths
            for name, paths in sets.items():
                kb = sum(os.path.getsize(p) for p in paths) / n / 1e3
                say(f'  {name}: {kb:.1f} kB per file')
                t0 = time.perf_counter()
                want = []
                for p in paths:
                    want.append(blender.read_png(p))
                    if args.loop_budget_s and time.perf_counter() - t0 > args.loop_budget_s:
                        break
                loop_ms, looped = (time.perf_counter() - t0) * 1e3, len(want)
                parsed = [P.parse_png(open(p, 'rb').read(), p) for p in paths]
                t0 = time.perf_counter()
                for p in parsed:
                    zlib.decompress(p[3])
                zlib_ms = (time.perf_counter() - t0) * 1e3
                # the library call alone, on streams already uploaded
                sizes = np.array([len(p[3]) for p in parsed], dtype=np.int64)
                off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)).cuda()
                z = torch.from_numpy(np.frombuffer(b''.join(p[3] for p in parsed), np.uint8).copy()).cuda()
                need = L.r2l_png_decode_workspace_bytes(n, H, W, ch)
                ws = torch.empty(need, dtype=torch.uint8, device='cuda')
                out = torch.empty((n, H, W, ch), dtype=torch.uint8, device='cuda')
                status = torch.empty(n, dtype=torch.int32, device='cuda')

                def call():
                    _lib.check(L.r2l_png_decode(C.c_void_p(z.data_ptr()), C.c_void_p(off.data_ptr()), n, H, W, ch, C.c_void_p(ws.data_ptr()), need,
                                                C.c_void_p(out.data_ptr()), C.c_void_p(status.data_ptr()), _lib.current_stream()))

                call()
                torch.cuda.synchronize()
                assert not status.any()
                call_ms = []
                for _ in range(args.windows):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    call()
                    b.record()
                    torch.cuda.synchronize()
                    call_ms.append(a.elapsed_time(b))
                got = P.decode_pngs(paths)
                torch.cuda.synchronize()
                same = bool(np.array_equal(got[:looped].cpu().numpy(), np.stack(want)))
                wall_ms = []
                for _ in range(args.windows):
                    t0 = time.perf_counter()
                    got = P.decode_pngs(paths)
                    torch.cuda.synchronize()
                    wall_ms.append((time.perf_counter() - t0) * 1e3)
                call_s, call_med = spread(call_ms)
                wall_s, wall_med = spread(wall_ms)
                whole = '' if looped == n else f' (the loop was stopped there: all {n} would take about {loop_ms / looped * n / 1e3:.0f} s)'
                say(f'    parent: blender.read_png in a loop over {looped} of the {n} files, wall clock: {loop_ms:.0f} ms = {loop_ms / looped:.1f} ms per file{whole}')
                say(f'    zlib.decompress alone on the host, the batch, wall clock: {zlib_ms:.1f} ms = {zlib_ms / n:.2f} ms per file')
                say(f'    r2l_png_decode, streams on the device to pixels on the device (HIP events): {call_s} = {call_med / n:.3f} ms per file')
                say(f'    png.decode_pngs, paths to pixels on the device, wall clock: {wall_s} = {wall_med / n:.3f} ms per file; '
                    f'the parent\'s loop over {looped} file(s) takes {loop_ms / wall_med:.1f} x as long as this over {n}; pixels equal to the loop\'s: {same}')
                del z, ws, out, status, got
    with open(args.out, 'a' if args.append else 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
