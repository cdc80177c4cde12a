"""GPU: the PNG encoder (csrc/r2l_png.hip behind png.encode_png) and --png_device on the command lines.

The judges are zlib.decompress (with its Adler-32 check), zlib.crc32, blender.read_png and PIL; nothing is compared with a tolerance.
Every case is encoded under filter -1 (adaptive) and 0 .. 4 (forced).  The cases are the smallest at which each stage can go wrong
(H x W): 1 x 1, 1 x 7, 7 x 1, 3 x 2, 33 x 65 (fewer rows than a segment, odd row strides); R x 60, (R + 1) x 60 and (2 R + 2) x 60 with
R = r2l_png_layout's rows of a segment at that width (exactly one segment, one row more, two rows more than two segments); constant
white 64 x 96 (runs far longer than 258, Adler-32 over 18 KB of 255, all-zero residual rows); constant grey at widths 1, 2, 85, 86, 87
and 173 (runs of 3 W and 3 W - 1 bytes: 258 exactly, and 1, 2 or 3 bytes over); black rows over a segment boundary (under filter 0 one
byte value in the whole stream, a run that has to stop at the segment's start); uniform random bytes 64 x 96 (the stored path); a
Fibonacci histogram in one segment (an unrestricted Huffman code is 18 bits deep, whichever way it breaks ties); a segment without any run; a shaded
disc on white with and without noise at 96 x 128; three frames in one call; NaN and values outside [0, 1]; bad arguments.  A segment is
never longer than 49,153 bytes (16 KiB, or one row of at most 16,384 pixels), so no stored block has to be split."""
import heapq
import io
import math
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = b'\x89PNG\r\n\x1a\n'
FILTERS = (-1, 0, 1, 2, 3, 4)
EDGE_W = 60


def exact(values):
    """frames whose bytes are the given integers: floor(255 (v + 0.25) / 255) = v in float32"""
    return ((np.asarray(values, np.float64) + 0.25) / 255.).astype(np.float32)


def natural(H, W, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    f = np.stack([0.5 + 0.4 * np.sin(x / 5 + c) * np.cos(y / 7) for c in range(3)], -1)
    return (f + 0.02 * rng.standard_normal(f.shape)).astype(np.float32)[None]


def disc(H, W, sigma, seed=0):
    """white, and inside a disc of radius 0.3 min(H, W) around (0.5 W, 0.55 H) a shaded colour; Gaussian noise of sigma inside the disc"""
    y, x = np.mgrid[:H, :W].astype(np.float64)
    d = np.hypot(x - 0.5 * W, y - 0.55 * H) / (0.3 * min(H, W))
    inside = d < 1
    z = np.sqrt(np.clip(1 - d * d, 0, None))
    col = np.stack([0.2 + 0.7 * z, 0.3 + 0.5 * z * (0.5 + 0.5 * np.sin(x / 7)), 0.1 + 0.8 * z * (0.5 + 0.5 * np.cos(y / 5))], -1)
    if sigma:
        col = col + sigma * np.random.default_rng(seed).standard_normal(col.shape)
    f = np.ones((H, W, 3))
    f[inside] = col[inside]
    return f.astype(np.float32)[None]


FIB_ROWS = 89


def fibonacci_pixels(n_bytes):
    """n_bytes pixel bytes for FIB_ROWS rows under filter 0 whose literal / length histogram is the Fibonacci sequence: end of block is the
    first 1, the 89 filter bytes (value 0) are the term 89, value i + 1 takes the other terms as far as they fit and the next value the
    rest.  The sorted bytes are read with a stride longer than any count, so that no byte repeats: no run, and the histogram is exact.
    Without the term 89 being met exactly the partial sums tie with the next term and the tree may come out half as deep."""
    fib = [1, 1]
    while sum(fib) + fib[-1] + fib[-2] <= n_bytes + 1 + FIB_ROWS:
        fib.append(fib[-1] + fib[-2])
    counts = [c for c in fib[1:] if c != FIB_ROWS]
    counts.append(n_bytes - sum(counts))
    v = np.concatenate([np.full(c, i + 1) for i, c in enumerate(counts)])
    step = max(counts) + 1
    while math.gcd(step, n_bytes) != 1:
        step += 1
    assert step < n_bytes - max(counts)
    return v[(np.arange(n_bytes) * step) % n_bytes], fib


def huffman_depth(counts):
    """the longest code of an unrestricted Huffman code over these counts"""
    heap = [(c, 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def layout(H, W):
    from efficient_nerf_amd import png
    return png.layout(H, W)


def build_cases():
    R = layout(1000, EDGE_W)[0]
    cases = {f'{H}x{W}': natural(H, W, 10 * H + W) for H, W in ((1, 1), (1, 7), (7, 1), (3, 2), (33, 65))}
    cases.update({f'edge-{name}': natural(H, EDGE_W, H) for name, H in (('R', R), ('R+1', R + 1), ('2R+2', 2 * R + 2))})
    cases['white'] = np.ones((1, 64, 96, 3), np.float32)
    cases.update({f'grey-w{W}': np.full((1, 5, W, 3), 0.5, np.float32) for W in (1, 2, 85, 86, 87, 173)})
    cases['black'] = np.zeros((1, R + 3, EDGE_W, 3), np.float32)
    cases['random'] = exact(np.random.default_rng(5).integers(0, 256, (1, 64, 96, 3)))
    fib, _ = fibonacci_pixels(FIB_ROWS * 3 * EDGE_W)
    cases['fibonacci'] = exact(fib.reshape(1, FIB_ROWS, EDGE_W, 3))
    y, x = np.mgrid[:20, :90]
    cases['norun'] = exact(((x * 5 + y * 3) % 17 + 1).reshape(1, 20, 30, 3))
    cases['disc'] = disc(96, 128, 0.)
    cases['disc-noise'] = disc(96, 128, 0.01)
    cases['stack'] = np.concatenate([natural(33, 65, 1), np.ones((1, 33, 65, 3), np.float32),
                                     exact(np.random.default_rng(8).integers(0, 256, (1, 33, 65, 3)))])
    odd = natural(9, 17, 3)
    odd = 3. * odd - 1.                                                   # from -1.5 to 2.5
    cases['outside'] = odd
    return cases, R


def chunks(data):
    """[(tag, body)] of a PNG file; asserts the signature, every CRC against zlib.crc32 and that nothing follows IEND"""
    assert data[:8] == SIG
    pos, out = 8, []
    while pos < len(data):
        n, tag = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert len(body) == n
        crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xffffffff, (tag, len(out))
        out.append((tag, body))
        pos += 12 + n
    assert pos == len(data) and out[-1] == (b'IEND', b'')
    return out


def filtered_rows(img):
    """the five residual rows of every row of a uint8 image [H, W, 3]: [5, H, 3 W] uint8, the PNG specification's arithmetic"""
    H, W, _ = img.shape
    x = img.reshape(H, 3 * W).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - (a + b) // 2, x - paeth]).astype(np.uint8)


def min_sum_choice(img):
    """per row the type with the smallest sum of |residual as int8|, ties to the lowest type"""
    r = filtered_rows(img).astype(np.int8).astype(np.int64)
    return np.argmin(np.abs(r).sum(-1), 0)                               # argmin returns the first of equal sums


def to8b(frames):
    from efficient_nerf_amd import frontend as fe
    return fe.to8b(frames)


@pytest.fixture(scope='module')
def results(pkg, built_lib):
    """every case encoded once under every filter: shared by the tests below, changed by none"""
    from efficient_nerf_amd.png import encode_png
    cases, R = build_cases()
    out = {}
    for name, frames in cases.items():
        dev = torch.from_numpy(frames).cuda()
        out[name] = dict(frames=frames, files={f: encode_png(dev, f) for f in FILTERS})
    return out, R


CASE_NAMES = ['1x1', '1x7', '7x1', '3x2', '33x65', 'edge-R', 'edge-R+1', 'edge-2R+2', 'white', 'grey-w1', 'grey-w2', 'grey-w85', 'grey-w86', 'grey-w87',
              'grey-w173', 'black', 'random', 'fibonacci', 'norun', 'disc', 'disc-noise', 'stack', 'outside']


def test_the_cases_cover_what_they_are_meant_to(results):
    res, R = results
    assert sorted(res) == sorted(CASE_NAMES)
    S = 1 + 3 * EDGE_W
    assert 2048 <= R * S <= 65535 and (R + 1) * S > 16384 >= R * S       # a few KiB to a few tens of KiB: the builder's 16 KiB
    assert layout(R, EDGE_W) == (R, 1) and layout(R + 1, EDGE_W) == (R, 2) and layout(2 * R + 2, EDGE_W) == (R, 3)
    assert layout(33, 65) == (33, 1) and layout(64, 96)[1] >= 2 and layout(7, 1) == (7, 1)
    _, fib = fibonacci_pixels(FIB_ROWS * 3 * EDGE_W)
    img = to8b(res['fibonacci']['frames'][0]).reshape(-1)
    assert FIB_ROWS <= R and img.min() >= 1 and (img[1:] != img[:-1]).all()      # one segment, no run: the literals are the bytes
    counts = np.bincount(np.concatenate([img, np.zeros(FIB_ROWS, np.uint8)]), minlength=256).tolist() + [1]      # filter bytes, end of block
    print(f'Fibonacci case: {len(fib)} terms; an unrestricted code over {sorted(c for c in counts if c)} is {huffman_depth(counts)} bits deep')
    assert sorted(c for c in counts if c)[:len(fib)] == fib and huffman_depth(counts) > 15
    rows = np.concatenate([np.zeros((20, 1), np.uint8), to8b(res['norun']['frames'][0]).reshape(20, 90)], 1).reshape(-1)
    assert (rows[1:] != rows[:-1]).all()                                 # under filter 0 no byte repeats: no run, no distance code
    assert not to8b(res['black']['frames']).any() and res['black']['frames'].shape[1] > R
    for W in (85, 86, 87, 173):                                          # under filter 0 a row is the filter byte and a run of 3 W
        assert {85: 254, 86: 257, 87: 260, 173: 518}[W] == 3 * W - 1     # bytes behind the run's literal: 254, 257, 258 + 2, 2 x 258 + 2


@pytest.mark.parametrize('name', CASE_NAMES)
@pytest.mark.parametrize('filt', FILTERS)
def test_every_file_is_a_png_of_the_frame(results, tmp_path, name, filt):
    from efficient_nerf_amd import blender
    Image = pytest.importorskip('PIL.Image')
    res, _ = results
    frames = res[name]['frames']
    n, H, W, _ = frames.shape
    want = to8b(frames)
    for k, data in enumerate(res[name]['files'][filt]):
        ch = chunks(data)
        tags = [t for t, _ in ch]
        assert tags[0] == b'IHDR' and struct.unpack('>IIBBBBB', ch[0][1]) == (W, H, 8, 2, 0, 0, 0)
        assert tags[1:-1] == [b'IDAT'] * layout(H, W)[1]                 # one chunk per segment
        stream = b''.join(b for t, b in ch if t == b'IDAT')
        assert stream[0] == 0x78 and (stream[0] * 256 + stream[1]) % 31 == 0
        raw = zlib.decompress(stream)                                    # checks the Adler-32 as well
        assert len(raw) == H * (1 + 3 * W)
        rows = np.frombuffer(raw, np.uint8).reshape(H, 1 + 3 * W)
        fr = filtered_rows(want[k])
        choice = np.full(H, filt) if filt >= 0 else min_sum_choice(want[k])
        assert np.array_equal(rows[:, 0], choice), (rows[:, 0], choice)
        assert np.array_equal(rows[:, 1:], fr[choice, np.arange(H)])
        path = str(tmp_path / f'{k}.png')
        with open(path, 'wb') as f:
            f.write(data)
        assert np.array_equal(blender.read_png(path), want[k])
        im = Image.open(io.BytesIO(data))
        assert im.size == (W, H) and im.mode == 'RGB' and np.array_equal(np.asarray(im.convert('RGB')), want[k])


def test_file_sizes(results):
    res, _ = results
    N = 64 * (1 + 3 * 96)
    for f in FILTERS:
        white, rand = len(res['white']['files'][f][0]), len(res['random']['files'][f][0])
        print(f'filter {f}: white {white} bytes, random {rand} bytes of {N}')
        assert white < N / 50       # 258 bytes per length / distance pair: the segments' headers dominate
        assert rand <= 1.02 * N + 128      # stored: 5 bytes per block, 12 per chunk


@pytest.mark.parametrize('name', ['disc', 'disc-noise'])
def test_adaptive_file_is_no_larger_than_the_host_writers(results, tmp_path, name):
    """The host writer is the parent's frontend.write_png (filter 0, zlib level 6).  Measured on an MI355X at 96 x 128: 4,401 bytes against 8,006
    without noise (0.550 x) and 5,342 against 8,118 with noise of sigma 0.01 (0.658 x); under forced filters 0 .. 4: 8,001 5,590 5,549 5,734 4,328 and
    8,101 5,934 5,987 6,032 5,380."""
    from efficient_nerf_amd import frontend as fe
    res, _ = results
    path = str(tmp_path / 'host.png')
    fe.write_png(path, to8b(res[name]['frames'][0]))
    host, ours = os.path.getsize(path), len(res[name]['files'][-1][0])
    print(f'{name} 96 x 128: {ours} bytes on the device, {host} through frontend.write_png: {ours / host:.3f} x; forced filters: '
          f'{[len(res[name]["files"][f][0]) for f in range(5)]}')
    assert ours <= host


def test_same_bytes_every_time_and_frames_are_independent(results):
    from efficient_nerf_amd import png
    res, _ = results
    frames = res['stack']['frames']
    dev = torch.from_numpy(frames).cuda()
    for f in (-1, 0, 4):
        assert png.encode_png(dev, f) == res['stack']['files'][f]
        for k in range(3):
            assert png.encode_png(dev[k:k + 1], f) == [res['stack']['files'][f][k]]
    old, png.ENCODE_CHUNK_BYTES = png.ENCODE_CHUNK_BYTES, 1               # one frame per library call: the chunked path
    try:
        assert png.encode_png(dev, -1) == res['stack']['files'][-1]
    finally:
        png.ENCODE_CHUNK_BYTES = old
    assert len(set(res['stack']['files'][-1])) == 3


def test_nan_and_values_outside_the_unit_interval(pkg, built_lib, tmp_path):
    from efficient_nerf_amd import blender
    from efficient_nerf_amd.png import write_pngs
    f = np.full((1, 3, 4, 3), 0.5, np.float32)
    f[0, 0, 0] = (np.nan, -0.5, 1.5)
    f[0, 2, 3] = (np.inf, -np.inf, 1.0)
    path = str(tmp_path / 'n.png')
    assert write_pngs([path], torch.from_numpy(f).cuda()) == os.path.getsize(path)
    img = blender.read_png(path)
    assert img[0, 0].tolist() == [0, 0, 255] and img[2, 3].tolist() == [255, 0, 255] and (np.delete(img.reshape(-1, 3), [0, 11], 0) == 127).all()


def test_bad_arguments_are_refused(pkg, built_lib):
    import ctypes as C
    from efficient_nerf_amd import _lib
    L = _lib.lib()
    EINVAL = L.r2l_mjpeg_tables(0, (C.c_ubyte * 64)(), (C.c_ubyte * 64)())
    H, W = 16, 24
    pitch, need = L.r2l_png_max_frame_bytes(H, W), L.r2l_png_workspace_bytes(2, H, W)
    frames = torch.rand(2, H, W, 3, device='cuda')
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    out = torch.full((2, pitch), 7, dtype=torch.uint8, device='cuda')
    sizes = torch.full((2,), -1, dtype=torch.int64, device='cuda')

    def enc(**k):
        a = dict(H=H, W=W, filter=-1, need=need, pitch=pitch)
        a.update(k)
        return L.r2l_png_encode(C.c_void_p(frames.data_ptr()), 2, a['H'], a['W'], a['filter'], C.c_void_p(ws.data_ptr()), a['need'],
                                C.c_void_p(out.data_ptr()), a['pitch'], C.c_void_p(sizes.data_ptr()), None)

    for kw, word in ((dict(H=0), 'H=0'), (dict(W=-1), 'W=-1'), (dict(filter=5), 'filter = 5'), (dict(pitch=pitch - 1), 'pitch'),
                     (dict(need=need - 1), 'workspace')):
        assert enc(**kw) == EINVAL
        assert word in L.r2l_last_error().decode()
    torch.cuda.synchronize()
    assert (out == 7).all() and (sizes == -1).all()                      # nothing was launched
    assert enc() == 0
    torch.cuda.synchronize()
    assert (sizes > 0).all() and (sizes <= pitch).all()


# ---- the command lines ----
def decoded(folder):
    from efficient_nerf_amd import blender
    return {f: blender.read_png(os.path.join(folder, f)) for f in sorted(os.listdir(folder)) if f.endswith('.png')}


def write_scene(root, splits, side=16):
    """a Blender-layout scene: opaque RGBA PNGs, a smooth function of the ray"""
    import json
    from efficient_nerf_amd import frontend as fe
    from oracle import r2l_oracle as O
    angle = O.LEGO_CAMERA_ANGLE_X
    focal = O.focal_from_angle(side, angle)
    k = 0
    for split, count in splits:
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for i in range(count):
            c2w = O.pose_spherical(-180. + 47. * k, -30. + 5. * (k % 3), 4.)
            k += 1
            ro, rd = O.get_rays(side, side, focal, c2w[:3, :4])
            rgb = 0.5 + 0.4 * torch.sin(2 * rd + ro + torch.tensor([0., 1., 2.]))
            img = torch.cat([rgb, torch.ones_like(rgb[..., :1])], -1).reshape(side, side, 4)
            fe.write_png(os.path.join(root, split, f'r_{i}.png'), fe.to8b(img.numpy()))
            frames.append(dict(file_path=f'./{split}/r_{i}', transform_matrix=c2w.tolist()))
        with open(os.path.join(root, f'transforms_{split}.json'), 'w') as fp:
            json.dump(dict(camera_angle_x=angle, frames=frames), fp)


def without_times(text, *folders):
    for d in folders:
        text = text.replace(str(d), '<dir>')
    return [re.sub(r'\d+\.\d+(e[+-]\d+)?( rays/s|s\b| ms)', 'T', ln) for ln in text.splitlines()]


def test_render_only_writes_the_same_pictures_with_the_flag(pkg, tmp_path, capsys, monkeypatch):
    from efficient_nerf_amd import frontend as fe
    monkeypatch.setattr(fe, 'PNG_FRAMES_PER_CALL', 2)                    # three frames in batches of two: two encode calls, the last one short
    from oracle import r2l_oracle as O
    ck = str(tmp_path / 'r2l.tar')
    fe.save_checkpoint(ck, O.make_r2l_state(seed=4, netdepth=6))
    scene = str(tmp_path / 'scene')
    write_scene(scene, (('test', 3),), side=20)
    base = ['--model_name', 'R2L', '--config', os.path.join(ROOT, 'configs', 'lego_noview.txt'), '--datadir', scene, '--n_sample_per_ray', '16',
            '--netwidth', '256', '--netdepth', '6', '--use_residual', '--trial.ON', '--trial.body_arch', 'resmlp', '--pretrained_ckpt', ck,
            '--render_only', '--render_test', '--testskip', '1', '--precision', 'fp16x3', '--frames_per_batch', '2']
    logs = {}
    for tag, extra in (('plain', []), ('device', ['--png_device'])):
        assert fe.main(base + ['--outdir', str(tmp_path / tag)] + extra) == 0
        logs[tag] = capsys.readouterr().out
    plain, device = decoded(tmp_path / 'plain'), decoded(tmp_path / 'device')
    assert sorted(os.listdir(tmp_path / 'plain')) == sorted(os.listdir(tmp_path / 'device'))
    assert sorted(plain) == ['000.png', '000_gt.png', '001.png', '001_gt.png', '002.png', '002_gt.png']
    for f in plain:
        assert np.array_equal(plain[f], device[f]), f
        assert open(tmp_path / 'plain' / f, 'rb').read() != open(tmp_path / 'device' / f, 'rb').read()      # other bytes: the device wrote them
        assert len(chunks(open(tmp_path / 'device' / f, 'rb').read())) >= 3
    assert open(tmp_path / 'plain' / 'rgbs.npy', 'rb').read() == open(tmp_path / 'device' / 'rgbs.npy', 'rb').read()
    assert np.array_equal(plain['001.png'], fe.to8b(np.load(tmp_path / 'device' / 'rgbs.npy')[1]))
    assert without_times(logs['plain'], tmp_path / 'plain') == without_times(logs['device'], tmp_path / 'device')


def same_checkpoint(a, b):
    a, b = (torch.load(p, map_location='cpu', weights_only=False) for p in (a, b))
    assert set(a) == set(b) and a['global_step'] == b['global_step']
    n = 0
    for key in a:
        if key.startswith('network') and a[key] is not None:
            assert list(a[key]) == list(b[key])
            for k in a[key]:
                assert torch.equal(a[key][k], b[key][k]), (key, k)
                n += 1
    for k, st in a['optimizer_state_dict']['state'].items():
        for name, v in st.items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(b['optimizer_state_dict']['state'][k][name])), (k, name)
    assert n


def test_student_test_renders_are_the_same_pictures_with_the_flag(pkg, tmp_path):
    from efficient_nerf_amd import convert_data as CD, frontend as fe, train as T
    scene = str(tmp_path / 'scene')
    write_scene(scene, (('train', 16), ('test', 2)))                      # 16 views of 16 x 16: one shard of 4,096 rays
    assert CD.convert(CD.parse_args(['--splits', 'train', '--datadir', scene, '--full_res', '--seed', '1']), log=lambda *a: None)
    base = ['--model_name', 'R2L', '--dataset_type', 'blender', '--white_bkgd', '--testskip', '1', '--n_sample_per_ray', '4', '--multires', '3',
            '--netdepth', '6', '--netwidth', '64', '--use_residual', '--trial.ON', '--trial.body_arch', 'resmlp', '--basedir', str(tmp_path),
            '--datadir', scene, '--datadir_kd', f'{scene}_real_train', '--data_mode', 'rays', '--N_rand', '1', '--N_iters', '6', '--i_testset', '3',
            '--i_weights', '6', '--i_print', '3']
    logs, ckpt = {}, {}
    for tag, extra in (('plain', []), ('device', ['--png_device'])):
        torch.manual_seed(11)
        np.random.seed(11)
        logs[tag] = []
        ckpt[tag] = T.train(fe.parse_args(base + ['--expname', tag] + extra), log=lambda *a: logs[tag].append(' '.join(map(str, a))))
    same_checkpoint(ckpt['plain'], ckpt['device'])
    for it in (3, 6):
        plain, device = decoded(tmp_path / 'plain' / f'testset_iter{it}'), decoded(tmp_path / 'device' / f'testset_iter{it}')
        assert sorted(plain) == sorted(device) == ['000.png', '001.png']
        for f in plain:
            assert np.array_equal(plain[f], device[f]), (it, f)
            assert len(chunks(open(tmp_path / 'device' / f'testset_iter{it}' / f, 'rb').read())) >= 3
    key = lambda ln: re.sub(r'(data_time|batch_time|Time) \S+', '', ln).replace(str(tmp_path / 'device'), str(tmp_path / 'plain'))
    assert [key(ln) for ln in logs['device']] == [key(ln) for ln in logs['plain']]


def test_teacher_training_is_untouched_by_the_flag(pkg, tmp_path):
    """the teacher's test pass writes no pictures (train_teacher.eval_test_split returns the two PSNRs), so the flag has nothing to encode
    there: the run prints the same lines and ends on the same bits"""
    from efficient_nerf_amd import frontend as fe, train_teacher as TT
    scene = str(tmp_path / 'scene')
    write_scene(scene, (('train', 4), ('val', 1), ('test', 1)), side=32)
    base = ['--config', os.path.join(ROOT, 'configs', 'lego.txt'), '--datadir', scene, '--basedir', str(tmp_path), '--N_rand', '64', '--testskip', '1',
            '--netdepth', '4', '--netwidth', '64', '--netdepth_fine', '4', '--netwidth_fine', '64', '--N_samples', '16', '--N_importance', '16',
            '--multires', '4', '--multires_views', '2', '--precrop_iters', '0', '--i_print', '5', '--i_weights', '10', '--i_testset', '5', '--N_iters', '10',
            '--i_video', '1000']
    logs, ckpt = {}, {}
    for tag, extra in (('plain', []), ('device', ['--png_device'])):
        torch.manual_seed(5)
        np.random.seed(5)
        logs[tag] = []
        ckpt[tag] = TT.train(fe.parse_args(base + ['--expname', tag] + extra), log=lambda *a: logs[tag].append(' '.join(map(str, a))))
    same_checkpoint(ckpt['plain'], ckpt['device'])
    assert any(ln.startswith('[TEST]') for ln in logs['plain'])
    files = lambda tag: sorted(os.path.relpath(os.path.join(d, f), tmp_path / tag) for d, _, fs in os.walk(tmp_path / tag) for f in fs)
    assert files('plain') == files('device') and not [f for f in files('device') if f.endswith('.png')]
    key = lambda ln: re.sub(r'(data_time|batch_time|Time) \S+', '', ln).replace(str(tmp_path / 'device'), str(tmp_path / 'plain'))
    assert [key(ln) for ln in logs['device']] == [key(ln) for ln in logs['plain']]
