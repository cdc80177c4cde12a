"""GPU: the Motion-JPEG encoder (csrc/r2l_mjpeg.hip behind video.encode_jpeg) and --write_video on the three command lines.

The yardsticks are in tests/jpeg_baseline.py, written from T.81: the encoder's arithmetic in float64 and a baseline decoder that reads
its tables from the file itself.

Shapes: 8 x 8 (one block, prediction from 0), 9 x 17 (replicate padding both ways, 2 x 3 blocks in raster order), 30 x 40 x 3 frames (the
LLFF fixture's size; prediction restarts and sizes per frame), 64 x 72 (216 units: more than one wave of the scan), 136 x 264 (1,683
units: more than the SCAN_TILE = 1,024 elements a workgroup of the scan takes per round, so the carry between rounds is used), each at
quality 50, 90 and 100 on 0.5 + 0.4 sin(x / 5 + c) cos(y / 7) + 0.08 N(0, 1); and constructed frames: all 0, all 1, values outside
[0, 1], one NaN and one +inf pixel, a block that is DC + k basis(7, 7) (coefficient 63 behind 62 zeros: three ZRL, no EOB), a block of binary noise at
quality 100 (every AC coefficient non-zero; stuffed bytes), a 0 / 1 checkerboard at quality 100 (the largest AC coefficients).

1. Arithmetic: the returned coefficients equal the rounded float64 ones wherever the float64 value is farther than 0.01 from a tie (the fp32
   DCT's error is below 8e-3: |F| <= 8,192 and a few dozen roundings of 2^-24 each), differ by at most 1 elsewhere, and at most 3 % of a
   case's coefficients are that close to a tie.
2. Entropy coder, exactly: the decoder recovers the returned coefficients from every file; the scan is stuffed and padded as T.81 asks.
3. The same input gives the same bytes; a frame's bytes do not depend on the stack it is in.
4. PIL opens every frame; its decode is no farther from the 8-bit frame than PIL's own encode with the same quantisers and 4:4:4, minus
   0.1 dB.  Measured on an MI355X, PSNR through our encoder minus PSNR through PIL's: see test_pil_decodes_every_frame.
5. --render_only --write_video, and training with --i_video --write_video on both trainers, leave everything else as it was."""
import io
import os
import re
import struct

import numpy as np
import pytest
import torch

import jpeg_baseline as J

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_TILE = 1024                    # csrc/r2l_mjpeg.hip MJPEG_SCAN_TILE
SHAPES = [(1, 8, 8), (1, 9, 17), (3, 30, 40), (1, 64, 72), (1, 136, 264)]
QUALITIES = (50, 90, 100)
TIE_GUARD, TIE_SHARE = 0.01, 0.03


def natural(n, H, W, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:H, :W]
    f = np.stack([np.stack([0.5 + 0.4 * np.sin(x / 5 + c + k) * np.cos(y / 7) for c in range(3)], -1) for k in range(n)])
    return (f + 0.08 * rng.standard_normal(f.shape)).astype(np.float32)


def exact(values):
    """frames whose bytes are the given integers: floor(255 (v + 0.25) / 255) = v in float32"""
    return ((np.asarray(values, np.float64) + 0.25) / 255.).astype(np.float32)


def constructed():
    flat = natural(4, 9, 17, 7)
    flat[0], flat[1] = 0., 1.
    flat[2] = 3. * flat[2] - 1.                                   # from -1.5 to 2.5
    flat[3, 4, 5, 1], flat[3, 2, 11, 0] = np.nan, np.inf
    y, x = np.mgrid[:8, :8]
    basis = np.cos((2 * x + 1) * 7 * np.pi / 16) * np.cos((2 * y + 1) * 7 * np.pi / 16)
    b77 = exact(np.repeat(np.rint(128 + 100 * basis)[None, :, :, None], 3, -1))
    noise = exact(255 * np.random.default_rng(NOISE_SEED).integers(0, 2, (1, 8, 8, 3)))
    yy, xx = np.mgrid[:16, :24]
    checker = np.repeat(((xx + yy) % 2).astype(np.float32)[None, :, :, None], 3, -1)
    return {'flat': (flat, 90), 'basis77': (b77, 50), 'noise': (noise, 100), 'checker': (checker, 100)}


NOISE_SEED = 2                      # the first seed whose 189 float64 AC coefficients all round away from 0
CASES = {f'{H}x{W}x{n}-q{q}': (natural(n, H, W, 100 * H + q), q) for n, H, W in SHAPES for q in QUALITIES}
CASES.update(constructed())


def library_tables(q):
    import ctypes as C
    from efficient_nerf_amd import _lib
    luma, chroma = (C.c_ubyte * 64)(), (C.c_ubyte * 64)()
    assert _lib.lib().r2l_mjpeg_tables(q, luma, chroma) == 0
    return list(luma), list(chroma)


def encode(frames, q):
    """(files, coefficients int64 [n, n_blocks, 3, 64]) of a numpy stack, on the device"""
    from efficient_nerf_amd.video import encode_jpeg
    files, coef = encode_jpeg(torch.from_numpy(frames).cuda(), q, return_coef=True)
    return files, coef.cpu().numpy().astype(np.int64)


@pytest.fixture(scope='module')
def results(pkg, built_lib):
    """every case encoded once, its float64 reference and its decode: shared by the tests below, changed by none"""
    out = {}
    for name, (frames, q) in CASES.items():
        files, coef = encode(frames, q)
        pre = J.reference_coefficients(frames, *library_tables(q))
        out[name] = dict(frames=frames, q=q, files=files, coef=coef, pre=pre, dec=[J.decode(f) for f in files])
    return out


def test_the_shapes_cover_what_they_are_meant_to(pkg, built_lib):
    units = [3 * ((H + 7) // 8) * ((W + 7) // 8) for _, H, W in SHAPES]
    assert units[0] == 3 and units[3] > 64 and units[4] == 1683 > SCAN_TILE
    for name, lo in (('basis77', 50), ('noise', 100), ('checker', 100)):
        frames, q = CASES[name]
        c = J.quantise(J.reference_coefficients(frames, *library_tables(q)))
        if name == 'basis77':
            assert not c[0, 0, 0, 1:63].any() and c[0, 0, 0, 63] != 0 and not c[0, 0, 1:, 1:].any()      # coefficient 63 behind 62 zeros
        if name == 'noise':
            assert (c[..., 1:] != 0).all()
        if name == 'checker':
            assert 800 < np.abs(c[..., 1:]).max() <= 1023                                                   # large, under the clamp


@pytest.mark.parametrize('name', list(CASES))
def test_coefficients_against_float64(results, name):
    r = results[name]
    want, got = J.quantise(r['pre']), r['coef']
    assert got.shape == want.shape
    near = J.tie_distance(r['pre']) <= TIE_GUARD
    near[..., 1:] &= np.abs(r['pre'][..., 1:]) < 1023.5                  # beyond the clamp a tie decides nothing
    share = near.mean()
    wrong = (got != want) & ~near
    print(f'{name}: {got.size} coefficients, {share:.2%} within {TIE_GUARD} of a tie, {int((got != want).sum())} differ from float64, '
          f'largest |AC| {np.abs(got[..., 1:]).max()}, DC {got[..., 0].min()} .. {got[..., 0].max()}')
    assert share <= TIE_SHARE
    assert not wrong.any(), f'{int(wrong.sum())} coefficients away from a tie differ, first at {np.argwhere(wrong)[0]}: {got[wrong][0]} for {r["pre"][wrong][0]}'
    assert np.abs(got - want).max() <= 1
    assert np.abs(got[..., 1:]).max() <= 1023


@pytest.mark.parametrize('name', list(CASES))
def test_scan_decodes_to_the_returned_coefficients(results, name):
    r = results[name]
    n, H, W, _ = r['frames'].shape
    luma, chroma = library_tables(r['q'])
    for k, (data, dec) in enumerate(zip(r['files'], r['dec'])):
        assert data[:2] == b'\xff\xd8' and data[-2:] == b'\xff\xd9'
        assert dec['end'] == len(data)                                   # sizes_dev: the position after the first FF D9 behind the scan
        assert (dec['H'], dec['W']) == (H, W) and dec['qt'] == {0: luma, 1: chroma}
        assert dec['markers'] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
        assert np.array_equal(dec['coef'], r['coef'][k]), f'frame {k}: first difference at {np.argwhere(dec["coef"] != r["coef"][k])[:1]}'
    if name == 'noise':
        assert r['dec'][0]['stuffed'] >= 1 and r['dec'][0]['eob'] == 0   # every unit ends on coefficient 63
    if name == 'basis77':
        assert r['dec'][0]['zrl'] == 3 and r['dec'][0]['eob'] == 2       # Y: three ZRL, no EOB; Cb, Cr: EOB alone
    print(f'{name}: {[len(f) for f in r["files"]]} bytes, {sum(d["stuffed"] for d in r["dec"])} stuffed, {sum(d["zrl"] for d in r["dec"])} ZRL')


def test_same_bytes_every_time_and_frames_are_independent(results):
    r = results['30x40x3-q90']
    again, coef = encode(r['frames'], 90)
    assert again == r['files'] and np.array_equal(coef, r['coef'])
    for k in range(3):
        alone, coef = encode(r['frames'][k:k + 1], 90)
        assert alone[0] == r['files'][k] and np.array_equal(coef[0], r['coef'][k])
    from efficient_nerf_amd import video as V
    old, V.ENCODE_CHUNK_BYTES = V.ENCODE_CHUNK_BYTES, 1               # one frame per library call: the chunked path
    try:
        assert encode(r['frames'], 90)[0] == r['files']
    finally:
        V.ENCODE_CHUNK_BYTES = old
    flat = results['flat']
    assert flat['files'][0] != flat['files'][1] and len(set(map(len, flat['files']))) > 1


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return np.inf if mse == 0 else 10 * np.log10(255. ** 2 / mse)


@pytest.mark.parametrize('name', list(CASES))
def test_pil_decodes_every_frame(results, name):
    """Measured on an MI355X, PSNR of PIL's decode of our file minus PSNR of PIL's own encode and decode, both against the 8-bit frame, dB:
    8 x 8 at quality 50 / 90 / 100: 0.000 / +0.028 / +0.822; 9 x 17: +0.053 / +0.062 / +0.301; 30 x 40, three frames: +0.018 +0.004 +0.003 /
    +0.040 -0.018 +0.018 / +0.212 +0.172 +0.255; 64 x 72: -0.004 / +0.018 / +0.170; 136 x 264: +0.004 / +0.015 / +0.188; out of range
    +0.083, NaN and inf +0.044, noise +0.792; all 0, all 1, basis (7, 7) and the checkerboard decode to the same pixels through both.  The
    worst is -0.018 dB; at quality 100 the fp32 DCT is ahead of libjpeg's integer one by 0.2 dB and more.  Every coefficient of every case
    equalled the rounded float64 one, those near a tie included, so these are the figures of the float64 arithmetic as well."""
    Image = pytest.importorskip('PIL.Image')
    r = results[name]
    n, H, W, _ = r['frames'].shape
    inv = np.argsort(J.ZZ)
    qtables = [[t[i] for i in inv] for t in library_tables(r['q'])]      # PIL takes them in natural order
    for k, data in enumerate(r['files']):
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (W, H) and im.mode == 'RGB'
        ref = J.to_bytes(r['frames'][k])
        buf = io.BytesIO()
        Image.fromarray(ref.astype(np.uint8)).save(buf, 'JPEG', qtables=qtables, subsampling=0)
        theirs = J.parse(buf.getvalue())
        assert theirs.qt == {0: library_tables(r['q'])[0], 1: library_tables(r['q'])[1]} and [s for _, s, _ in theirs.comps] == [0x11] * 3
        ours, pils = psnr(np.asarray(im), ref), psnr(np.asarray(Image.open(io.BytesIO(buf.getvalue()))), ref)
        print(f'{name} frame {k}: {ours:.3f} dB through our encoder, {pils:.3f} dB through PIL\'s, ' + ('equal' if ours == pils else f'{ours - pils:+.3f} dB'))
        assert ours >= pils - 0.1


# ---- the command lines ----
def avi_frames(path):
    """the 00dc chunks of an AVI file, through its index"""
    data = open(path, 'rb').read()
    movi = data.index(b'movi')
    idx = data.rindex(b'idx1')
    n = struct.unpack('<I', data[idx + 4:idx + 8])[0] // 16
    out = []
    for k in range(n):
        ckid, flags, off, size = struct.unpack('<4sIII', data[idx + 8 + 16 * k:idx + 24 + 16 * k])
        assert ckid == b'00dc' and data[movi + off:movi + off + 4] == b'00dc'
        out.append(data[movi + off + 8:movi + off + 8 + size])
    return out


def test_render_only_writes_the_video_and_nothing_else_changes(pkg, tmp_path, capsys):
    from efficient_nerf_amd import frontend as fe
    from efficient_nerf_amd.video import encode_jpeg
    from oracle import r2l_oracle as O
    ck = str(tmp_path / 'r2l.tar')
    fe.save_checkpoint(ck, O.make_r2l_state(seed=4, netdepth=6))
    base = ['--model_name', 'R2L', '--config', os.path.join(ROOT, 'configs', 'lego_noview.txt'), '--n_sample_per_ray', '16', '--netwidth', '256',
            '--netdepth', '6', '--use_residual', '--trial.ON', '--trial.body_arch', 'resmlp', '--pretrained_ckpt', ck, '--render_only',
            '--precision', 'fp16x3', '--synthetic_poses', '3', '--H', '36', '--W', '44']
    logs = {}
    for tag, extra in (('plain', []), ('video', ['--write_video', '--video_quality', '75'])):
        assert fe.main(base + ['--outdir', str(tmp_path / tag)] + extra) == 0
        logs[tag] = capsys.readouterr().out
    plain, video = sorted(os.listdir(tmp_path / 'plain')), sorted(os.listdir(tmp_path / 'video'))
    assert video == sorted(plain + ['video.avi']) and 'rgbs.npy' in plain and '002.png' in plain
    for f in plain:
        assert open(tmp_path / 'plain' / f, 'rb').read() == open(tmp_path / 'video' / f, 'rb').read(), f
    assert 'Save video' not in logs['plain']
    line = [ln for ln in logs['video'].splitlines() if ln.startswith('Save video: ')]
    assert len(line) == 1 and f'"{tmp_path / "video" / "video.avi"}" (3 frames, ' in line[0] and logs['video'].index('Save renders') < logs['video'].index('Save video')
    rgbs = np.load(tmp_path / 'video' / 'rgbs.npy')
    assert rgbs.shape == (3, 18, 22, 3)                                  # half_res of 36 x 44: padded both ways
    files = avi_frames(str(tmp_path / 'video' / 'video.avi'))
    want, coef = encode_jpeg(torch.from_numpy(rgbs).cuda(), 75, return_coef=True)
    assert files == want
    for k, f in enumerate(files):
        assert np.array_equal(J.decode(f)['coef'], coef[k].cpu().numpy())


def same_checkpoint(a, b):
    a, b = (torch.load(p, map_location='cpu', weights_only=False) for p in (a, b))
    assert set(a) == set(b) and a['global_step'] == b['global_step']
    n = 0
    for key in a:
        if key.startswith('network'):
            assert list(a[key]) == list(b[key])
            for k in a[key]:
                assert torch.equal(a[key][k], b[key][k]), (key, k)
                n += 1
    for k, st in a['optimizer_state_dict']['state'].items():
        for name, v in st.items():
            w = b['optimizer_state_dict']['state'][k][name]
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(w)), (k, name)
    assert n


def test_student_training_writes_videos_and_ends_on_the_same_bits(pkg, tmp_path):
    from efficient_nerf_amd import frontend as fe, train as T
    data = tmp_path / 'shards'
    data.mkdir()
    g = torch.Generator().manual_seed(3)
    for k in range(2):
        o = torch.randn(256, 3, generator=g) * 0.3 + torch.tensor([0., 0., 4.])
        d = torch.nn.functional.normalize(torch.randn(256, 3, generator=g) * 0.2 - torch.tensor([0., 0., 1.]), dim=-1)
        np.save(str(data / f'pseudo_{k}.npy'), torch.cat([o, d, torch.rand(256, 3, generator=g)], -1).numpy().astype(np.float32))
    base = ['--model_name', 'R2L', '--dataset_type', 'blender', '--n_sample_per_ray', '4', '--multires', '3', '--netdepth', '6', '--netwidth', '64',
            '--use_residual', '--trial.ON', '--trial.body_arch', 'resmlp', '--basedir', str(tmp_path), '--datadir', str(tmp_path / 'none'),
            '--datadir_kd', str(data), '--data_mode', 'rays', '--N_rand', '1', '--N_iters', '20', '--i_video', '10', '--i_testset', '0', '--i_weights', '20',
            '--i_print', '10', '--H', '18', '--W', '20', '--n_pose_video', '3,1,1']
    logs, ckpt = {}, {}
    for tag, extra in (('plain', []), ('video', ['--write_video'])):
        torch.manual_seed(11)
        np.random.seed(11)
        logs[tag] = []
        ckpt[tag] = T.train(fe.parse_args(base + ['--expname', tag] + extra), log=lambda *a: logs[tag].append(' '.join(map(str, a))))
    same_checkpoint(ckpt['plain'], ckpt['video'])
    assert not any('VIDEO' in ln or 'Rendering video' in ln for ln in logs['plain'])
    assert not [f for f in os.listdir(tmp_path / 'plain') if f.endswith('.avi')]
    key = lambda ln: re.sub(r'data_time \S+ batch_time \S+ ', '', ln).replace(str(tmp_path / 'video'), str(tmp_path / 'plain'))
    video_line = lambda ln: ln.startswith('[VIDEO]') or 'Rendering video...' in ln
    assert [key(ln) for ln in logs['video'] if not video_line(ln)] == [key(ln) for ln in logs['plain']]      # every other line as it was
    for it in (10, 20):
        path = str(tmp_path / 'video' / f'video_iter{it}.avi')
        assert f'Iter {it} Rendering video... (n_pose: 3)' in logs['video']
        assert any(ln.startswith('[VIDEO] Rendering done. Time ') and ln.endswith(f's. Save video: "{path}"') for ln in logs['video'])
        files = avi_frames(path)
        assert len(files) == 3
        for f in files:
            dec = J.decode(f)
            assert (dec['H'], dec['W']) == (18, 20)
    assert avi_frames(str(tmp_path / 'video' / 'video_iter10.avi')) != avi_frames(str(tmp_path / 'video' / 'video_iter20.avi'))      # the weights moved


def write_scene(root, n_train=4, side=32):
    """a Blender-layout scene as the teacher-training tests write it: opaque RGBA PNGs, a smooth function of the ray"""
    import json
    from efficient_nerf_amd import frontend as fe
    from oracle import r2l_oracle as O
    angle = O.LEGO_CAMERA_ANGLE_X
    focal = O.focal_from_angle(side, angle)
    k = 0
    for split, count in (('train', n_train), ('val', 1), ('test', 1)):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for i in range(count):
            c2w = O.pose_spherical(-180. + 47. * k, -30. + 5. * (k % 3), 4.)
            k += 1
            ro, rd = O.get_rays(side, side, focal, c2w[:3, :4])
            rgb = 0.2 + 0.1 * torch.sin(2 * rd + ro + torch.tensor([0., 1., 2.]))
            img = torch.cat([rgb, torch.ones_like(rgb[..., :1])], -1).reshape(side, side, 4)
            fe.write_png(os.path.join(root, split, f'r_{i}.png'), fe.to8b(img.numpy()))
            frames.append(dict(file_path=f'./{split}/r_{i}', transform_matrix=c2w.tolist()))
        with open(os.path.join(root, f'transforms_{split}.json'), 'w') as fp:
            json.dump(dict(camera_angle_x=angle, frames=frames), fp)


def test_teacher_training_writes_videos_and_ends_on_the_same_bits(pkg, tmp_path):
    from efficient_nerf_amd import frontend as fe, train_teacher as TT
    scene = str(tmp_path / 'scene')
    write_scene(scene)
    base = ['--config', os.path.join(ROOT, 'configs', 'lego.txt'), '--datadir', scene, '--basedir', str(tmp_path), '--N_rand', '64', '--testskip', '1',
            '--netdepth', '4', '--netwidth', '64', '--netdepth_fine', '4', '--netwidth_fine', '64', '--N_samples', '16', '--N_importance', '16',
            '--multires', '4', '--multires_views', '2', '--precrop_iters', '0', '--i_print', '10', '--i_weights', '20', '--i_testset', '0', '--N_iters', '20',
            '--i_video', '10', '--n_pose_video', '2,1,1', '--video_tag', 't']
    with pytest.raises(SystemExit, match='--i_video 10 falls inside this run'):
        TT.train(fe.parse_args(base + ['--expname', 'refused']), log=lambda *a: None)
    logs, ckpt = {}, {}
    for tag, extra in (('plain', ['--i_video', '1000']), ('video', ['--write_video'])):
        torch.manual_seed(5)
        np.random.seed(5)
        logs[tag] = []
        ckpt[tag] = TT.train(fe.parse_args(base + ['--expname', tag] + extra), log=lambda *a: logs[tag].append(' '.join(map(str, a))))
    same_checkpoint(ckpt['plain'], ckpt['video'])
    assert not any(ln.startswith('[VIDEO]') or 'Rendering video...' in ln for ln in logs['plain'])
    for it in (10, 20):
        path = str(tmp_path / 'video' / f'video_iter{it}_t.avi')
        assert f'Iter {it} Rendering video... (n_pose: 2)' in logs['video']
        assert any(ln.startswith('[VIDEO] Rendering done. Time ') and ln.endswith(f's. Save video: "{path}"') for ln in logs['video'])
        files = avi_frames(path)
        assert len(files) == 2 and all((J.decode(f)['H'], J.decode(f)['W']) == (16, 16) for f in files)      # half_res of the 32 x 32 scene
