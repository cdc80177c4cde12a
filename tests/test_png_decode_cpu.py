"""CPU: the PNG decoder without a device.  csrc/png_inflate.h, the text the device runs, is built with its own main
(tools/png_decode_asan_main.cpp, `make asan_png_decode`: AddressSanitizer + UBSan, host code only) and run ONCE over every stream of
tests/png_decode_cases.py, well-formed and broken, in buffers of exactly the sizes the decoder is told: no sanitizer report, the bytes
of zlib.decompress for every stream that is a picture, a non-zero status for every other one.  Then: the flag on the four command
lines, the two entry points in the header and the binding, and bad arguments refused before a device is touched."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import png_decode_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('r2l_png_decode_workspace_bytes', 'r2l_png_decode')


def all_cases():
    """[(name, H, W, C, stream, want or None)]"""
    cases = []
    for H, W in K.SHAPES:
        for ch in (1, 2, 3, 4):
            img = K.pixels(H, W, ch, 100 * H + W + ch)
            for mode in K.FILTER_MODES:
                raw = K.filtered(img, mode, H + W)
                cases.append((f'shape-{H}x{W}x{ch}-{mode}', H, W, ch, K.compress(raw), raw))
    streams, raw = K.deflate_streams()
    cases += [(f'deflate-{name}', *K.BIG, s, raw) for name, s in streams.items()]
    cases += [(f'hand-{name}', *K.HAND, s, raw) for name, (s, raw, _) in K.hand_streams().items()]
    broken, _, _ = K.broken_streams()
    cases += [(f'broken-{name}', H, W, ch, s, None) for name, (H, W, ch, s, _) in broken.items()]
    return cases


def test_the_streams_are_what_they_are_meant_to_be():
    """zlib is the judge of the streams before the decoder sees them"""
    streams, raw = K.deflate_streams()
    assert len(raw) == 67730 and len(streams) == 10 and len(streams['level0']) > 67730 and zlib.decompress(streams['wbits9']) == raw
    assert streams['wbits9'][0] >> 4 == 1                                  # a 512-byte window in the header
    for name, (s, want, crossing) in K.hand_streams().items():
        assert zlib.decompress(s) == want and len(want) == 200 * 201, name
        if name == 'dynamic-crossing-run':
            assert crossing and crossing[0][0] in (16, 17, 18)             # one repeat code over the end of the literal / length lengths
    broken, good, raw = K.broken_streams()
    assert zlib.decompress(good) == raw and len(broken) == 27
    for name, (H, W, ch, s, accepted) in broken.items():
        if accepted:
            got = zlib.decompress(s)
            assert len(got) != H * (W * ch + 1) or max(got[::W * ch + 1]) > 4, name
        else:
            with pytest.raises(zlib.error):
                zlib.decompress(s)


def test_the_decoder_under_asan_ubsan(tmp_path):
    r = subprocess.run(['make', '-C', os.path.join(ROOT, 'efficient-nerf_amd', 'csrc'), 'asan_png_decode'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    cases = all_cases()
    with open(tmp_path / 'manifest.txt', 'w') as mf:
        for name, H, W, ch, s, _ in cases:
            mf.write(f'{name} {H} {W} {ch}\n')
            with open(tmp_path / f'{name}.z', 'wb') as f:
                f.write(s)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([os.path.join(ROOT, 'tests', '_build', 'png_decode_asan'), str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    log = r.stdout + r.stderr
    assert r.returncode == 0 and 'AddressSanitizer' not in log and 'runtime error' not in log and 'LeakSanitizer' not in log, log[-3000:]
    got = {t[0]: (int(t[1]), int(t[2], 16)) for t in (ln.split() for ln in r.stdout.splitlines())}
    assert sorted(got) == sorted(c[0] for c in cases)
    statuses = {}
    for name, H, W, ch, s, want in cases:
        status, adler = got[name]
        if want is None:
            assert status != 0, name
            statuses[name] = status
            continue
        assert status == 0, (name, status)
        assert adler == zlib.adler32(want) & 0xffffffff, name
        assert open(tmp_path / f'{name}.raw', 'rb').read() == want == zlib.decompress(s), name
        if name.startswith('shape-'):                                      # ... and the filters undone give the picture back
            img = K.pixels(H, W, ch, 100 * H + W + ch)
            assert open(tmp_path / f'{name}.px', 'rb').read() == img.tobytes(), name
    # the causes, by the enum of include/r2l_hip.h
    header = open(os.path.join(ROOT, 'include', 'r2l_hip.h')).read()
    code = {m.group(1): int(m.group(2)) for m in re.finditer(r'R2L_PNG_([A-Z_]+) = (\d+)', header)}
    for word in ('TRUNCATED', 'BAD_HEADER', 'BAD_BLOCK', 'BAD_STORED', 'OVERSUBSCRIBED', 'INCOMPLETE', 'BAD_CODE', 'FAR_DISTANCE', 'TOO_LONG',
                 'TOO_SHORT', 'BAD_FILTER', 'BAD_ADLER'):
        assert word in code, word
    want = {'cut-header': 'TRUNCATED', 'adler': 'BAD_ADLER', 'block-type-3': 'BAD_BLOCK', 'stored-nlen': 'BAD_STORED', 'far-distance': 'FAR_DISTANCE',
            'oversubscribed': 'OVERSUBSCRIBED', 'incomplete': 'INCOMPLETE', 'row-short': 'TOO_SHORT', 'row-long': 'TOO_LONG', 'filter-5': 'BAD_FILTER',
            'fdict': 'BAD_HEADER'}
    for name, word in want.items():
        assert statuses[f'broken-{name}'] == code[word], (name, statuses[f'broken-{name}'])
    assert all(v == code['TRUNCATED'] for k, v in statuses.items() if k.startswith('broken-cut-'))


def test_png_read_device_flag_on_the_four_command_lines(pkg):
    from efficient_nerf_amd import convert_data as CD, create_data as CR, frontend as fe
    assert fe.parse_args([]).png_read_device is False                      # main.py and train_teacher.py share this table
    assert fe.parse_args(['--png_read_device']).png_read_device is True
    assert fe.parse_args(['--model_name', 'nerf', '--png_device', '--png_read_device']).png_read_device is True
    assert CD.parse_args(['--splits', 'train', '--datadir', 'x']).png_read_device is False
    assert CD.parse_args(['--splits', 'train', '--datadir', 'x', '--png_read_device']).png_read_device is True
    base = ['--create_data', 'rand', '--teacher_ckpt', 'x.tar', '--datadir_kd', 'a:b']
    assert CR.parse_args(base)[1].png_read_device is False
    assert CR.parse_args(base + ['--png_read_device'])[1].png_read_device is True
    for script in ('main.py', 'train_teacher.py', 'convert_data.py', 'create_data.py'):
        assert os.path.exists(os.path.join(ROOT, script)), script


def test_header_and_binding_name_the_entry_points(pkg, built_lib):
    from efficient_nerf_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'r2l_hip.h')).read()
    for name in ENTRY_POINTS:
        assert re.search(r'^(int|long long)\s+' + name + r'\(', header, re.M), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.SIGNATURES['r2l_png_decode'][0] is C.c_int and len(_lib.SIGNATURES['r2l_png_decode'][1]) == 11
    assert _lib.SIGNATURES['r2l_png_decode_workspace_bytes'] == (C.c_longlong, [C.c_int] * 4)
    makefile = open(os.path.join(ROOT, 'efficient-nerf_amd', 'csrc', 'Makefile')).read()
    assert 'r2l_png_decode.hip' in re.search(r'^SRCS\s*:=(.*)$', makefile, re.M).group(1)


def test_bad_arguments_are_refused_on_the_host(pkg, built_lib):
    from efficient_nerf_amd import _lib
    L = _lib.lib()
    EINVAL = -1

    def refused(rc, word):
        assert rc == EINVAL and word in L.r2l_last_error().decode(), (rc, L.r2l_last_error())

    refused(L.r2l_png_decode_workspace_bytes(-1, 8, 8, 3), 'n_img = -1')
    refused(L.r2l_png_decode_workspace_bytes(1, 0, 8, 3), 'H=0')
    refused(L.r2l_png_decode_workspace_bytes(1, 8, 16385, 3), 'W=16385')
    refused(L.r2l_png_decode_workspace_bytes(1, 8, 8, 5), 'C = 5')
    assert L.r2l_png_decode_workspace_bytes(0, 8, 8, 3) == 0
    need = L.r2l_png_decode_workspace_bytes(2, 16, 24, 3)
    assert need >= 2 * 16 * (24 * 3 + 1) and need % 16 == 0
    assert L.r2l_png_decode_workspace_bytes(1, 16384, 16384, 4) >= 16384 * (16384 * 4 + 1)
    fake = C.c_void_p(1 << 20)                                           # never dereferenced: every refusal comes before a device is touched

    def dec(**k):
        a = dict(z=fake, off=fake, n=2, H=16, W=24, C=3, ws=fake, need=need, out=fake, status=fake)
        a.update(k)
        return L.r2l_png_decode(a['z'], a['off'], a['n'], a['H'], a['W'], a['C'], a['ws'], a['need'], a['out'], a['status'], None)

    refused(dec(n=-1), 'n_img = -1')
    refused(dec(H=0), 'H=0')
    refused(dec(W=-3), 'W=-3')
    refused(dec(C=5), 'C = 5')
    refused(dec(C=0), 'C = 0')
    refused(dec(z=None), 'NULL')
    refused(dec(off=None), 'NULL')
    refused(dec(ws=None), 'NULL')
    refused(dec(out=None), 'NULL')
    refused(dec(status=None), 'NULL')
    refused(dec(need=need - 1), 'workspace')
    refused(dec(ws=C.c_void_p((1 << 20) + 8)), 'alignment')
    refused(dec(off=C.c_void_p((1 << 20) + 4)), 'alignment')
    assert dec(n=0, z=None, off=None, ws=None, out=None, status=None) == 0      # nothing to do


def test_decode_pngs_refuses_on_the_host(pkg, tmp_path):
    """what png.decode_pngs decides before it needs a device: the files' own faults, in read_png's words, and two shapes in one call"""
    from efficient_nerf_amd import blender, png
    raw = K.filtered(K.pixels(5, 3, 3, 1), 0)
    good = K.png_file(5, 3, 3, K.compress(raw))
    other = K.png_file(3, 5, 3, K.compress(K.filtered(K.pixels(3, 5, 3, 1), 0)))
    bad = {'signature': b'\x89PNX' + good[4:], 'no-ihdr': K.SIG + good[33:], 'sixteen': K.png_file(5, 3, 3, K.compress(raw), depth=16),
           'interlaced': K.png_file(5, 3, 3, K.compress(raw), interlace=1), 'palette': K.png_file(5, 3, 3, K.compress(raw), colour=3)}
    for name, data in bad.items():
        path = str(tmp_path / f'{name}.png')
        with open(path, 'wb') as f:
            f.write(data)
        with pytest.raises(ValueError) as host:
            blender.read_png(path)
        with pytest.raises(ValueError) as ours:
            png.decode_pngs([path])
        assert str(ours.value) == str(host.value) and path in str(ours.value), name
    a, b = str(tmp_path / 'a.png'), str(tmp_path / 'b.png')
    for path, data in ((a, good), (b, other)):
        with open(path, 'wb') as f:
            f.write(data)
    with pytest.raises(ValueError, match='differ in shape') as e:
        png.decode_pngs([a, a, b])
    assert a in str(e.value) and b in str(e.value)
