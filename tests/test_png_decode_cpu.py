"""CPU: the PNG decoder without a device.  csrc/png_inflate.h, the text the device runs, is built with its own main
(tools/png_decode_asan_main.cpp, `make asan_png_decode`: AddressSanitizer + UBSan, host code only) and run ONCE over every stream of
tests/png_decode_cases.py, well-formed and broken, in buffers of exactly the sizes the decoder is told: no sanitizer report, the bytes
of zlib.decompress for every stream that is a picture, a non-zero status for every other one, and the one status it is built to give
for every refusal that is built to give one.  What the streams laid out on purpose reach (codes longer than the lookup tables, the
turns of the ring, the longest flushes, the fetches of the stream, the promised refusals, the filters' branches) is computed from
their symbols and asserted, group by group.  Then: the flag on the four command
lines, the two entry points in the header and the binding, and bad arguments refused before a device is touched."""
import collections
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
    cases += [(f'built-{name}', H, W, ch, s, raw) for name, (H, W, ch, s, raw, _) in K.built_streams().items()]
    good, bad = K.refill_streams()
    cases += [(f'refill-{total}', *K.REFILL, s, raw) for total, (s, raw) in good.items()]
    cases += [(f'refill-{name}', *K.REFILL, s, None) for name, (s, _) in bad.items()]
    promised, _, raw = K.promised_streams()
    cases += [(f'promised-{name}', *K.SMALL, s, raw if K.PROMISED[name] == 'OK' else None) for name, s in promised.items()]
    cases += [(f'card-{k}', *K.CARD, broken, None) for k, (_, _, broken, _) in enumerate(K.card_streams()) if broken]
    return cases


def exact_statuses():
    """{case name: status word} of the refusals that are built to give one status"""
    out = {f'refill-{name}': word for name, (_, word) in K.refill_streams()[1].items()}
    out.update({f'card-{k}': word for k, (_, _, broken, word) in enumerate(K.card_streams()) if broken})
    out.update({f'promised-{name}': word for name, word in K.PROMISED.items() if word != 'OK'})
    return out


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


def test_the_long_code_stream_covers_the_walk_and_the_symbol_tables():
    """group 1: codes of every length from 1 to 15 in both alphabets, so the table's edge, the first walked length and the last; all 29
    length and 30 distance symbols at least twice, their extra bits all 0 and all 1"""
    H, W, ch, stream, raw, blocks = K.built_streams()['long-codes']
    assert zlib.decompress(stream) == raw and len(raw) == H * (W * ch + 1) and max(raw) <= 4
    for _, ll, dd, _ in blocks:                                            # complete codes with a member of every length
        for lens in (ll, dd):
            assert sum(2 ** (15 - v) for v in lens if v) == 2 ** 15 and set(lens) - {0} == set(range(1, 16))
    ll_bits, d_bits, len_uses, dist_uses = K.code_coverage(blocks)
    assert {K.PNG_LBITS, K.PNG_LBITS + 1, 15} <= ll_bits and {K.PNG_DBITS, K.PNG_DBITS + 1, 15} <= d_bits
    assert ll_bits == d_bits == set(range(1, 16))
    for i in range(29):
        ones = (1 << K.LEN_EXTRA[i]) - 1
        assert len_uses[(i, 0)] >= 1 and len_uses[(i, ones)] >= 1 and len_uses[(i, 0)] + (len_uses[(i, ones)] if ones else 0) >= 2, i
    for j in range(30):
        ones = (1 << K.DIST_EXTRA[j]) - 1
        assert dist_uses[(j, 0)] >= 1 and dist_uses[(j, ones)] >= 1 and dist_uses[(j, 0)] + (dist_uses[(j, ones)] if ones else 0) >= 2, j
    assert K.LEN_BASE[27] + 31 == 258 and len_uses[(27, 31)] and len_uses[(28, 0)]      # 258 in both spellings
    assert dist_uses[(29, 8191)] and K.DIST_BASE[29] + 8191 == 32768


def test_the_ring_streams_cover_the_turns_and_the_flushes():
    """group 2: at each multiple of the ring's size, matches of 3 and of 258 whose destination and whose source lie across it, that end
    on it and that start on it; distances 1, below the length, 32768 and 32767; flushes of PNG_FLUSH, + 257 and + 258 bytes"""
    source = open(os.path.join(ROOT, 'efficient-nerf_amd', 'csrc', 'png_inflate.h')).read()
    for name in ('PNG_FLUSH', 'PNG_WIN', 'PNG_LBITS', 'PNG_DBITS'):        # the mirrored constants are the decoder's
        assert int(re.search(r'constexpr \w+ %s = (\d+);' % name, source).group(1)) == getattr(K, name), name
    assert K.PNG_INW_BYTES == 4 * int(re.search(r'constexpr unsigned PNG_INW = (\d+);', source).group(1))
    built = K.built_streams()
    H, W, ch = K.RING
    n = H * (W * ch + 1)
    assert n == 204800 == 3 * K.PNG_WIN + 8192
    hits, classes = set(), {}
    for v in range(4):
        _, _, _, stream, raw, blocks = built[f'ring-{v}']
        assert zlib.decompress(stream) == raw and len(raw) == n and max(raw) <= 4 and len(set(raw)) == 5
        symbols = blocks[0][1]
        h, c = K.ring_coverage(symbols)
        hits |= h
        for how, which in c.items():
            classes.setdefault(how, set()).update(which)
        sizes = K.flush_sizes(symbols)
        assert {K.PNG_FLUSH, K.PNG_FLUSH + 257, K.PNG_FLUSH + 258} <= set(sizes) and max(sizes) == K.PNG_FLUSH + 258, (v, sorted(set(sizes)))
        # the longest flushes end in a match of 258 at distance 32768
        ends = dict(K.flushes(symbols))
        assert ends[K.PNG_FLUSH + 257] == ends[K.PNG_FLUSH + 258] == (258, 32768)
    assert hits == {(mark, how, length) for mark in K.RING_MARKS for how in ('dest-across', 'source-across', 'ends-on', 'starts-on')
                    for length in (3, 258)}
    for how in ('dest-across', 'ends-on', 'starts-on'):
        assert classes[how] >= set(K.RING_CLASSES), how
    assert classes['source-across'] >= {'32768', '32767', 'other'}         # a source the match runs into does not lie across anything
    # the mixed blocks: stored, fixed, dynamic with codes of 15 bits, dynamic with codes of 3
    _, _, _, stream, raw, blocks = built['mixed-blocks']
    assert zlib.decompress(stream) == raw and len(raw) == n and max(raw) <= 4
    assert [b[0] for b in blocks] == ['stored', 'fixed', 'dynamic', 'dynamic'] and len(blocks[0][1]) == K.MIXED_STORED
    fixed, first, second = (K.sources(b[-1], start) for b, start in zip(blocks[1:], K.MIXED_EDGES))
    assert any(d == 32768 and op - d + ln <= K.MIXED_STORED for op, ln, d in fixed)
    assert any(d == 32768 and op - d + ln <= K.MIXED_STORED and op < K.PNG_WIN < op + ln for op, ln, d in fixed)
    assert any(op - d + ln <= K.MIXED_STORED for op, ln, d in first) and any(K.MIXED_EDGES[0] <= op - d < K.MIXED_EDGES[1] for op, ln, d in first)
    assert any(op < 2 * K.PNG_WIN < op + ln for op, ln, d in first) and any(op < 3 * K.PNG_WIN < op + ln for op, ln, d in second)
    assert max(blocks[2][1]) == max(blocks[2][2]) == 15 and max(blocks[3][1]) == 3 and max(blocks[3][2]) == 2
    ll_bits, d_bits, _, _ = K.code_coverage(blocks[2:3])
    assert max(ll_bits) == 15                                              # the first dynamic block's longest code is used: its end of block


def test_the_refill_streams_end_around_the_fetches():
    """group 3: good streams of every length PNG_INW_BYTES k + r, k = 1 and 2, r = -4 .. 5; cuts, an Adler-32 bit and a far distance
    behind the first fetch"""
    good, bad = K.refill_streams()
    H, W, ch = K.REFILL
    assert sorted(good) == [K.PNG_INW_BYTES * k + r for k in (1, 2) for r in range(-4, 6)]
    for k in (1, 2):
        assert {(K.PNG_INW_BYTES * k + r) % 4 for r in range(-4, 6)} == {0, 1, 2, 3}
    for total, (stream, raw) in good.items():
        assert len(stream) == total and zlib.decompress(stream) == raw and len(raw) == H * (W * ch + 1) and max(raw) <= 4, total
    base = good[2 * K.PNG_INW_BYTES + 5][0]
    assert sorted(bad) == sorted(['cut-8190', 'cut-8191', 'cut-8192', 'cut-8193', 'cut-8194', 'cut-16384', 'adler-bit', 'far-distance'])
    for name, (stream, word) in bad.items():
        with pytest.raises(zlib.error):
            zlib.decompress(stream)
        if name.startswith('cut-'):
            assert stream == base[:int(name[4:])] and word == 'TRUNCATED'
    assert sum(x != y for x, y in zip(bad['adler-bit'][0], base)) == 1 and bad['adler-bit'][0][:-4] == base[:-4]
    # the far distance: the first match of its stream, behind 8300 literals of a byte each, in a picture of fewer bytes than the distance
    far = zlib.decompressobj()
    with pytest.raises(zlib.error, match='too far back'):
        far.decompress(bad['far-distance'][0])
    assert H * (W * ch + 1) < 32768 and len(zlib.decompressobj().decompress(bad['far-distance'][0][:K.PNG_INW_BYTES])) > 8000


def test_the_promised_refusals_are_what_zlib_refuses():
    """group 4: one small stream per refusal of png_inflate.h's header comment, and the streams that have to pass next to them"""
    promised, good, raw = K.promised_streams()
    H, W, ch = K.SMALL
    assert zlib.decompress(good) == raw and len(raw) == H * (W * ch + 1) and sorted(promised) == sorted(K.PROMISED)
    assert set(K.PROMISED.values()) <= set(K.STATUS_WORDS) and len(promised) == 29
    for name, stream in promised.items():
        if K.PROMISED[name] == 'OK':
            assert zlib.decompress(stream) == raw, name
        elif name in K.ZLIB_TAKES:                                         # the stream is fine, the picture is a byte too long
            assert len(zlib.decompress(stream)) == len(raw) + 1, name
        else:
            with pytest.raises(zlib.error):
                zlib.decompress(stream)
    header = open(os.path.join(ROOT, 'include', 'r2l_hip.h')).read()
    code = {m.group(1): int(m.group(2)) for m in re.finditer(r'R2L_PNG_([A-Z_]+) = (\d+)', header)}
    assert code == {word: k for k, word in enumerate(K.STATUS_WORDS)}


def test_the_pictures_reach_every_branch_of_paeth_and_average():
    """group 5: the pictures of SHAPES under filters 3 and 4 take every branch of the two filters that can be taken on row 0, on the
    first pixel of a row, on the first row of a band of 64, and anywhere"""
    reach = K.reachable_branches()
    assert reach['row-0'] == {'paeth-a', 'tie-ab', 'avg-odd'} and reach['first-pixel'] == {'paeth-a', 'paeth-b', 'tie-ab', 'avg-odd'}
    got = set()
    for H, W in K.SHAPES:
        for ch in (1, 2, 3, 4):
            img = K.pixels(H, W, ch, 100 * H + W + ch)
            for mode in (3, 4):
                got |= K.filter_branches(img, K.row_choice(img, mode, H + W))
    assert got == {(branch, place) for place in K.PLACES for branch in reach[place]}


def test_the_card_streams_are_600_pictures_and_86_refusals():
    """group 6: more one-wave workgroups than run at once (each holds about 77 KiB of LDS, a compute unit has 160 KiB, an MI355X 256 of
    them: 512), every picture another one; every 7th has a broken twin for the call that reports statuses"""
    card = K.card_streams()
    H, W, ch = K.CARD
    assert len(card) == K.CARD_FILES == 600 and len({img.tobytes() for _, img, _, _ in card}) == 600
    assert [k for k, c in enumerate(card) if c[2]] == list(range(3, 600, 7))
    assert collections.Counter(c[3] for c in card if c[2]) == {'TRUNCATED': 22, 'BAD_ADLER': 22, 'BAD_HEADER': 21, 'TOO_SHORT': 21}
    for k, (good, img, broken, word) in enumerate(card):
        assert K.filtered(img, K.FILTER_MODES[k % 7], k) == zlib.decompress(good), k
        if word == 'TOO_SHORT':                                            # a stream that is fine for a picture that is not
            assert len(zlib.decompress(broken)) == (H - 1) * (W * ch + 1), k
        elif broken:
            with pytest.raises(zlib.error):
                zlib.decompress(broken)


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
    exact = exact_statuses()
    assert len(exact) == 8 + 27 + 86
    for name, word in exact.items():
        assert statuses[name] == code[word], (name, statuses[name], word)


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
