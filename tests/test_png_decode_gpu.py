"""GPU: the PNG decoder (csrc/png_inflate.h in csrc/r2l_png_decode.hip behind png.decode_pngs) and --png_read_device behind the loaders.

The files are written here with zlib and struct (tests/png_decode_cases.py); the judges are zlib.decompress, which accepts every
stream before the device sees it, blender.read_png, and the pictures the files were made from; every comparison is array_equal.  The
unfilter kernel walks bands of 64 rows in tiles of 64 steps: heights 63, 64, 65 and 129 and widths 63, 64 and 65 lie around both.  The
broken streams have all been through the same text on the CPU under the sanitizers (test_png_decode_cpu.py); here they are tests of a
refusal by bounds-checked code.  The streams laid out on purpose (codes of up to 15 bits and every length and distance symbol, matches
around every turn of the ring and the longest flushes, streams that end around a fetch of 8 KiB, the refusals png_inflate.h promises,
600 files in one call) go through decode_pngs and through the C-ABI call, and a refusal has to be the one status the CPU run gave."""
import ctypes as C
import os
import shutil
import struct
import zlib

import numpy as np
import pytest
import torch

import png_decode_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def save(folder, name, data):
    path = os.path.join(str(folder), name)
    with open(path, 'wb') as f:
        f.write(data)
    return path


def decode(sources):
    from efficient_nerf_amd import png
    out = png.decode_pngs(sources)
    assert out.is_cuda and out.dtype == torch.uint8
    return out.cpu().numpy()


def refiltered(px, types):
    """the filtered bytes of a picture under the given row types: equal to a stream's bytes exactly when px is that stream's picture"""
    H = px.shape[0]
    return np.concatenate([np.asarray(types, np.uint8)[:, None], K.residuals(px)[np.asarray(types), np.arange(H)]], 1).tobytes()


def decode_streams(streams, H, W, ch):
    """the C-ABI call itself: (pictures uint8 [n, H, W, ch] on the host, status list)"""
    from efficient_nerf_amd import _lib
    L = _lib.lib()
    n = len(streams)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    z = torch.from_numpy(np.frombuffer(b''.join(streams) + b'\0', np.uint8).copy()).cuda()
    off = torch.from_numpy(offsets).cuda()
    need = L.r2l_png_decode_workspace_bytes(n, H, W, ch)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    out = torch.full((n, H, W, ch), 0xee, dtype=torch.uint8, device='cuda')
    guard = torch.full((4096,), 0x5a, dtype=torch.uint8, device='cuda')
    status = torch.full((n,), -7, dtype=torch.int32, device='cuda')
    _lib.check(L.r2l_png_decode(C.c_void_p(z.data_ptr()), C.c_void_p(off.data_ptr()), n, H, W, ch, C.c_void_p(ws.data_ptr()), need,
                                C.c_void_p(out.data_ptr()), C.c_void_p(status.data_ptr()), _lib.current_stream()))
    torch.cuda.synchronize()
    assert (guard == 0x5a).all()
    return out.cpu().numpy(), status.cpu().tolist()


@pytest.mark.parametrize('H,W', K.SHAPES)
def test_shapes_channels_and_filters(pkg, built_lib, tmp_path, H, W):
    from efficient_nerf_amd import blender
    for ch in (1, 2, 3, 4):
        img = K.pixels(H, W, ch, 100 * H + W + ch)
        paths = []
        for mode in K.FILTER_MODES:
            raw = K.filtered(img, mode, H + W)
            stream = K.compress(raw)
            assert zlib.decompress(stream) == raw
            paths.append(save(tmp_path, f'{ch}-{mode}.png', K.png_file(H, W, ch, stream)))
        got = decode(paths)
        assert got.shape == (len(paths), H, W, ch)
        for k, mode in enumerate(K.FILTER_MODES):
            assert np.array_equal(got[k], img), (ch, mode)
        for k in (5, 6):                                                   # the mixed and the minimum-sum rows: the host reader as well
            assert np.array_equal(got[k], blender.read_png(paths[k])), (ch, K.FILTER_MODES[k])
    if (H, W) == (33, 7):                                                  # the cases do hold every type on row 0 and both kinds of bytes
        assert sorted(set(K.row_choice(img, 'mix', H + W).tolist())) == [0, 1, 2, 3, 4] and len(set(K.row_choice(img, 'min').tolist())) > 1


@pytest.fixture(scope='module')
def big():
    """the 130 x 130 RGBA picture, its filtered bytes and its deflate streams"""
    streams, raw = K.deflate_streams()
    H, W, ch = K.BIG
    for s in streams.values():
        assert zlib.decompress(s) == raw
    return K.pixels(H, W, ch, 5), raw, streams


def test_deflate_streams_and_chunkings(pkg, built_lib, tmp_path, big):
    from efficient_nerf_amd import blender
    img, raw, streams = big
    H, W, ch = K.BIG
    files = {name: K.png_file(H, W, ch, s) for name, s in streams.items()}
    for step in (1, 7, 8192):
        files[f'idat-{step}'] = K.png_file(H, W, ch, streams['level6'], idat_bytes=step)
    files['ancillary'] = K.png_file(H, W, ch, streams['level9'], before=((b'tEXt', b'Comment\0a test'), (b'gAMA', struct.pack('>I', 45455))))
    assert len(raw) == 67730 and len(streams['level0']) > 65535 + 5 and files['idat-1'].count(b'IDAT') >= len(streams['level6'])
    paths = [save(tmp_path, f'{name}.png', data) for name, data in files.items()]
    got = decode(paths)
    for k, name in enumerate(files):
        assert np.array_equal(got[k], img), name
    assert np.array_equal(blender.read_png(paths[-1]), img)
    assert np.array_equal(decode([files['rle'], files['level0']]), np.stack([img, img]))      # bytes instead of paths


def test_hand_assembled_streams(pkg, built_lib, tmp_path):
    from efficient_nerf_amd import blender
    H, W, ch = K.HAND
    hand = K.hand_streams()
    assert sorted(hand) == ['dynamic-crossing-run', 'dynamic-one-distance', 'len258-dist1', 'len258-dist32768', 'len3-dist2']
    paths = []
    for name, (stream, raw, crossing) in hand.items():
        assert zlib.decompress(stream) == raw and len(raw) == H * (W + 1)  # zlib first
        assert crossing is None or (len(crossing) == 1 and crossing[0][0] == 17)
        paths.append(save(tmp_path, f'{name}.png', K.png_file(H, W, ch, stream)))
    got = decode(paths)
    for k, (name, (stream, raw, _)) in enumerate(hand.items()):
        assert refiltered(got[k], np.frombuffer(raw, np.uint8)[::W + 1]) == raw, name
    assert np.array_equal(got[0], blender.read_png(paths[0]))


def test_committed_fixtures_and_the_projects_writers(pkg, built_lib, tmp_path, golden_dir):
    from efficient_nerf_amd import blender, frontend as fe, png
    for folder in (os.path.join(golden_dir, 'convert', 'scene', 'train'), os.path.join(golden_dir, 'llff', 'scene', 'images_8')):
        paths = [os.path.join(folder, f) for f in sorted(os.listdir(folder)) if f.endswith('.png')]
        assert len(paths) >= 5
        got = decode(paths)
        for k, p in enumerate(paths):
            assert np.array_equal(got[k], blender.read_png(p)), p
    frames = torch.from_numpy(K.pixels(40, 52, 3, 8).astype(np.float32) / 255.).cuda()[None]
    want = fe.to8b(frames[0].cpu().numpy())
    files = [png.encode_png(frames, f)[0] for f in (-1, 0, 1, 2, 3, 4)]
    host = save(tmp_path, 'host.png', b'')
    fe.write_png(host, want)
    got = decode(files + [host])
    for k in range(len(files) + 1):
        assert np.array_equal(got[k], want), k


def test_batches(pkg, built_lib, tmp_path, big):
    from efficient_nerf_amd import png
    img, raw, streams = big
    H, W, ch = K.BIG
    flat = np.full((H, W, ch), 200, np.uint8)
    noise = np.random.default_rng(2).integers(0, 256, (H, W, ch)).astype(np.uint8)
    pics = [img, flat, noise, img, flat, noise, img, flat, noise]
    levels = [0, 0, 0, 9, 9, 9, 1, 6, 6]
    modes = ['min', 0, 0, 4, 2, 'mix', 1, 3, 'min']
    files = [K.png_file(H, W, ch, K.compress(K.filtered(p, m, k), lv)) for k, (p, lv, m) in enumerate(zip(pics, levels, modes))]
    sizes = [len(f) for f in files]
    assert max(sizes) > 100 * min(sizes)                                   # very different amounts of work per workgroup
    together = decode(files)
    for k, f in enumerate(files):
        alone = decode([f])                                                # n = 1
        assert alone.shape == (1, H, W, ch) and np.array_equal(alone[0], pics[k]) and np.array_equal(together[k], pics[k]), k
    assert np.array_equal(decode(files), together)                         # the same bytes every time
    other = K.png_file(5, 3, 3, K.compress(K.filtered(K.pixels(5, 3, 3, 1), 0)))
    a, b = save(tmp_path, 'a.png', files[0]), save(tmp_path, 'b.png', other)
    with pytest.raises(ValueError, match='differ in shape') as e:
        png.decode_pngs([a, b])
    assert a in str(e.value) and b in str(e.value)
    assert png.decode_pngs([]).shape[0] == 0


def test_broken_files_are_refused_by_name_and_disturb_nothing(pkg, built_lib, tmp_path):
    from efficient_nerf_amd import png
    broken, good, raw = K.broken_streams()
    H, W, ch = 33, 7, 4
    img = K.pixels(H, W, ch, 9)
    assert len(broken) == 27 and zlib.decompress(good) == raw
    # one call of the library: every broken stream between two good ones
    streams = [good]
    for s in broken.values():
        streams += [s[3], good]
    out, status = decode_streams(streams, H, W, ch)
    assert all(st != 0 for st in status[1::2]), status
    assert all(st == 0 for st in status[0::2]), status
    for k in range(0, len(streams), 2):
        assert np.array_equal(out[k], img), k
    # ... and through decode_pngs: the file's name, then the next call as if nothing had been
    ok = save(tmp_path, 'ok.png', K.png_file(H, W, ch, good))
    for name, (_, _, _, s, _) in broken.items():
        path = save(tmp_path, f'{name}.png', K.png_file(H, W, ch, s))
        with pytest.raises(ValueError) as e:
            png.decode_pngs([ok, path, ok])
        assert str(e.value).startswith(path + ': '), (name, str(e.value))
    assert np.array_equal(decode([ok, ok]), np.stack([img, img]))
    # what the host refuses, in read_png's words
    raw0 = K.compress(K.filtered(img, 0))
    bad = {'signature': b'\x89PNX' + K.png_file(H, W, ch, raw0)[4:], 'no-ihdr': K.SIG + K.png_file(H, W, ch, raw0)[33:],
           'sixteen': K.png_file(H, W, ch, raw0, depth=16), 'interlaced': K.png_file(H, W, ch, raw0, interlace=1),
           'palette': K.png_file(H, W, ch, raw0, colour=3)}
    from efficient_nerf_amd import blender
    for name, data in bad.items():
        path = save(tmp_path, f'host-{name}.png', data)
        with pytest.raises(ValueError) as host:
            blender.read_png(path)
        with pytest.raises(ValueError) as ours:
            png.decode_pngs([ok, path])
        assert str(ours.value) == str(host.value) and path in str(ours.value), name


# ---- streams laid out on purpose (tests/png_decode_cases.py; what they reach is asserted in test_png_decode_cpu.py) ----
def status_codes():
    from efficient_nerf_amd import png
    assert sorted(png.DECODE_STATUS) == list(range(1, len(K.STATUS_WORDS)))
    return {word: k for k, word in enumerate(K.STATUS_WORDS)}


def is_picture_of(px, raw, W, ch):
    """px [H, W, ch] is what the filtered bytes `raw` reconstruct to"""
    return refiltered(px, np.frombuffer(raw, np.uint8)[::W * ch + 1]) == raw


def between_good(good, bad):
    """good[0], bad[0], good[1], bad[1], ..., good again: every broken stream between two good ones"""
    streams = []
    for k, s in enumerate(bad):
        streams += [good[k % len(good)], s]
    return streams + [good[len(bad) % len(good)]]


def test_long_codes_ring_turns_and_mixed_blocks(pkg, built_lib):
    built = K.built_streams()
    assert sorted(built) == ['long-codes', 'mixed-blocks', 'ring-0', 'ring-1', 'ring-2', 'ring-3']
    for shape in (K.HAND, K.RING):
        names = [name for name, b in built.items() if b[:3] == shape]
        H, W, ch = shape
        for name in names:
            assert zlib.decompress(built[name][3]) == built[name][4] and len(built[name][4]) == H * (W * ch + 1), name      # zlib first
        files = decode([K.png_file(H, W, ch, built[name][3], idat_bytes=8192 if k % 2 else None) for k, name in enumerate(names)])
        abi, status = decode_streams([built[name][3] for name in names], H, W, ch)
        assert status == [0] * len(names), status
        for k, name in enumerate(names):
            assert is_picture_of(files[k], built[name][4], W, ch), name
            assert np.array_equal(abi[k], files[k]), name


def test_streams_that_end_around_a_fetch_and_refusals_behind_the_first(pkg, built_lib):
    from efficient_nerf_amd import png
    good, bad = K.refill_streams()
    code = status_codes()
    H, W, ch = K.REFILL
    totals = sorted(good)
    assert totals == [K.PNG_INW_BYTES * k + r for k in (1, 2) for r in range(-4, 6)] and len(bad) == 8
    for total in totals:
        assert zlib.decompress(good[total][0]) == good[total][1] and len(good[total][0]) == total
    files = decode([K.png_file(H, W, ch, good[total][0]) for total in totals])
    for k, total in enumerate(totals):
        assert is_picture_of(files[k], good[total][1], W, ch), total
    streams = between_good([good[total][0] for total in totals], [s for s, _ in bad.values()])
    abi, status = decode_streams(streams, H, W, ch)
    assert status[1::2] == [code[word] for _, word in bad.values()], status
    assert status[0::2] == [0] * (len(bad) + 1), status
    for k in range(0, len(streams), 2):
        assert np.array_equal(abi[k], files[k // 2 % len(totals)]), k
    for name, (stream, word) in bad.items():
        with pytest.raises(ValueError) as e:
            png.decode_pngs([K.png_file(H, W, ch, good[totals[0]][0]), K.png_file(H, W, ch, stream)])
        assert str(e.value) == f'<bytes #1>: {png.DECODE_STATUS[code[word]]}', (name, str(e.value))


def test_promised_refusals_give_their_status(pkg, built_lib):
    from efficient_nerf_amd import png
    promised, good, raw = K.promised_streams()
    code = status_codes()
    H, W, ch = K.SMALL
    assert zlib.decompress(good) == raw and sorted(promised) == sorted(K.PROMISED) and len(promised) == 29
    want = decode([K.png_file(H, W, ch, good)])[0]
    assert is_picture_of(want, raw, W, ch)
    streams = between_good([good], list(promised.values()))
    abi, status = decode_streams(streams, H, W, ch)
    assert status[1::2] == [code[K.PROMISED[name]] for name in promised], list(zip(promised, status[1::2]))
    assert status[0::2] == [0] * (len(promised) + 1), status
    for k, st in enumerate(status):
        if st == 0:
            assert np.array_equal(abi[k], want), k
    # through decode_pngs: the refusal in the status' words, and the streams that pass
    ok = K.png_file(H, W, ch, good)
    for name, stream in promised.items():
        if K.PROMISED[name] == 'OK':
            assert np.array_equal(decode([ok, K.png_file(H, W, ch, stream), ok]), np.stack([want] * 3)), name
        else:
            with pytest.raises(ValueError) as e:
                png.decode_pngs([ok, K.png_file(H, W, ch, stream), ok])
            assert str(e.value) == f'<bytes #1>: {png.DECODE_STATUS[code[K.PROMISED[name]]]}', (name, str(e.value))


def test_more_workgroups_than_run_at_once(pkg, built_lib):
    card = K.card_streams()
    code = status_codes()
    H, W, ch = K.CARD
    assert len(card) == 600
    pictures = np.stack([img for _, img, _, _ in card])
    assert np.array_equal(decode([K.png_file(H, W, ch, good) for good, _, _, _ in card]), pictures)
    abi, status = decode_streams([broken or good for good, _, broken, _ in card], H, W, ch)
    assert status == [code[word] if broken else 0 for _, _, broken, word in card]
    assert sum(st != 0 for st in status) == 86
    keep = np.array(status) == 0
    assert np.array_equal(abi[keep], pictures[keep])


# ---- the loaders ----
def write_scene(root, counts, side):
    """a Blender-layout scene of RGBA files with a real alpha channel, rows under mixed filters"""
    import json
    k = 0
    for split, count in counts:
        os.makedirs(os.path.join(root, split), exist_ok=True)
        frames = []
        for i in range(count):
            img = K.pixels(side, side + 2, 4, 50 + k)
            save(os.path.join(root, split), f'r_{i}.png', K.png_file(side, side + 2, 4, K.compress(K.filtered(img, 'mix' if k % 2 else 'min', k))))
            pose = np.eye(4)
            pose[:3, 3] = (0.1 * k, -0.2 * k, 4.)
            frames.append(dict(file_path=f'./{split}/r_{i}', transform_matrix=pose.tolist()))
            k += 1
        with open(os.path.join(root, f'transforms_{split}.json'), 'w') as fp:
            json.dump(dict(camera_angle_x=0.6911112070083618, frames=frames), fp)


def test_load_blender_data_with_the_device_reader(pkg, built_lib, tmp_path):
    from efficient_nerf_amd import blender, png
    scene = str(tmp_path / 'scene')
    write_scene(scene, (('train', 3), ('val', 2), ('test', 4)), side=18)
    calls = []
    reader = png.device_reader()

    def counted(paths):
        calls.append(len(paths))
        return reader(paths)

    for half in (False, True):
        host = blender.load_blender_data(scene, half_res=half, testskip=2)
        del calls[:]
        dev = blender.load_blender_data(scene, half_res=half, testskip=2, decode=counted)
        assert calls == [3, 1, 2]                                          # one call per split
        assert dev[0].dtype == host[0].dtype == torch.float32 and not dev[0].is_cuda and dev[0].shape[-1] == 4
        assert torch.equal(dev[0], host[0]) and torch.equal(dev[1], host[1]) and dev[2] == host[2]
        assert all(np.array_equal(a, b) for a, b in zip(dev[3], host[3]))


def test_llff_load_scene_with_the_device_reader(pkg, built_lib, golden_dir):
    from efficient_nerf_amd import llff, png
    base = os.path.join(golden_dir, 'llff', 'scene')
    host, dev = llff.load_scene(base), llff.load_scene(base, decode=png.device_reader())
    assert dev.bytes.dtype == np.uint8 and np.array_equal(dev.bytes, host.bytes) and np.array_equal(dev.images, host.images)
    assert np.array_equal(dev.poses, host.poses) and np.array_equal(dev.bds, host.bds) and np.array_equal(dev.render_poses, host.render_poses)
    assert dev.hwf == host.hwf and dev.i_test == host.i_test


def test_convert_data_writes_the_same_shards_with_the_flag(pkg, built_lib, golden_dir, tmp_path):
    from efficient_nerf_amd import convert_data as CD
    written = {}
    for tag, extra in (('plain', []), ('device', ['--png_read_device'])):
        scene = str(tmp_path / tag / 'scene')
        shutil.copytree(os.path.join(golden_dir, 'convert', 'scene'), scene)
        lines = []
        paths = CD.convert(CD.parse_args(['--splits', 'train', '--datadir', scene, '--seed', '1234'] + extra), log=lines.append)
        written[tag] = ([os.path.basename(p) for p in paths], [open(p, 'rb').read() for p in paths], [ln.replace(str(tmp_path / tag), '') for ln in lines])
    assert written['plain'][0] and written['plain'] == written['device']
