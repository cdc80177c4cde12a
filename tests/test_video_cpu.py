"""CPU: the host side of --write_video (efficient-nerf_amd/video.py, the r2l_mjpeg_* entry points that need no device): the quantiser
tables against libjpeg's rule written out here, the JPEG header segment by segment against T.81's Annex K tables written out here, every
argument check, the AVI container through a RIFF walker written here, the Blender video poses against their formula, the flags."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGO = ['--config', os.path.join(ROOT, 'configs', 'lego.txt')]

# T.81 Annex K.1 / K.2, row-major
K1 = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K2 = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def zigzag():
    """zig-zag position -> (row, column), walked along the anti-diagonals (T.81 figure A.6)"""
    order = []
    for s in range(15):
        diag = [(r, s - r) for r in range(8) if 0 <= s - r < 8]
        order += diag if s % 2 else diag[::-1]
    return order


ZZ = [r * 8 + c for r, c in zigzag()]

# T.81 Annex K.3.3: (BITS, HUFFVAL) of tables K.3 (DC luminance), K.5 (AC luminance), K.4 (DC chrominance), K.6 (AC chrominance)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def libjpeg_table(base, q):
    s = 5000 // q if q < 50 else 200 - 2 * q
    return [min(max((base[ZZ[i]] * s + 50) // 100, 1), 255) for i in range(64)]


def library_tables(L, q):
    luma, chroma = (C.c_ubyte * 64)(), (C.c_ubyte * 64)()
    assert L.r2l_mjpeg_tables(q, luma, chroma) == 0
    return list(luma), list(chroma)


def test_zigzag_walk_is_the_standard_s():
    assert ZZ[:12] == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25] and ZZ[-4:] == [47, 55, 62, 63] and sorted(ZZ) == list(range(64))
    for bits, vals in (DC_LUMA, DC_CHROMA, AC_LUMA, AC_CHROMA):
        assert sum(bits) == len(vals) == len(set(vals))
    assert len(AC_LUMA[1]) == len(AC_CHROMA[1]) == 162


@pytest.mark.parametrize('q', [1, 25, 50, 75, 90, 100])
def test_tables_follow_libjpeg_s_rule(pkg, built_lib, q):
    from efficient_nerf_amd import _lib
    luma, chroma = library_tables(_lib.lib(), q)
    assert luma == libjpeg_table(K1, q) and chroma == libjpeg_table(K2, q)
    if q == 100:
        assert set(luma) == set(chroma) == {1}
    if q == 50:
        assert [luma[i] for i in range(64)] == [K1[ZZ[i]] for i in range(64)]
    if q == 1:
        assert luma.count(255) == 64 and max(luma) == 255          # 16 x 50 = 800 and up: every entry is clamped


def segments(data):
    """(marker, payload) of every segment up to and including SOS, and where the scan starts"""
    assert data[:2] == b'\xff\xd8'
    at, out = 2, []
    while True:
        assert data[at] == 0xFF, f'no marker at {at}'
        marker = data[at + 1]
        n = struct.unpack('>H', data[at + 2:at + 4])[0]
        out.append((marker, data[at + 4:at + 2 + n]))
        at += 2 + n
        if marker == 0xDA:
            return out, at


@pytest.mark.parametrize('H,W,q', [(8, 8, 90), (378, 504, 50), (800, 800, 100), (65535, 1, 1)])
def test_header_parses_segment_by_segment(pkg, built_lib, H, W, q):
    from efficient_nerf_amd import _lib
    L = _lib.lib()
    buf = (C.c_ubyte * 1024)()
    n = L.r2l_mjpeg_header(H, W, q, buf, 1024)
    assert n == 623
    data = bytes(buf[:n])
    segs, end = segments(data)
    assert end == n                                                                          # SOS is last
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    assert segs[0][1] == b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])                      # 1.01, no units, 1:1, no thumbnail
    luma, chroma = library_tables(L, q)
    assert segs[1][1] == bytes([0]) + bytes(luma) and segs[2][1] == bytes([1]) + bytes(chroma)       # 8-bit tables 0 and 1, zig-zag order
    assert segs[3][1] == struct.pack('>BHHB', 8, H, W, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for (marker, payload), (tc_th, (bits, vals)) in zip(segs[4:8], ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA))):
        assert payload == bytes([tc_th]) + bytes(bits) + bytes(vals)
    assert segs[8][1] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert L.r2l_mjpeg_max_frame_bytes(H, W) >= n + 2


def test_argument_checks(pkg, built_lib):
    """R2L_EINVAL with its line, before a device is looked for (this box has none)"""
    from efficient_nerf_amd import _lib
    L = _lib.lib()
    EINVAL = L.r2l_mjpeg_tables(0, (C.c_ubyte * 64)(), (C.c_ubyte * 64)())
    assert EINVAL < 0

    def refused(rc, words):
        msg = L.r2l_last_error().decode()
        assert rc == EINVAL and words in msg and '\n' not in msg, (rc, msg)
    t64, buf = (C.c_ubyte * 64)(), (C.c_ubyte * 1024)()
    refused(L.r2l_mjpeg_tables(0, t64, t64), 'quality = 0')
    refused(L.r2l_mjpeg_tables(101, t64, t64), 'quality = 101')
    refused(L.r2l_mjpeg_tables(90, None, t64), 'NULL')
    refused(L.r2l_mjpeg_header(0, 8, 90, buf, 1024), 'H=0')
    refused(L.r2l_mjpeg_header(8, 65536, 90, buf, 1024), 'W=65536')
    refused(L.r2l_mjpeg_header(8, 8, 0, buf, 1024), 'quality = 0')
    refused(L.r2l_mjpeg_header(8, 8, 90, None, 1024), 'NULL')
    refused(L.r2l_mjpeg_header(8, 8, 90, buf, 622), 'the header takes 623')
    refused(L.r2l_mjpeg_workspace_bytes(1, 0, 8), 'H=0')
    refused(L.r2l_mjpeg_workspace_bytes(-1, 8, 8), 'n_img = -1')
    refused(L.r2l_mjpeg_max_frame_bytes(8, 70000), 'W=70000')
    pitch, need = L.r2l_mjpeg_max_frame_bytes(16, 24), L.r2l_mjpeg_workspace_bytes(2, 16, 24)
    assert pitch == 623 + 2 * 208 * 18 + 2 and need > 0 and need % 16 == 0
    p = C.c_void_p(4096)          # never dereferenced: every call below is refused first
    enc = lambda **k: L.r2l_mjpeg_encode(*[k.get(name, default) for name, default in (
        ('rgb', p), ('n', 2), ('H', 16), ('W', 24), ('q', 90), ('ws', p), ('ws_bytes', need), ('out', p), ('pitch', pitch), ('sizes', p), ('coef', None),
        ('stream', None))])
    refused(enc(rgb=None), 'the frame stack is NULL')
    refused(enc(ws=None), 'workspace / out / sizes is NULL')
    refused(enc(out=None), 'workspace / out / sizes is NULL')
    refused(enc(sizes=None), 'workspace / out / sizes is NULL')
    refused(enc(H=0), 'H=0')
    refused(enc(W=0), 'W=0')
    refused(enc(H=65536), 'H=65536')
    refused(enc(W=65536), 'W=65536')
    refused(enc(q=0), 'quality = 0')
    refused(enc(q=101), 'quality = 101')
    refused(enc(n=-1), 'n_img = -1')
    refused(enc(pitch=pitch - 1), f'a pitch of {pitch - 1} bytes')
    refused(enc(ws_bytes=need - 1), f'a workspace of {need - 1} bytes')
    refused(enc(coef=C.c_void_p(4098)), 'alignment')
    refused(enc(ws=C.c_void_p(4100)), 'alignment')
    assert enc(n=0) == 0                                                                     # nothing to do, nothing touched


# ---- the container ----
def riff_walk(data):
    """Every chunk of an AVI file as (path, offset of its data, size); asserts that each declared size fits its parent exactly"""
    found = []

    def walk(at, end, path):
        while at < end:
            fourcc, size = data[at:at + 4], struct.unpack('<I', data[at + 4:at + 8])[0]
            assert at + 8 + size <= end, f'{path}/{fourcc} runs past its parent'
            if fourcc in (b'RIFF', b'LIST'):
                kind = data[at + 8:at + 12]
                found.append((path + '/' + kind.decode(), at + 12, size - 4))
                walk(at + 12, at + 8 + size, path + '/' + kind.decode())
            else:
                found.append((path + '/' + fourcc.decode(), at + 8, size))
            at += 8 + size + (size & 1)
        assert at == end, f'{path} ends at {at}, declared {end}'
    walk(0, len(data), '')
    return found


def fake_jpeg(n, seed):
    assert n >= 4
    return b'\xff\xd8' + bytes(np.random.default_rng(seed).integers(0, 255, n - 4, dtype=np.uint8)) + b'\xff\xd9'


@pytest.mark.parametrize('fps', [30, 24, 7.5])
def test_mjpeg_writer_container(pkg, tmp_path, fps):
    from efficient_nerf_amd.video import MJPEGWriter
    frames = [fake_jpeg(n, k) for k, n in enumerate((101, 64, 7, 1000, 333))]               # odd and even lengths
    path = str(tmp_path / 'v.avi')
    w = MJPEGWriter(path, 30, 40, fps=fps)
    for f in frames:
        w.add(f)
    w.close()
    data = open(path, 'rb').read()
    chunks = riff_walk(data)
    names = [c[0] for c in chunks]
    assert names == ['/AVI ', '/AVI /hdrl', '/AVI /hdrl/avih', '/AVI /hdrl/strl', '/AVI /hdrl/strl/strh', '/AVI /hdrl/strl/strf', '/AVI /movi'] + \
        ['/AVI /movi/00dc'] * len(frames) + ['/AVI /idx1']
    assert struct.unpack('<I', data[4:8])[0] == len(data) - 8
    at = {n: (o, s) for n, o, s in chunks if not n.endswith('00dc')}
    avih = struct.unpack('<14I', data[at['/AVI /hdrl/avih'][0]:][:56])
    assert avih[0] == round(1e6 / fps) and avih[3] == 0x10 and avih[4] == len(frames) and avih[6] == 1
    assert avih[7] == max(map(len, frames)) and avih[8:10] == (40, 30)
    o, s = at['/AVI /hdrl/strl/strh']
    assert s == 56
    strh = struct.unpack('<4s4sIHHIIIIIIII4H', data[o:o + 56])
    assert strh[:2] == (b'vids', b'MJPG') and strh[9] == len(frames) and strh[7] / strh[6] == fps and strh[-2:] == (40, 30)
    if fps == int(fps):
        assert (strh[6], strh[7]) == (1, fps)
    o, s = at['/AVI /hdrl/strl/strf']
    assert s == 40
    bih = struct.unpack('<IiiHH4sIiiII', data[o:o + 40])
    assert bih[:6] == (40, 40, 30, 1, 24, b'MJPG')
    movi = at['/AVI /movi'][0] - 4                                                           # the 'movi' fourcc
    o, s = at['/AVI /idx1']
    assert s == 16 * len(frames)
    for k, f in enumerate(frames):
        ckid, flags, off, size = struct.unpack('<4sIII', data[o + 16 * k:o + 16 * k + 16])
        assert (ckid, flags, size) == (b'00dc', 0x10, len(f))
        assert data[movi + off:movi + off + 4] == b'00dc' and struct.unpack('<I', data[movi + off + 4:movi + off + 8])[0] == len(f)
        assert data[movi + off + 8:movi + off + 8 + len(f)] == f
        if len(f) & 1:
            assert data[movi + off + 8 + len(f)] == 0                                        # the pad byte
    frame_chunks = [(o_, s_) for n, o_, s_ in chunks if n.endswith('00dc')]
    assert [s_ for _, s_ in frame_chunks] == [len(f) for f in frames]


def test_mjpeg_writer_refusals(pkg, tmp_path):
    from efficient_nerf_amd.video import MJPEGWriter
    path = str(tmp_path / 'none.avi')
    with pytest.raises(ValueError, match='has no frame'):
        MJPEGWriter(path, 8, 8).close()
    assert not os.path.exists(path)
    path = str(tmp_path / 'big.avi')
    w = MJPEGWriter(path, 8, 8, size_limit=2000)
    w.add(fake_jpeg(1000, 0))
    with pytest.raises(ValueError, match='would pass 2000 bytes') as e:
        w.add(fake_jpeg(1000, 1))
    assert '\n' not in str(e.value) and not os.path.exists(path)
    with pytest.raises(ValueError):
        w.add(fake_jpeg(10, 2))
    # exactly at the limit is accepted: 224 bytes of headers + movi + idx1, one frame
    one = fake_jpeg(100, 3)
    limit = 12 + 8 + 192 + 12 + 8 + 100 + 8 + 16
    for lim, ok in ((limit, True), (limit - 1, False)):
        w = MJPEGWriter(path, 8, 8, size_limit=lim)
        if ok:
            w.add(one)
            w.close()
            assert os.path.getsize(path) == limit
            os.remove(path)
        else:
            with pytest.raises(ValueError):
                w.add(one)
            assert not os.path.exists(path)


# ---- the Blender video poses ----
def pose_formula(theta, phi, radius):
    """load_blender.py's pose_spherical written as one matrix: the camera on a sphere around the origin, looking in (float64)"""
    th, ph = np.radians(theta), np.radians(phi)
    trans = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, radius], [0, 0, 0, 1.]])
    rot_phi = np.array([[1, 0, 0, 0], [0, np.cos(ph), -np.sin(ph), 0], [0, np.sin(ph), np.cos(ph), 0], [0, 0, 0, 1.]])
    rot_theta = np.array([[np.cos(th), 0, -np.sin(th), 0], [0, 1, 0, 0], [np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1.]])
    return np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1.]]) @ rot_theta @ rot_phi @ trans


def test_get_novel_poses(pkg):
    from efficient_nerf_amd.video import get_novel_poses
    got = get_novel_poses('20,4,1')
    thetas, phis, radii = np.arange(20) * 18. - 180., [-72., -54., -36., -18.], [4.]
    want = np.stack([pose_formula(t, p, r) for r in radii for p in phis for t in thetas])
    assert got.shape == (80, 4, 4) and got.dtype == np.float32
    assert np.abs(got - want).max() < 2e-6                                                   # float32 products of entries up to 4
    assert np.allclose(np.linalg.norm(got[:, :3, 3], axis=1), 4., atol=1e-5)                 # on the sphere
    assert np.array_equal(get_novel_poses(['20', '4', '1']), got)
    got = get_novel_poses('sample:5,fixed:-30,fixed:4')
    want = np.stack([pose_formula(t, -30., 4.) for t in (-180., -108., -36., 36., 108.)])
    assert got.shape == (5, 4, 4) and np.abs(got - want).max() < 2e-6
    assert np.abs(get_novel_poses(40) - np.stack([pose_formula(t, -30., 4.) for t in np.arange(40) * 9. - 180.])).max() < 2e-6
    got = get_novel_poses('fixed:10,sample:2,sample:3')
    want = np.stack([pose_formula(10., p, r) for r in (3., 4., 5.) for p in (-60., -30.)])
    assert np.abs(got - want).max() < 2e-6
    with pytest.raises(ValueError):
        get_novel_poses('20,4')


# ---- the flags ----
def test_parsers_accept_the_flags(pkg):
    from efficient_nerf_amd import frontend as fe, train_teacher as TT
    d = fe.parse_args([])
    assert (d.write_video, d.video_quality, d.video_fps) == (False, 90, 30)
    a = fe.parse_args(LEGO + ['--write_video', '--video_quality', '75', '--video_fps', '24'])       # the one parser of main.py, train.py, train_teacher.py
    assert (a.write_video, a.video_quality, a.video_fps) == (True, 75, 24)
    inside = LEGO + ['--i_video', '50', '--N_iters', '100']
    with pytest.raises(SystemExit) as e:
        TT.check_supported(fe.parse_args(inside))
    assert '--i_video 50 falls inside this run' in str(e.value)
    with pytest.raises(SystemExit) as e:
        TT.main(inside)
    assert '--i_video 50 falls inside this run' in str(e.value)
    TT.check_supported(fe.parse_args(inside + ['--write_video']))                            # lifted, and only then
    from efficient_nerf_amd.video import check_video_args, video_path
    for bad, line in ((['--video_quality', '0'], '--video_quality 0'), (['--video_quality', '101'], '--video_quality 101'),
                      (['--video_fps', '0'], '--video_fps 0')):
        with pytest.raises(SystemExit) as e:
            check_video_args(fe.parse_args(['--write_video'] + bad))
        assert line in str(e.value)
        check_video_args(fe.parse_args(bad))                                                 # without --write_video nothing is read
    assert video_path('d', fe.parse_args([])) == os.path.join('d', 'video.avi')
    assert video_path('d', fe.parse_args(['--video_tag', 'x']), it=10) == os.path.join('d', 'video_iter10_x.avi')


def test_training_video_poses(pkg, tmp_path):
    """Blender: get_novel_poses(--n_pose_video) at the run's own intrinsics, else at what the front end would render at; LLFF: the
    loader's render path at the scene's intrinsics; one line when the scene is not there"""
    from efficient_nerf_amd import frontend as fe, llff
    from efficient_nerf_amd.video import get_novel_poses, training_video_poses
    poses, hwf = training_video_poses(fe.parse_args(LEGO + ['--datadir', str(tmp_path)]), hwf=(16, 24, 20.))
    assert tuple(poses.shape) == (80, 3, 4) and hwf == (16, 24, 20.)
    assert np.array_equal(poses.numpy(), get_novel_poses('20,4,1')[:, :3, :4])
    poses, hwf = training_video_poses(fe.parse_args(['--dataset_type', 'blender', '--datadir', str(tmp_path), '--n_pose_video', 'sample:5,fixed:-30,fixed:4',
                                                     '--H', '18', '--W', '20']))
    assert tuple(poses.shape) == (5, 3, 4) and hwf[:2] == (18, 20)
    scene_dir = os.path.join(ROOT, 'tests', 'golden', 'llff', 'scene')
    args = fe.parse_args(['--config', os.path.join(ROOT, 'configs', 'fern.txt'), '--datadir', scene_dir])
    poses, hwf = training_video_poses(args)
    scene = llff.load_scene(scene_dir, args.factor, n_pose_video=llff.n_pose_video_from_flag(args.n_pose_video))
    assert np.array_equal(poses.numpy(), scene.render_poses[:, :3, :4].astype(np.float32)) and tuple(hwf) == tuple(scene.hwf) and len(poses) > 1
    with pytest.raises(SystemExit) as e:
        training_video_poses(fe.parse_args(['--dataset_type', 'llff', '--datadir', str(tmp_path)]))
    assert 'needs the scene under --datadir' in str(e.value)
