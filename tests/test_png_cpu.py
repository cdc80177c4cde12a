"""CPU: what of the device PNG writer needs no device (csrc/r2l_png.hip's host-only entry points, png.py's argument checks, the
--png_device flag): the header and the binding name the four entry points, the layout arithmetic holds its own bounds, bad arguments
are refused in one line."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('r2l_png_max_frame_bytes', 'r2l_png_workspace_bytes', 'r2l_png_layout', 'r2l_png_encode')


def test_header_and_binding_name_the_entry_points(pkg, built_lib):
    from efficient_nerf_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'r2l_hip.h')).read()
    for name in ENTRY_POINTS:
        assert re.search(r'^(int|long long)\s+' + name + r'\(', header, re.M), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)
    assert _lib.SIGNATURES['r2l_png_encode'][0] is C.c_int and len(_lib.SIGNATURES['r2l_png_encode'][1]) == 11
    assert _lib.SIGNATURES['r2l_png_max_frame_bytes'][0] is C.c_longlong and _lib.SIGNATURES['r2l_png_workspace_bytes'][0] is C.c_longlong
    makefile = open(os.path.join(ROOT, 'efficient-nerf_amd', 'csrc', 'Makefile')).read()
    assert 'r2l_png.hip' in re.search(r'^SRCS\s*:=(.*)$', makefile, re.M).group(1)
    # to8b's byte is stated once, in the header both encoders include
    csrc = os.path.join(ROOT, 'efficient-nerf_amd', 'csrc')
    stated = [f for f in sorted(os.listdir(csrc)) if f.endswith(('.hip', '.h')) and 'floorf(255.0f' in open(os.path.join(csrc, f)).read()]
    assert stated == ['r2l_to8b.h']
    for f in ('r2l_mjpeg.hip', 'r2l_png.hip'):
        assert '#include "r2l_to8b.h"' in open(os.path.join(csrc, f)).read()


@pytest.mark.parametrize('H,W', [(1, 1), (7, 1), (1, 7), (64, 96), (800, 800), (378, 504), (3, 5461), (3, 5462), (2, 16384), (16384, 1)])
def test_layout_arithmetic(pkg, built_lib, H, W):
    from efficient_nerf_amd import _lib, png
    L = _lib.lib()
    rows, segs = png.layout(H, W)
    S = 1 + 3 * W
    assert 1 <= rows <= H and segs == -(-H // rows)
    assert rows * S <= 16384 or rows == 1                                # at most 16 KiB of filtered bytes, or one row
    assert rows == H or (rows + 1) * S > 16384                           # and no fewer rows than fit
    assert rows * S <= 65535                                             # one stored block holds a segment
    # every segment stored: signature 8, IHDR 25, per segment chunk 12 + block 5, zlib header 2, Adler 4, IEND 12
    assert L.r2l_png_max_frame_bytes(H, W) == 8 + 25 + 17 * segs + 2 + 4 + 12 + H * S
    one, three = L.r2l_png_workspace_bytes(1, H, W), L.r2l_png_workspace_bytes(3, H, W)
    assert one >= H * S + segs * (rows * S + 5) and one % 16 == 0 and one < three <= 3 * one and L.r2l_png_workspace_bytes(0, H, W) == 0


def test_bad_arguments_are_refused_on_the_host(pkg, built_lib):
    from efficient_nerf_amd import _lib
    L = _lib.lib()
    EINVAL = L.r2l_mjpeg_tables(0, (C.c_ubyte * 64)(), (C.c_ubyte * 64)())
    rows, segs = C.c_int(-5), C.c_int(-5)

    def refused(rc, word):
        assert rc == EINVAL and word in L.r2l_last_error().decode(), (rc, L.r2l_last_error())

    refused(L.r2l_png_max_frame_bytes(0, 8), 'H=0')
    refused(L.r2l_png_max_frame_bytes(8, 16385), 'W=16385')
    refused(L.r2l_png_workspace_bytes(-1, 8, 8), 'n_img = -1')
    refused(L.r2l_png_workspace_bytes(1, 8, -2), 'W=-2')
    refused(L.r2l_png_layout(0, 8, C.byref(rows), C.byref(segs)), 'H=0')
    refused(L.r2l_png_layout(8, 8, None, C.byref(segs)), 'NULL')
    assert (rows.value, segs.value) == (-5, -5)
    pitch, need = L.r2l_png_max_frame_bytes(16, 24), L.r2l_png_workspace_bytes(2, 16, 24)
    fake = C.c_void_p(1 << 20)                                           # never dereferenced: every refusal comes before a device is touched

    def enc(**k):
        a = dict(rgb=fake, n=2, H=16, W=24, filter=-1, ws=fake, need=need, out=fake, pitch=pitch, sizes=fake)
        a.update(k)
        return L.r2l_png_encode(a['rgb'], a['n'], a['H'], a['W'], a['filter'], a['ws'], a['need'], a['out'], a['pitch'], a['sizes'], None)

    refused(enc(H=0), 'H=0')
    refused(enc(W=0), 'W=0')
    refused(enc(n=-1), 'n_img = -1')
    refused(enc(filter=5), 'filter = 5')
    refused(enc(filter=-2), 'filter = -2')
    refused(enc(pitch=pitch - 1), 'pitch')
    refused(enc(need=need - 1), 'workspace')
    refused(enc(rgb=None), 'NULL')
    refused(enc(sizes=None), 'NULL')
    refused(enc(ws=C.c_void_p((1 << 20) + 8)), 'alignment')
    assert enc(n=0, rgb=None, ws=None, out=None, sizes=None) == 0        # nothing to do


def test_png_device_flag(pkg):
    from efficient_nerf_amd import frontend as fe
    assert fe.parse_args([]).png_device is False
    assert fe.parse_args(['--png_device']).png_device is True
    assert fe.parse_args(['--model_name', 'nerf', '--png_device', '--write_video']).png_device is True


def test_encode_png_refuses_in_one_line(pkg):
    import torch
    from efficient_nerf_amd import png
    with pytest.raises(ValueError, match=r'^encode_png: a float32 tensor on the GPU, got torch.float32 on cpu$'):
        png.encode_png(torch.zeros(1, 4, 4, 3))
    with pytest.raises(ValueError, match=r'^encode_png: a stack \[n, H, W, 3\], got \(4, 4, 3\)$'):
        png.encode_png(torch.zeros(4, 4, 3))
    with pytest.raises(ValueError, match=r'^encode_png: a stack \[n, H, W, 3\], got \(1, 4, 4, 4\)$'):
        png.encode_png(torch.zeros(1, 4, 4, 4))
    with pytest.raises(ValueError, match=r'^write_pngs: 2 path\(s\) for 1 frame\(s\)$'):
        png.write_pngs(['a', 'b'], torch.zeros(1, 4, 4, 3))
