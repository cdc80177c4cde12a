"""The still images of the reference (`imageio.imwrite(filename, to8b(rgb))`, main.py:337-341) as files finished on the device: every
frame of a device stack becomes a complete PNG (csrc/r2l_png.hip: filters, deflate, Adler-32 and CRC-32 in kernels, one C-ABI call per
chunk of frames).  Frames leave the device as .png bytes, not as pixels; --png_device puts this behind the front end's writers.

And the way in: decode_pngs turns a batch of 8-bit PNG files of one shape into pixels on the device (csrc/png_inflate.h, csrc/r2l_png_decode.hip:
inflate and the row filters in kernels, one C-ABI call per batch); --png_read_device puts it behind the loaders, whose results stay what
blender.read_png gives."""
import ctypes as C
import struct

ENCODE_CHUNK_BYTES = 256 << 20  # frames per library call: as many as keep the output slots and the workspace under this, each


def _frames_per_call(n, pitch, ws_one):
    return max(1, min(n, ENCODE_CHUNK_BYTES // max(pitch, ws_one)))


def layout(H, W):
    """(rows of a segment, segments of a frame): how the encoder cuts a frame of that size"""
    from . import _lib
    rows, segs = C.c_int(), C.c_int()
    _lib.check(_lib.lib().r2l_png_layout(int(H), int(W), C.byref(rows), C.byref(segs)))
    return rows.value, segs.value


class PNGEncoder:
    """The buffers of r2l_png_encode for up to n_max frames of H x W at a time: workspace, one output slot of `pitch` bytes per frame and
    the sizes, allocated once.  launch(frames) queues the encoder on the current stream and returns device views (slots [n, pitch] uint8,
    sizes [n] int64) that the next launch overwrites; the host does not wait."""

    def __init__(self, H, W, n_max, device, filter=-1):
        import torch
        from . import _lib
        if int(filter) not in (-1, 0, 1, 2, 3, 4):
            raise ValueError(f'PNGEncoder: filter = {filter} (-1 adaptive, 0 .. 4 that type on every row)')
        self.H, self.W, self.n_max, self.filter = int(H), int(W), max(1, int(n_max)), int(filter)
        L = _lib.lib()
        self.pitch = int(L.r2l_png_max_frame_bytes(self.H, self.W))
        if self.pitch < 0:
            _lib.check(self.pitch)
        self.need = int(L.r2l_png_workspace_bytes(self.n_max, self.H, self.W))
        if self.need < 0:
            _lib.check(self.need)
        self.ws = torch.empty(self.need, dtype=torch.uint8, device=device)
        self.buf = torch.empty((self.n_max, self.pitch), dtype=torch.uint8, device=device)
        self.sizes = torch.empty(self.n_max, dtype=torch.int64, device=device)

    def launch(self, frames):
        from . import _lib
        nb = len(frames)
        if nb > self.n_max or tuple(frames.shape[1:]) != (self.H, self.W, 3):
            raise ValueError(f'PNGEncoder: built for up to {self.n_max} frames of {self.H} x {self.W} x 3, got {tuple(frames.shape)}')
        _lib.check(_lib.lib().r2l_png_encode(_lib.dptr(frames), nb, self.H, self.W, self.filter, C.c_void_p(self.ws.data_ptr()), self.need,
                                             C.c_void_p(self.buf.data_ptr()), self.pitch, C.c_void_p(self.sizes.data_ptr()),
                                             _lib.current_stream()))
        return self.buf[:nb], self.sizes[:nb]


def encode_png(frames, filter=-1):
    """frames: float32 [n, H, W, 3] on the GPU (values as the renderer leaves them: to8b's clamp happens on the device).  Returns one
    complete PNG file per frame as bytes.  filter: -1 chooses a filter type per row, 0 .. 4 forces that type on every row.  One
    r2l_png_encode call per chunk of frames on the current stream and, per chunk, one copy of the sizes and one of the used bytes."""
    import torch
    from . import _lib
    if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f'encode_png: a stack [n, H, W, 3], got {tuple(frames.shape) if hasattr(frames, "shape") else type(frames).__name__}')
    if not (frames.is_cuda and frames.dtype == torch.float32):
        raise ValueError(f'encode_png: a float32 tensor on the GPU, got {frames.dtype} on {frames.device}')
    if int(filter) not in (-1, 0, 1, 2, 3, 4):
        raise ValueError(f'encode_png: filter = {filter} (-1 adaptive, 0 .. 4 that type on every row)')
    frames = frames.contiguous()
    n, H, W = (int(v) for v in frames.shape[:3])
    L = _lib.lib()
    pitch = L.r2l_png_max_frame_bytes(H, W)
    if pitch < 0:
        _lib.check(int(pitch))
    out = []
    if n == 0:
        return out
    with torch.cuda.device(frames.device):
        enc = PNGEncoder(H, W, _frames_per_call(n, pitch, L.r2l_png_workspace_bytes(1, H, W)), frames.device, filter)
        for i0 in range(0, n, enc.n_max):
            buf, sizes = enc.launch(frames[i0:i0 + enc.n_max])
            sz = sizes.cpu()
            host = buf[:, :int(sz.max())].cpu().numpy()          # the used bytes of every slot, one copy
            out += [host[k, :int(sz[k])].tobytes() for k in range(len(sz))]
    return out


def write_pngs(paths, frames, filter=-1):
    """frames [n, H, W, 3] float32 on the GPU -> the files at paths, one per frame.  Returns the bytes written."""
    paths = list(paths)
    if len(paths) != len(frames):
        raise ValueError(f'write_pngs: {len(paths)} path(s) for {len(frames)} frame(s)')
    total = 0
    for path, data in zip(paths, encode_png(frames, filter)):
        with open(path, 'wb') as f:
            f.write(data)
        total += len(data)
    return total


# ---- the way in ----
DECODE_STATUS = {1: 'the compressed data ends early', 2: 'not a zlib stream (bad header, or a preset dictionary)', 3: 'deflate block type 3',
                 4: 'a stored block whose LEN and NLEN disagree', 5: 'over-subscribed code lengths', 6: 'incomplete code lengths',
                 7: 'bad code lengths (too many, a repeat with nothing to repeat or past the end, or no end-of-block code)',
                 8: 'bits that are no symbol of the code', 9: 'a match that starts before the first byte', 10: 'more image data than the header\'s size',
                 11: 'truncated image data', 12: 'a filter type above 4', 13: 'the Adler-32 of the data is not the stream\'s',
                 14: 'offsets that do not ascend'}      # r2l_png_status (include/r2l_hip.h)


def parse_png(data, name):
    """(H, W, C, the zlib stream) of an 8-bit non-interlaced PNG file: blender.read_png's walk over the chunks (IDAT payloads joined,
    other chunks skipped, CRCs not checked, IEND ends it) and its refusals, word for word"""
    from .blender import _CHANNELS, _PNG_SIG
    if data[:8] != _PNG_SIG:
        raise ValueError(f'{name}: not a PNG file')
    pos, idat, hdr = 8, [], None
    while pos + 8 <= len(data):
        n, tag = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat.append(body)
        elif tag == b'IEND':
            break
        pos += 12 + n
    if hdr is None:
        raise ValueError(f'{name}: no IHDR chunk')
    w, h, depth, ctype, _, _, interlace = hdr
    if depth != 8 or ctype not in _CHANNELS or interlace != 0:
        raise ValueError(f'{name}: unsupported PNG (bit depth {depth}, colour type {ctype}, interlace {interlace}); '
                         'only 8-bit gray/RGB/RGBA non-interlaced files are read')
    return h, w, _CHANNELS[ctype], b''.join(idat)


def decode_pngs(sources, device=None):
    """sources: paths or bytes of 8-bit non-interlaced PNG files (gray, gray + alpha, RGB or RGBA) of ONE shape.  Returns their pixels,
    uint8 [n, H, W, C] on the device, equal to blender.read_png's.  The host reads the files and walks the chunks; one upload of all the
    compressed streams and their offsets, one r2l_png_decode call on the current stream, one read of the status.  A file the host or the
    device refuses raises a ValueError that names it."""
    import numpy as np
    import torch
    from . import _lib
    sources = list(sources)
    names, parsed = [], []
    for k, src in enumerate(sources):
        if isinstance(src, (bytes, bytearray, memoryview)):
            name, data = f'<bytes #{k}>', bytes(src)
        else:
            name = str(src)
            with open(src, 'rb') as f:
                data = f.read()
        names.append(name)
        parsed.append(parse_png(data, name))
    for k in range(1, len(parsed)):
        if parsed[k][:3] != parsed[0][:3]:
            raise ValueError(f'decode_pngs: the files differ in shape: {names[0]} is {parsed[0][:3]}, {names[k]} is {parsed[k][:3]} (H, W, C); '
                             f'one call decodes one shape')
    if not torch.cuda.is_available():
        raise _lib.R2LError('no HIP device visible to torch: PNG decoding on the device has no CPU fallback (blender.read_png is the host reader)')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if not parsed:
        return torch.empty((0, 0, 0, 0), dtype=torch.uint8, device=dev)
    H, W, ch = parsed[0][:3]
    n = len(parsed)
    L = _lib.lib()
    need = int(L.r2l_png_decode_workspace_bytes(n, H, W, ch))
    if need < 0:
        _lib.check(need)
    # one host buffer, one copy: the offsets (int64, n + 1) in front of the streams
    sizes = np.array([len(p[3]) for p in parsed], dtype=np.int64)
    head = 8 * (n + 1)
    host = np.empty(head + int(sizes.sum()) + 1, dtype=np.uint8)
    offsets = host[:head].view(np.int64)
    offsets[0] = 0
    np.cumsum(sizes, out=offsets[1:])
    for k, p in enumerate(parsed):
        host[head + int(offsets[k]):head + int(offsets[k + 1])] = np.frombuffer(p[3], dtype=np.uint8)
    with torch.cuda.device(dev):
        up = torch.from_numpy(host).to(dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty((n, H, W, ch), dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(L.r2l_png_decode(C.c_void_p(up.data_ptr() + head), C.c_void_p(up.data_ptr()), n, H, W, ch, C.c_void_p(ws.data_ptr()), need,
                                    C.c_void_p(out.data_ptr()), C.c_void_p(status.data_ptr()), _lib.current_stream()))
        st = status.cpu().tolist()
    bad = [k for k in range(n) if st[k]]
    if bad:
        k = bad[0]
        more = f' (and {len(bad) - 1} more of the call\'s files: {", ".join(names[j] for j in bad[1:4])})' if len(bad) > 1 else ''
        raise ValueError(f'{names[k]}: {DECODE_STATUS.get(st[k], "status %d" % st[k])}{more}')
    return out


def device_reader(device=None):
    """the loaders' decode= hook (--png_read_device): paths -> uint8 [n, H, W, C] on the HOST, what [read_png(p) for p in paths] stacks to"""
    def decode(paths):
        return decode_pngs(paths, device).cpu().numpy()
    return decode
