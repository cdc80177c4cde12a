"""The still images of the reference (`imageio.imwrite(filename, to8b(rgb))`, main.py:337-341) as files finished on the device: every
frame of a device stack becomes a complete PNG (csrc/r2l_png.hip: filters, deflate, Adler-32 and CRC-32 in kernels, one C-ABI call per
chunk of frames).  Frames leave the device as .png bytes, not as pixels; --png_device puts this behind the front end's writers."""
import ctypes as C

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
