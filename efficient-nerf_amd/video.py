"""The fly-through video of the reference (`imageio.mimwrite(video_path, to8b(rgbs), fps=30, quality=8)`, main.py:1096-1098, and
every --i_video iterations, :1474-1499) without imageio or ffmpeg: every frame becomes a baseline JPEG on the device
(csrc/r2l_mjpeg.hip, one C-ABI call per chunk of frames) and the files go into an AVI 1.0 container as Motion-JPEG, written here in
plain struct.  Frames leave the device as finished JPEG bytes, not as pixels."""
import ctypes as C
import os
import struct

import numpy as np

AVI_SIZE_LIMIT = 1 << 30        # AVI 1.0 without OpenDML: one RIFF chunk; a file that would pass this is refused
ENCODE_CHUNK_BYTES = 256 << 20  # frames per library call: as many as keep the output slots and the workspace under this, each


def _frames_per_call(n, pitch, ws_one):
    return max(1, min(n, ENCODE_CHUNK_BYTES // max(pitch, ws_one)))


def encode_jpeg(frames, quality=90, return_coef=False):
    """frames: float32 [n, H, W, 3] on the GPU (values as the renderer leaves them: to8b's clamp happens on the device).  Returns one
    complete JPEG file per frame as bytes; with return_coef also the quantised coefficients, int16 [n, n_blocks, 3, 64] on the device
    (zig-zag order, DC before prediction).  One r2l_mjpeg_encode call per chunk of frames on the current stream and, per chunk, one copy of
    the sizes and one of the used bytes."""
    import torch
    from . import _lib
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f'encode_jpeg: a stack [n, H, W, 3], got {tuple(frames.shape)}')
    if not (frames.is_cuda and frames.dtype == torch.float32):
        raise ValueError('encode_jpeg: a float32 tensor on the GPU')
    frames = frames.contiguous()
    n, H, W = (int(v) for v in frames.shape[:3])
    L = _lib.lib()
    pitch = L.r2l_mjpeg_max_frame_bytes(H, W)
    if pitch < 0:
        _lib.check(int(pitch))
    if not 1 <= int(quality) <= 100:
        raise ValueError(f'encode_jpeg: quality = {quality} (1 .. 100)')
    out, coefs = [], []
    if n == 0:
        return (out, torch.empty((0, 0, 3, 64), dtype=torch.int16, device=frames.device)) if return_coef else out
    n_blocks = ((H + 7) // 8) * ((W + 7) // 8)
    with torch.cuda.device(frames.device):
        per = _frames_per_call(n, pitch, L.r2l_mjpeg_workspace_bytes(1, H, W))
        need = L.r2l_mjpeg_workspace_bytes(per, H, W)
        if need < 0:
            _lib.check(int(need))
        ws = torch.empty(need, dtype=torch.uint8, device=frames.device)
        buf = torch.empty((per, pitch), dtype=torch.uint8, device=frames.device)
        sizes = torch.empty(per, dtype=torch.int64, device=frames.device)
        for i0 in range(0, n, per):
            nb = min(per, n - i0)
            coef = torch.empty((nb, n_blocks, 3, 64), dtype=torch.int16, device=frames.device) if return_coef else None
            _lib.check(L.r2l_mjpeg_encode(_lib.dptr(frames[i0:i0 + nb]), nb, H, W, int(quality), C.c_void_p(ws.data_ptr()), need,
                                          C.c_void_p(buf.data_ptr()), pitch, C.c_void_p(sizes.data_ptr()),
                                          C.c_void_p(coef.data_ptr()) if return_coef else None, _lib.current_stream()))
            sz = sizes[:nb].cpu()
            used = int(sz.max())
            host = buf[:nb, :used].cpu().numpy()          # the used bytes of every slot, one copy
            out += [host[k, :int(sz[k])].tobytes() for k in range(nb)]
            if return_coef:
                coefs.append(coef)
    return (out, torch.cat(coefs, 0)) if return_coef else out


class MJPEGWriter:
    """An AVI 1.0 file of Motion-JPEG frames: RIFF 'AVI ' { LIST 'hdrl' { avih, LIST 'strl' { strh, strf } }, LIST 'movi' { 00dc ... },
    idx1 }, little-endian.  add(frame_bytes) takes one complete JPEG file per frame and does not look inside; close() writes the index
    and patches the sizes and counts.  Nothing is written before the first frame; a file that would pass size_limit (2^30 bytes: no
    OpenDML) or that has no frame is refused with a ValueError."""
    _HDRL = 4 + (8 + 56) + (12 + (8 + 56) + (8 + 40))      # 'hdrl' + avih + LIST strl { strh, strf }
    _MOVI_AT = 12 + 8 + _HDRL                               # offset of the 'LIST' of movi

    def __init__(self, path, H, W, fps=30, size_limit=AVI_SIZE_LIMIT):
        if not (fps > 0):
            raise ValueError(f'MJPEGWriter: fps = {fps}')
        self.path, self.H, self.W, self.fps, self.size_limit = path, int(H), int(W), fps, int(size_limit)
        self._f = None
        self._index = []            # (offset from the 'movi' fourcc, unpadded size)
        self._movi = 4              # bytes of the movi list's data so far: its fourcc
        self._largest = 0
        self.closed = False

    def _total(self, movi, n):
        return self._MOVI_AT + 8 + movi + 8 + 16 * n

    def _headers(self, n, movi):
        usec = int(round(1e6 / self.fps))
        rate, scale = (int(self.fps), 1) if float(self.fps) == int(self.fps) else (int(round(self.fps * 1000)), 1000)
        avih = struct.pack('<14I', usec, 0, 0, 0x10, n, 0, 1, self._largest, self.W, self.H, 0, 0, 0, 0)
        strh = struct.pack('<4s4sIHHIIIIIIII4H', b'vids', b'MJPG', 0, 0, 0, 0, scale, rate, 0, n, self._largest, 0xFFFFFFFF, 0, 0, 0,
                           self.W, self.H)
        strf = struct.pack('<IiiHH4sIiiII', 40, self.W, self.H, 1, 24, b'MJPG', self.W * self.H * 3, 0, 0, 0, 0)
        strl = b'strl' + b'strh' + struct.pack('<I', len(strh)) + strh + b'strf' + struct.pack('<I', len(strf)) + strf
        hdrl = b'hdrl' + b'avih' + struct.pack('<I', len(avih)) + avih + b'LIST' + struct.pack('<I', len(strl)) + strl
        assert len(hdrl) == self._HDRL
        return (b'RIFF' + struct.pack('<I', self._total(movi, n) - 8) + b'AVI ' + b'LIST' + struct.pack('<I', len(hdrl)) + hdrl +
                b'LIST' + struct.pack('<I', movi) + b'movi')

    def add(self, frame_bytes):
        if self.closed:
            raise ValueError('MJPEGWriter: closed')
        size = len(frame_bytes)
        movi = self._movi + 8 + size + (size & 1)
        if self._total(movi, len(self._index) + 1) > self.size_limit:
            self._abort()
            raise ValueError(f'MJPEGWriter: "{self.path}" would pass {self.size_limit} bytes at frame {len(self._index)}: an AVI 1.0 file '
                             f'holds one RIFF chunk (OpenDML is not built); lower the quality or the number of frames')
        if self._f is None:
            self._f = open(self.path, 'wb')
            self._f.write(self._headers(0, 4))
        self._f.write(b'00dc' + struct.pack('<I', size) + bytes(frame_bytes) + (b'\0' if size & 1 else b''))
        self._index.append((self._movi, size))
        self._movi = movi
        self._largest = max(self._largest, size)

    def _abort(self):
        self.closed = True
        if self._f is not None:
            self._f.close()
            self._f = None
            os.remove(self.path)

    def close(self):
        if self.closed:
            return
        if not self._index:
            self._abort()
            raise ValueError(f'MJPEGWriter: "{self.path}" has no frame')
        self.closed = True
        idx = b''.join(struct.pack('<4sIII', b'00dc', 0x10, off, size) for off, size in self._index)
        self._f.write(b'idx1' + struct.pack('<I', len(idx)) + idx)
        self._f.seek(0)
        self._f.write(self._headers(len(self._index), self._movi))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, exc_type, *a):
        if exc_type is None:
            self.close()
        else:
            self._abort()


def write_video(path, frames_dev, fps=30, quality=90, size_limit=AVI_SIZE_LIMIT):
    """frames_dev [n, H, W, 3] float32 on the GPU -> an AVI file at path.  Returns (frames, bytes of the file)."""
    n, H, W = (int(v) for v in frames_dev.shape[:3])
    if n == 0:
        raise ValueError(f'write_video: "{path}" has no frame')
    jpegs = encode_jpeg(frames_dev, quality)
    w = MJPEGWriter(path, H, W, fps, size_limit=size_limit)
    total = w._total(4 + sum(8 + len(j) + (len(j) & 1) for j in jpegs), n)
    if total > size_limit:      # known before the file is opened
        raise ValueError(f'write_video: "{path}" would take {total} bytes, an AVI 1.0 file holds {size_limit} (OpenDML is not built); lower '
                         f'--video_quality or the number of frames')
    with w:
        for j in jpegs:
            w.add(j)
    return n, os.path.getsize(path)


def video_path(folder, args, it=None):
    """<folder>/video[_iter<i>][_<video_tag>].avi"""
    tag = getattr(args, 'video_tag', '')
    return os.path.join(folder, 'video' + (f'_iter{it}' if it is not None else '') + (f'_{tag}' if tag else '') + '.avi')


def check_video_args(args):
    """--write_video's own flags, refused in one line before a device is touched"""
    if not getattr(args, 'write_video', False):
        return
    if not 1 <= args.video_quality <= 100:
        raise SystemExit(f'--video_quality {args.video_quality}: 1 .. 100')
    if not args.video_fps > 0:
        raise SystemExit(f'--video_fps {args.video_fps}: a positive number')


def pose_spherical_np(theta, phi, radius):
    """dataset/load_blender.py:10-28 in float32 numpy: the camera at (theta, phi) degrees on a sphere of that radius, looking in"""
    t = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, radius], [0, 0, 0, 1]], dtype=np.float32)
    ph, th = phi / 180. * np.pi, theta / 180. * np.pi
    rp = np.array([[1, 0, 0, 0], [0, np.cos(ph), -np.sin(ph), 0], [0, np.sin(ph), np.cos(ph), 0], [0, 0, 0, 1]], dtype=np.float32)
    rt = np.array([[np.cos(th), 0, -np.sin(th), 0], [0, 1, 0, 0], [np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1]], dtype=np.float32)
    flip = np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=np.float32)
    return flip @ (rt @ (rp @ t))


def get_novel_poses(n_pose='20,4,1', theta1=-180, theta2=180, phi1=-90, phi2=0):
    """dataset/load_blender.py:327-356: the Blender video poses [n, 4, 4] float32, evenly spaced.  n_pose: an int (that many thetas at
    phi -30, radius 4), or 'a,b,c' / a list: a thetas, b phis strictly inside (phi1, phi2), c radii strictly inside (near, far) = (2, 6);
    with 'sample:k' / 'fixed:v' entries each axis is either sampled like that or one given value.  Order: for r, for phi, for theta."""
    near, far = 2, 6
    if isinstance(n_pose, (int, np.integer)):
        thetas, phis, radiuses = np.linspace(theta1, theta2, n_pose + 1)[:-1], [-30], [4]
    else:
        parts = [x.strip() for x in n_pose.split(',')] if isinstance(n_pose, str) else [str(x) for x in n_pose]
        if len(parts) != 3:
            raise ValueError(f'--n_pose_video {n_pose}: three entries (thetas, phis, radii)')
        if ':' not in parts[0]:
            parts = [f'sample:{int(x)}' for x in parts]

        def axis(part, inner, lo, hi):
            mode, value = part.split(':')
            if mode != 'sample':
                return [float(value)]
            return np.linspace(lo, hi, int(value) + 2)[1:-1] if inner else np.linspace(lo, hi, int(value) + 1)[:-1]
        thetas, phis, radiuses = axis(parts[0], False, theta1, theta2), axis(parts[1], True, phi1, phi2), axis(parts[2], True, near, far)
    return np.stack([pose_spherical_np(t, p, r) for r in radiuses for p in phis for t in thetas], 0)


def training_video_poses(args, hwf=None):
    """What a training run renders every --i_video iterations (main.py:1474-1499): (poses [n, 3, 4] float32, (H, W, focal)).  Blender:
    get_novel_poses(--n_pose_video) at hwf (the run's own, else what the front end would render at); LLFF: the loader's render_poses at
    the scene's intrinsics."""
    import argparse
    import torch
    from .frontend import has_llff_scene, load_llff_set, load_test_poses
    if args.dataset_type == 'llff':
        if not has_llff_scene(args):
            raise SystemExit(f'--write_video with --dataset_type llff needs the scene under --datadir ("{args.datadir}") for its render path')
        view = argparse.Namespace(**vars(args))
        view.render_test = False
        poses, scene_hwf, _ = load_llff_set(view)
        return poses.float(), tuple(scene_hwf)
    try:
        poses = get_novel_poses(args.n_pose_video)
    except ValueError as e:
        raise SystemExit(f'--n_pose_video {args.n_pose_video}: {e}')
    return torch.from_numpy(poses[:, :3, :4].copy()), tuple(hwf) if hwf is not None else load_test_poses(args)[1]


def video_pass(i, args, folder, log, poses, hwf, render):
    """One --i_video pass of a training loop: render(pose [3, 4], out [H * W, 3]) fills a frame from the weights as they stand; the stack
    goes through write_video into <folder>/video_iter<i>[_<video_tag>].avi."""
    import time
    import torch
    H, W, _ = hwf
    log(f'Iter {i} Rendering video... (n_pose: {len(poses)})')
    t_ = time.time()
    with torch.no_grad():
        frames = torch.empty((len(poses), int(H), int(W), 3), dtype=torch.float32, device=torch.device('cuda', torch.cuda.current_device()))
        for k, pose in enumerate(poses):
            render(pose, frames[k].view(-1, 3))
        path = video_path(folder, args, it=i)
        write_video(path, frames, fps=args.video_fps, quality=args.video_quality)
    log(f'[VIDEO] Rendering done. Time {time.time() - t_:.2f}s. Save video: "{path}"')
    return path
