"""Real images to `[4096, 9]` ray shards: the reference's utils/convert_original_data_to_rays_blender.py (step 4 of its README)
on the device.

    python convert_data.py --splits train --datadir data/nerf_synthetic/lego

reads transforms_<split>.json and the PNGs, and writes <datadir>_real_<splits><suffix>/<splits>_<k>.npy, k = 1, 2, ...: float32
[4096, 9] rows of (rays_o, rays_d, rgb) in the reference's shuffled order (two np.random.permutation draws of the global numpy
stream, :221-223).  The images stay uint8 on their way to the device; bytes / 255, the half-resolution 2 x 2 mean, the compositing
on white, get_rays and the shuffle are one launch of r2l_rays_from_images (csrc/r2l_convert.hip), one thread per output row.

Flags as the reference's (--splits a,b  --datadir  --suffix  --ignore i,j  --full_res; half resolution is the default, white_bkgd
True and 4096 rays per shard are fixed as there, :97-98) plus --seed N (np.random.seed(N) in front of the two draws; without it the
global stream as it stands, as the reference).  --donerf and the half resolution of non-square images (which the reference cannot
run either: it hands cv2.resize (H, W) where (W, H) is expected, :173) are refused.

    python convert_data.py --dataset_type llff --splits train --datadir data/nerf_llff_data/fern

is the reference's utils/convert_original_data_to_rays_llff.py: the scene through llff.py (factor 8, every 8th view held out and
4096 rays per shard are fixed there, :53-56, :80), train = the views that are not held out, val or test = the held-out ones, no
halving and no compositing (the images are RGB), the same two permutation draws, the same dropped remainder, the same directory
and file names; flags --splits --datadir --suffix --ignore (accepted and unused, as there) and --seed.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

from . import blender
from ._lib import R2LError, check, current_stream, dptr, lib

SPLIT_SIZE = 4096           # :98
# :113-115, the reference's hand-designed rule for the ficus scene: images of phi >= 0
FICUS_IGNORE = '10,13,14,24,26,30,31,37,39,40,41,47,48,49,52,54,55,57,58,66,67,74,75,76,77,79,81,82,87,88,89,94,97,99'


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog='convert_data.py', description=__doc__.split('\n\n')[0])
    p.add_argument('--splits', type=str, default='')
    p.add_argument('--datadir', type=str, default='')
    p.add_argument('--suffix', type=str, default='')
    p.add_argument('--ignore', type=str, default='', help='ignore some samples')
    p.add_argument('--donerf', action='store_true')
    p.add_argument('--full_res', action='store_true')
    p.add_argument('--seed', type=int, default=None, help='np.random.seed(N) in front of the two permutation draws')
    p.add_argument('--dataset_type', type=str, default='blender', choices=['blender', 'llff'])
    p.add_argument('--png_read_device', action='store_true', help='decode the PNGs on the device (png.decode_pngs) instead of in blender.read_png')
    args = p.parse_args(argv)
    if args.dataset_type == 'llff' and (args.full_res or args.donerf):
        raise SystemExit('--full_res / --donerf belong to --dataset_type blender: LLFF images are read at factor 8 and never halved')
    if args.donerf:
        raise SystemExit('--donerf: the DONERF ray rule is not built (rays are get_rays\', as for the Blender scenes)')
    if 'ficus' in args.datadir:
        args.ignore = FICUS_IGNORE
    return args


def save_layout(args):
    """:117-122: (splits, prefix, savedir)"""
    splits = args.splits.split(',')
    prefix = ''.join(splits)
    return splits, prefix, f'{os.path.normpath(args.datadir)}_real_{prefix}{args.suffix}'


def kept_frames(frames, ignore):
    """:126, 135-141: the frames whose index (the text behind the last '_' of file_path) is not in the --ignore list"""
    ignored = ignore.split(',')
    return [f for f in frames if f['file_path'].split('_')[-1] not in ignored]


def load_images(datadir, splits, ignore, decode=None):
    """:124-150 with the images left as the PNGs' bytes: (uint8 [n, H0, W0, C], float32 poses [n, 4, 4], camera_angle_x).  decode:
    blender.read_pngs', one call per split"""
    metas = {}
    for s in splits:
        with open(os.path.join(datadir, f'transforms_{s}.json')) as fp:
            metas[s] = json.load(fp)
    imgs, poses = [], []
    for s in splits:
        frames = kept_frames(metas[s]['frames'], ignore)
        imgs += blender.read_pngs([os.path.join(datadir, frame['file_path'] + '.png') for frame in frames], decode)
        poses += [np.array(frame['transform_matrix']) for frame in frames]
    if not imgs:
        raise SystemExit(f'no image left under "{datadir}" for --splits {",".join(splits)} --ignore {ignore}')
    shapes = {im.shape for im in imgs}
    if len(shapes) != 1:
        raise SystemExit(f'the images under "{datadir}" differ in shape: {sorted(shapes)}')
    meta = metas[splits[-1]]
    if 'camera_angle_x' in meta:
        angle = float(meta['camera_angle_x'])
    else:                                                     # :160-162
        with open(os.path.join(datadir, 'dataset_info.json')) as fp:
            angle = float(json.load(fp)['camera_angle_x'])
    return np.ascontiguousarray(np.array(imgs)), np.array(poses).astype(np.float32), angle


def output_grid(H0, W0, camera_angle_x, half_res):
    """:156-170: (H, W, focal) of the rays"""
    focal = .5 * W0 / np.tan(.5 * camera_angle_x)
    if not half_res:
        return H0, W0, focal
    if H0 != W0:
        raise SystemExit(f'half resolution of {H0} x {W0} images: only square images are halved (pass --full_res)')
    return H0 // 2, W0 // 2, focal / 2.


def draw_order(n, seed=None):
    """:221-223: all_data[rand_ix1][rand_ix2] = all_data[rand_ix1[rand_ix2]]"""
    if seed is not None:
        np.random.seed(seed)
    rand_ix1 = np.random.permutation(n)
    rand_ix2 = np.random.permutation(n)
    return rand_ix1[rand_ix2]


def saved_rows(n):
    """:228: whole shards only, the remainder is dropped"""
    return n // SPLIT_SIZE * SPLIT_SIZE


def rays_from_images(images, poses, focal, half_res, order, device=None):
    """out [len(order), 9] on the device: row k = (rays_o, rays_d, rgb) of pixel order[k] (image * H * W + row * W + column on the
    output grid).  images: uint8 [n, H0, W0, C], C = 3 or 4; poses: [n, 3 or 4, 4]; focal: of the output grid."""
    if not torch.cuda.is_available():
        raise R2LError('no HIP device visible to torch: the conversion has no CPU fallback')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    im = torch.as_tensor(images)
    if im.dtype != torch.uint8 or im.dim() != 4 or im.shape[-1] not in (3, 4):
        raise R2LError(f'images are {im.dtype} {tuple(im.shape)}, expected uint8 [n, H, W, 3 or 4]')
    n_img, H0, W0, ch = (int(v) for v in im.shape)
    po = torch.as_tensor(poses).to(torch.float32)
    if po.dim() != 3 or po.shape[0] != n_img or po.shape[1] < 3 or po.shape[2] != 4:
        raise R2LError(f'poses are {tuple(po.shape)}, expected [{n_img}, 3 or 4, 4]')
    od = torch.as_tensor(order)
    if od.dtype != torch.int64 or od.dim() != 1:
        raise R2LError(f'order is {od.dtype} {tuple(od.shape)}, expected int64 [rows]')
    im, po, od = im.contiguous().to(dev), po[:, :3, :4].contiguous().to(dev), od.contiguous().to(dev)
    rows = int(od.shape[0])
    out = torch.empty((rows, 9), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib().r2l_rays_from_images(C.c_void_p(im.data_ptr()), n_img, H0, W0, ch, dptr(po), float(focal), 1 if half_res else 0,
                                         C.c_void_p(od.data_ptr()), rows, dptr(out), current_stream()))
    return out


LLFF_FACTOR, LLFF_HOLD = 8, 8   # convert_original_data_to_rays_llff.py:56, :80


def llff_views(n, splits):
    """convert_original_data_to_rays_llff.py:90-105: the views of --splits in the order they are stacked -- the train views first
    when 'train' is named, then the held-out ones once when 'val' or 'test' is"""
    from . import llff
    i_train, _, i_test = llff.split_indices(n, LLFF_HOLD)
    views = []
    if 'train' in splits:
        views += [int(i) for i in i_train]
    if 'val' in splits or 'test' in splits:
        views += [int(i) for i in i_test]
    return views


def load_llff_images(datadir, splits, decode=None):
    """:79-107 with the images left as the PNGs' bytes: (uint8 [n, H, W, 3], float32 poses [n, 3, 4], (H, W, focal))"""
    from . import llff
    try:
        scene = llff.load_scene(datadir, factor=LLFF_FACTOR, recenter_poses=True, bd_factor=.75, spherify=False, path_zflat=False, n_pose_video=120, decode=decode)
    except llff.LLFFError as e:
        raise SystemExit(str(e))
    views = llff_views(len(scene.poses), splits)
    if not views:
        raise SystemExit(f'--splits {",".join(splits)} names no view of "{datadir}": train, val or test')
    return np.ascontiguousarray(scene.bytes[views]), np.ascontiguousarray(scene.poses[views][:, :3, :4]), scene.hwf


def convert(args, log=print):
    """the reference's script from its arguments on; returns the paths written"""
    splits, prefix, savedir = save_layout(args)
    decode = None
    if getattr(args, 'png_read_device', False):
        from . import png
        if not torch.cuda.is_available():
            raise SystemExit('--png_read_device: no HIP device visible to torch, and PNG decoding on the device has no CPU fallback')
        decode = png.device_reader()
    if getattr(args, 'dataset_type', 'blender') == 'llff':
        imgs, poses, (H, W, focal) = load_llff_images(args.datadir, splits, decode)
        n_img, H0, W0, ch = imgs.shape
        log(f'Read all images and poses, done. all_imgs shape {imgs.shape}, all_poses shape {poses.shape}')
        half_res = False
    else:
        imgs, poses, angle = load_images(args.datadir, splits, args.ignore, decode)
        n_img, H0, W0, ch = imgs.shape
        log(f'Read all images and poses, done. all_imgs shape {imgs.shape}, all_poses shape {poses.shape}')
        half_res = not args.full_res
        H, W, focal = output_grid(H0, W0, angle, half_res)
    os.makedirs(savedir, exist_ok=True)
    log(f'Resize, done. all_imgs shape {torch.Size([n_img, H, W, 3])}, all_poses shape {torch.Size(poses.shape)}, num_channels of the images {ch}')
    n = n_img * H * W
    log(f'Collect all rays, done. all_data shape {torch.Size([n, 9])}')
    order = draw_order(n, args.seed)
    num = saved_rows(n)
    data = rays_from_images(imgs, poses, focal, half_res, np.ascontiguousarray(order[:num]).astype(np.int64)).cpu().numpy()
    paths = []
    for split, ix in enumerate(range(0, num, SPLIT_SIZE), 1):
        save_path = f'{savedir}/{prefix}_{split}.npy'
        np.save(save_path, data[ix:ix + SPLIT_SIZE])
        paths.append(save_path)
        log(f'[{split}/{num // SPLIT_SIZE}] save_path: {save_path}')
    log(f'All data saved at "{savedir}"')
    return paths


def main(argv=None):
    args = parse_args(argv)
    if not args.splits or not args.datadir:
        raise SystemExit('convert_data.py needs --splits and --datadir (e.g. --splits train --datadir data/nerf_synthetic/lego)')
    from . import dist as D
    torch.cuda.set_device(D.local_device(0))
    convert(args, log=lambda *a, **k: print(*a, **k, flush=True))
    return 0


if __name__ == '__main__':
    sys.exit(main())
