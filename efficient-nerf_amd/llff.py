"""Forward-facing LLFF scenes (fern, flower, ... of nerf_llff_data): poses_bounds.npy and the `images_<factor>` PNGs to images,
poses, bounds, the spiral video path, the hold-out split and the random poses `create_data rand` renders.  numpy only.

Restates dataset/load_llff.py of the reference (`_load_data` :68-132, `poses_avg` / `recenter_poses` / `render_path_spiral`,
`get_rand_pose_v2` :187-236, `load_llff_data` :336-456) and the split rule of main.py:903-911, step by step in the same numpy
arithmetic, so that poses, bounds and paths come out to the last bit (tests/test_llff_cpu.py against the reference's own run).

What differs on purpose:
  * `mogrify` is never run: a missing `images_<factor>` folder is an error that names it and the command that makes it;
  * only PNGs are read (blender.read_png); a JPEG in that folder is refused by name;
  * an image count that differs from poses_bounds.npy is an error (the reference prints and returns None);
  * nothing is plotted or written (the reference leaves two PDFs in the working directory);
  * the state get_rand_pose_v2 keeps in module globals is an object (`RandPoseState`), and the draw takes the generator;
  * spherify=True is not built.
"""
import os

import numpy as np

from .blender import read_png, read_pngs  # noqa: F401


class LLFFError(ValueError):
    """the scene on disk is not what the loader reads; one line"""


def _normalize(x):
    return x / np.linalg.norm(x)


def view_matrix(z, up, pos):
    """[3, 4] camera-to-world from a viewing axis, an up hint and a position (load_llff.py:139-147)"""
    v2 = _normalize(z)
    v0 = _normalize(np.cross(up, v2))
    v1 = _normalize(np.cross(v2, v0))
    return np.stack([v0, v1, v2, pos], 1)


def average_pose(poses):
    """[3, 5]: mean position, summed viewing axes and up vectors, the first pose's (H, W, focal) column (load_llff.py:155-161)"""
    hwf = poses[0, :3, -1:]
    center = poses[:, :3, 3].mean(0)
    v2 = _normalize(poses[:, :3, 2].sum(0))
    up = poses[:, :3, 1].sum(0)
    return np.concatenate([view_matrix(v2, up, center), hwf], 1)


def recenter(poses):
    """every pose in the frame of the average pose; the (H, W, focal) column stays (load_llff.py:239-261)"""
    out = poses + 0
    bottom = np.reshape([0, 0, 0, 1.], [1, 4])
    c2w = np.concatenate([average_pose(poses)[:3, :4], bottom], -2)
    full = np.concatenate([poses[:, :3, :4], np.tile(np.reshape(bottom, [1, 1, 4]), [poses.shape[0], 1, 1])], -2)
    full = np.linalg.inv(c2w) @ full
    out[:, :3, :4] = full[:, :3, :4]
    return out


def spiral_path(c2w, up, rads, focal, zrate, rots, n):
    """n poses on a spiral around c2w, all looking at the point `focal` in front of it (load_llff.py:164-183)"""
    out = []
    rads = np.array(list(rads) + [1.])
    hwf = c2w[:, 4:5]
    for theta in np.linspace(0., 2. * np.pi * rots, n + 1)[:-1]:
        c = np.dot(c2w[:3, :4], np.array([np.cos(theta), -np.sin(theta), -np.sin(theta * zrate), 1.]) * rads)
        z = _normalize(c - np.dot(c2w[:3, :4], np.array([0, 0, -focal, 1.])))
        out.append(np.concatenate([view_matrix(z, up, c), hwf], 1))
    return out


class RandPoseState:
    """What a random pose is drawn from (the GLOBALS of load_llff.py:409-415): the average pose c2w [3, 5], the normalised summed
    up vector, and the recentred poses [N, 3, 5] whose positions and viewing axes span the two boxes"""

    def __init__(self, c2w, up, poses):
        self.c2w, self.up, self.poses = c2w, up, poses

    def boxes(self):
        """((mins, maxs) of the positions, (mins, maxs) of the viewing axes), load_llff.py:194-195, 222-228"""
        o, d = np.array(self.poses[:, :3, 3]), np.array(self.poses[:, :3, 2])
        return (np.min(o, axis=0), np.max(o, axis=0)), (np.min(d, axis=0), np.max(d, axis=0))


def _scaled_range(left, right, scale):
    """the interval [left, right] widened about its middle by `scale` (load_llff.py:231-235)"""
    assert right > left
    middle = (left + right) * 0.5
    left = middle - (right - left) * scale * 0.5
    return left, 2 * middle - left


def pose_in_boxes(state, uo, ud, scale=1.1):
    """the pose at fractions uo (x, y, z of the position box) and ud (of the viewing-axis box), both boxes widened by `scale`:
    float32 [3, 5] (load_llff.py:202-218 with the six draws given)"""
    (mins_o, maxs_o), (mins_d, maxs_d) = state.boxes()

    def at(u, lo, hi):
        left, right = _scaled_range(lo, hi, scale)
        return float(u) * (right - left) + left       # a Python float, as np.random.rand() gives: the product stays float32

    c2w = state.c2w
    c = np.dot(c2w[:3, :4], np.array([at(uo[0], mins_o[0], maxs_o[0]), at(uo[1], mins_o[1], maxs_o[1]), at(uo[2], mins_o[2], maxs_o[2]), 1]))
    z = np.dot(c2w[:3, :4], np.array([at(ud[0], mins_d[0], maxs_d[0]), at(ud[1], mins_d[1], maxs_d[1]), at(ud[2], mins_d[2], maxs_d[2]), 1]))
    return np.concatenate([view_matrix(_normalize(z), state.up, c), c2w[:, 4:5]], 1).astype(np.float32)


def pose_box(state, scale=1.1):
    """What pose_in_boxes reads of the state, as the 27 float64 r2l_llff_rand_poses takes (csrc/r2l_online.hip builds the poses of an
    online step from it on the device): the average pose c2w[:3, :4] row-major (12), up (3), then left [3], right [3] of the
    position box and of the viewing-axis box, each axis _scaled_range's own values in the state's dtype, widened to float64"""
    sides = []
    for mins, maxs in state.boxes():
        ranges = [_scaled_range(mins[a], maxs[a], scale) for a in range(3)]
        sides += [[r[0] for r in ranges], [r[1] for r in ranges]]
    return np.concatenate([np.asarray(state.c2w[:3, :4], dtype=np.float64).ravel(), np.asarray(state.up, dtype=np.float64).ravel(),
                           np.asarray(sides, dtype=np.float64).ravel()])


def rand_pose(state, rs, scale=1.1):
    """get_rand_pose_v2 (load_llff.py:187-218) on the generator `rs` (an np.random.RandomState): six rand() draws in the reference's
    order -- position x, y, z, then viewing axis x, y, z"""
    uo = [rs.rand(), rs.rand(), rs.rand()]
    ud = [rs.rand(), rs.rand(), rs.rand()]
    return pose_in_boxes(state, uo, ud, scale)


def split_indices(n, llffhold=8):
    """(i_train, i_val, i_test) of main.py:903-911: every llffhold-th view is held out, validation is the test set.  llffhold <= 0
    keeps `load_llff_data`'s own single hold-out, which the caller passes on instead."""
    if llffhold <= 0:
        raise LLFFError(f'llffhold={llffhold}: pass the loader\'s own hold-out view instead of calling split_indices')
    i_test = np.arange(n)[::llffhold]
    i_train = np.array([i for i in np.arange(int(n)) if i not in i_test])
    return i_train, i_test, i_test


def image_dir(basedir, factor):
    return os.path.join(basedir, 'images' + (f'_{factor}' if factor else ''))


def _load_data(basedir, factor, decode=None):
    """load_llff.py:68-132: (poses [3, 5, N] float64 with H, W of the first image and focal / factor, bds [2, N], bytes uint8
    [N, H, W, 3])"""
    pb = os.path.join(basedir, 'poses_bounds.npy')
    if not os.path.exists(pb):
        raise LLFFError(f'"{pb}" is not there: --dataset_type llff reads the scene\'s poses and bounds from it')
    arr = np.load(pb)
    poses = arr[:, :-2].reshape([-1, 3, 5]).transpose([1, 2, 0])
    bds = arr[:, -2:].transpose([1, 0])
    imgdir = image_dir(basedir, factor)
    if not os.path.isdir(imgdir):
        pct = 100. / factor if factor else 100.
        raise LLFFError(f'"{imgdir}" is not there; make it from "{os.path.join(basedir, "images")}" with: mogrify -resize {pct:g}% -format png *')
    names = sorted(os.listdir(imgdir))
    jpegs = [f for f in names if f.lower().endswith(('.jpg', '.jpeg'))]
    if jpegs:
        raise LLFFError(f'"{os.path.join(imgdir, jpegs[0])}": only PNGs are read; convert the folder with mogrify -format png, then remove the JPEGs')
    files = [os.path.join(imgdir, f) for f in names if f.endswith('png')]
    if poses.shape[-1] != len(files):
        raise LLFFError(f'"{imgdir}" holds {len(files)} PNG(s), "{pb}" {poses.shape[-1]} pose(s)')
    imgs = [im[..., :3] for im in read_pngs(files, decode)]
    shapes = {im.shape for im in imgs}
    if len(shapes) != 1 or imgs[0].shape[-1] != 3:
        raise LLFFError(f'the images under "{imgdir}" are not all of one RGB shape: {sorted(shapes)}')
    poses[:2, 4, :] = np.array(imgs[0].shape[:2]).reshape([2, 1])
    poses[2, 4, :] = poses[2, 4, :] * 1. / (factor or 1)
    return poses, bds, np.ascontiguousarray(np.stack(imgs, 0))


class Scene:
    """A loaded scene: bytes uint8 [N, H, W, 3] (the PNGs' own; `images` divides them), poses float32 [N, 3, 5], bds [N, 2],
    render_poses [n, 3, 5], i_test (the view nearest the average pose) and rand_state for `rand_pose`"""

    def __init__(self, image_bytes, poses, bds, render_poses, i_test, rand_state):
        self.bytes, self.poses, self.bds, self.render_poses, self.i_test, self.rand_state = image_bytes, poses, bds, render_poses, i_test, rand_state

    @property
    def images(self):
        """float32 [N, H, W, 3]: float32(byte / 255.) as the reference computes it (load_llff.py:127, :352)"""
        return (self.bytes / 255.).astype(np.float32)

    @property
    def hwf(self):
        """(H, W, focal) of main.py:898, 987-988"""
        H, W, focal = self.poses[0, :3, -1]
        return int(H), int(W), float(focal)


def load_scene(basedir, factor=8, recenter_poses=True, bd_factor=.75, spherify=False, path_zflat=False, n_pose_video=120, decode=None):
    """load_llff.py:336-456 up to its return, images left as bytes.  decode: blender.read_pngs', all the images in one call"""
    if spherify:
        raise LLFFError('--spherify (360-degree LLFF captures) is not built: forward-facing scenes only')
    poses, bds, image_bytes = _load_data(basedir, factor, decode)
    # [down, right, back] -> [right, up, back]; the view index to the front
    poses = np.concatenate([poses[:, 1:2, :], -poses[:, 0:1, :], poses[:, 2:, :]], 1)
    poses = np.moveaxis(poses, -1, 0).astype(np.float32)
    bds = np.moveaxis(bds, -1, 0).astype(np.float32)
    sc = 1. if bd_factor is None else 1. / (bds.min() * bd_factor)
    poses[:, :3, 3] *= sc
    bds *= sc
    if recenter_poses:
        poses = recenter(poses)
    c2w = average_pose(poses)
    # the depth the spiral looks at, and its radii
    close_depth, inf_depth = bds.min() * .9, bds.max() * 5.
    dt = .75
    focal = 1. / (((1. - dt) / close_depth + dt / inf_depth))
    rads = np.percentile(np.abs(poses[:, :3, 3]), 90, 0)
    n_views, n_rots = int(n_pose_video), 2
    if path_zflat:
        c2w[:3, 3] = c2w[:3, 3] + (-close_depth * .1) * c2w[:3, 2]
        rads[2] = 0.
        n_rots = 1
        n_views //= 2
    up = _normalize(poses[:, :3, 1].sum(0))
    state = RandPoseState(c2w, up, poses)
    render_poses = np.array(spiral_path(c2w, up, rads, focal, zrate=.5, rots=n_rots, n=n_views)).astype(np.float32)
    center = average_pose(poses)
    i_test = int(np.argmin(np.sum(np.square(center[:3, 3] - poses[:, :3, 3]), -1)))
    poses = poses.astype(np.float32)
    state.poses = poses
    return Scene(image_bytes, poses, bds, render_poses, i_test, state)


def load_llff_data(basedir, factor=8, recenter=True, bd_factor=.75, spherify=False, path_zflat=False, n_pose_video=120):
    """(images float32 [N, H, W, 3], poses float32 [N, 3, 5], bds [N, 2], render_poses [n, 3, 5], i_test), load_llff.py:336-456"""
    s = load_scene(basedir, factor, recenter, bd_factor, spherify, path_zflat, n_pose_video)
    return s.images, s.poses, s.bds, s.render_poses, s.i_test


def has_scene(datadir):
    return os.path.exists(os.path.join(datadir, 'poses_bounds.npy'))


def n_pose_video_from_flag(text):
    """--n_pose_video for an LLFF path: an integer is its length; the Blender triple default ('20,4,1') gives the loader's own 120"""
    text = str(text)
    return int(text) if text.strip().lstrip('-').isdigit() else 120
