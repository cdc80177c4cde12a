"""Golden data for efficient-nerf_amd/llff.py and the LLFF branch of convert_data.py: the REFERENCE's own loader
(dataset/load_llff.py: load_llff_data, get_rand_pose_v2) and its own converter (utils/convert_original_data_to_rays_llff.py),
unmodified, run from the reference tree (build container only; R2L_REFERENCE names the tree):

    python tests/golden/make_golden_llff.py

Modules they import that are not dependencies here are stood in for through sys.modules:
  imageio.imread                -> the package's PNG reader (blender.read_png), accepting ignoregamma
  configargparse.ArgumentParser -> argparse.ArgumentParser
  cv2                           -> an empty module (the LLFF converter imports it and calls nothing)
  visualize_3d                  -> a no-op (the loader would write two PDFs into the working directory)
and a temporary images/ folder with one PNG stands for the full-size captures the loader only takes a shape from.

Scene (tests/golden/llff/scene): poses_bounds.npy with 10 forward-facing poses in the LLFF layout ([down, right, back] rotation
columns, position, (240, 320, focal) column, near / far bound per view) and images_8/000.png .. 009.png, 30 x 40 RGB colour
ramps.  With hold-out 8 the test views are {0, 8}; the 8 train views give 9,600 rays = 2 shards, 1,408 rays dropped.

Written:
  llff_loader.npz                 images, poses, bds, render_poses (n_pose_video = 8), i_test, hwf; 16 get_rand_pose_v2 poses after
                                  np.random.seed(0), each followed by the focal draw np.random.rand() + 1
  scene_real_train/train_{1,2}.npy   the converter after np.random.seed(1234)
While generating, both shards are compared with a float64 recomputation of the same rows."""
import argparse
import os
import runpy
import shutil
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('R2L_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd import blender  # noqa: E402
from efficient_nerf_amd.frontend import write_png  # noqa: E402

OUT = os.path.join(HERE, 'llff')
SCENE = os.path.join(OUT, 'scene')
N_IMG, H0, W0, FOCAL0, FACTOR, HOLD, SEED = 10, 240, 320, 300., 8, 8, 1234
H, W = H0 // FACTOR, W0 // FACTOR


def make_scene():
    rs = np.random.RandomState(0)
    os.makedirs(os.path.join(SCENE, f'images_{FACTOR}'), exist_ok=True)
    rows = []
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    for k in range(N_IMG):
        img = np.zeros((H, W, 3), dtype=np.uint8)
        img[..., 0] = (5 * x + 23 * k) % 256
        img[..., 1] = (3 * y + 2 * x + 40 * k) % 256
        img[..., 2] = (255 - 4 * x - 3 * y + 9 * k) % 256
        write_png(os.path.join(SCENE, f'images_{FACTOR}', f'{k:03d}.png'), img)
        # a camera on a jittered 5 x 2 grid in front of the scene, looking down -z with a small tilt: [right, up, back] columns
        pos = np.array([(k % 5 - 2) * 0.6, (k // 5 - 0.5) * 0.5, 0.]) + rs.uniform(-0.1, 0.1, 3)
        back = np.array([0., 0., 1.]) + rs.uniform(-0.15, 0.15, 3)
        back /= np.linalg.norm(back)
        right = np.cross([0., 1., 0.] + rs.uniform(-0.05, 0.05, 3), back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        m = np.stack([-up, right, back, pos, [H0, W0, FOCAL0]], 1)         # the file's [down, right, back] order
        near = 3. + rs.uniform(0., 1.5)
        rows.append(np.concatenate([m.reshape(-1), [near, near * rs.uniform(3., 6.)]]))
    np.save(os.path.join(SCENE, 'poses_bounds.npy'), np.array(rows))


def stand_ins():
    cap = types.ModuleType('configargparse')
    cap.ArgumentParser = argparse.ArgumentParser
    iio = types.ModuleType('imageio')
    iio.imread = lambda f, ignoregamma=False: blender.read_png(f)
    sys.modules.update(configargparse=cap, imageio=iio, cv2=types.ModuleType('cv2'))
    sys.path.insert(0, REF)
    import utils.run_nerf_raybased_helpers as helpers
    helpers.visualize_3d = lambda *a, **k: None
    import dataset.load_llff as L
    return L


def float64_rows(poses, focal, views):
    """every ray of the given views in float64, view by view, row-major: [n * H * W, 9]"""
    rows = []
    focal = float(np.float32(focal))
    for k in views:
        rgb = blender.read_png(os.path.join(SCENE, f'images_{FACTOR}', f'{k:03d}.png')).astype(np.float64)[..., :3] / 255.
        c2w = poses[k, :3, :4].astype(np.float64)
        j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
        dirs = np.stack([(i - W * .5) / focal, -(j - H * .5) / focal, -np.ones_like(i)], -1)
        d = dirs @ c2w[:3, :3].T
        rows.append(np.concatenate([np.broadcast_to(c2w[:3, 3], d.shape), d, rgb], -1).reshape(-1, 9))
    return np.concatenate(rows, 0)


def main():
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    make_scene()
    L = stand_ins()
    tmp_images = os.path.join(SCENE, 'images')
    os.makedirs(tmp_images)
    shutil.copy(os.path.join(SCENE, f'images_{FACTOR}', '000.png'), tmp_images)
    cwd, argv0 = os.getcwd(), list(sys.argv)
    try:
        os.chdir(REF)
        images, poses, bds, render_poses, i_test = (np.asarray(t) for t in L.load_llff_data(SCENE, factor=FACTOR, n_pose_video=8))
        np.random.seed(0)
        rand_poses, rand_focal = [], []
        for _ in range(16):
            rand_poses.append(L.get_rand_pose_v2().numpy())
            rand_focal.append(np.random.rand() + 1)
        assert images.shape == (N_IMG, H, W, 3) and poses.shape == (N_IMG, 3, 5) and render_poses.shape == (8, 3, 5)
        np.savez_compressed(os.path.join(OUT, 'llff_loader.npz'), images=images, poses=poses, bds=bds, render_poses=render_poses,
                            i_test=np.int64(i_test), hwf=poses[0, :3, -1], rand_poses=np.array(rand_poses), rand_focal=np.array(rand_focal))
        script = os.path.join(REF, 'utils', 'convert_original_data_to_rays_llff.py')
        sys.argv = [script, '--splits', 'train', '--datadir', SCENE]
        np.random.seed(SEED)
        runpy.run_path(script, run_name='__main__')
    finally:
        os.chdir(cwd)
        sys.argv = argv0
        shutil.rmtree(tmp_images)
    train = [k for k in range(N_IMG) if k % HOLD]
    ref = float64_rows(poses, poses[0, 2, 4], train)
    n = ref.shape[0]
    np.random.seed(SEED)
    order = np.random.permutation(n)
    order = order[np.random.permutation(n)]
    d = f'{SCENE}_real_train'
    files = sorted(os.listdir(d), key=lambda f: int(f.split('_')[-1].split('.')[0]))
    assert n == 9600 and files == ['train_1.npy', 'train_2.npy'], (files, n)
    worst = np.zeros(3)
    for k, f in enumerate(files):
        got = np.load(os.path.join(d, f))
        assert got.dtype == np.float32 and got.shape == (4096, 9)
        diff = np.abs(got.astype(np.float64) - ref[order[k * 4096:(k + 1) * 4096]])
        worst = np.maximum(worst, [diff[:, 0:3].max(), diff[:, 3:6].max(), diff[:, 6:9].max()])
    print(f'{os.path.basename(d)}: {len(files)} shard(s), max |reference - float64| origins {worst[0]:.2e} directions {worst[1]:.2e} '
          f'colours {worst[2]:.2e} (max |d| {np.abs(ref[:, 3:6]).max():.2f}); hold-out view of the loader {int(i_test)}')
    assert worst[0] == 0 and worst[1:].max() < 2e-7


if __name__ == '__main__':
    main()
