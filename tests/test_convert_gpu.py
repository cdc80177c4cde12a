"""GPU: real images to ray shards (csrc/r2l_convert.hip, efficient-nerf_amd/convert_data.py) against the shards the reference's own
converter wrote for the same scene and seed (tests/golden/convert, tests/golden/make_golden_convert.py).

Bounds: origins are copies of the pose, so bit-equal.  Directions and colours within 5e-7 absolute at |value| <= 1.1: the 1e-7 the
reference itself is from exact arithmetic on this fixture plus at most five fp32 roundings of the same operations in the kernel.
Every comparison is row for row, no sorting: a wrong gather shows as a wrong colour in its row."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 5e-7
RUNS = {'': [], '_full': ['--full_res', '--suffix', '_full'], '_ign': ['--full_res', '--ignore', '1,3', '--suffix', '_ign']}


@pytest.fixture(scope='module')
def CD(pkg, built_lib):
    from efficient_nerf_amd import convert_data
    return convert_data


@pytest.fixture(scope='module')
def scene(golden_dir, tmp_path_factory):
    """a copy of the golden scene: the converter writes beside --datadir"""
    dst = tmp_path_factory.mktemp('convert') / 'scene'
    shutil.copytree(os.path.join(golden_dir, 'convert', 'scene'), str(dst))
    return str(dst)


def _shards(d):
    files = sorted((f for f in os.listdir(d) if f.endswith('.npy')), key=lambda f: int(f.split('_')[-1].split('.')[0]))
    return files, [np.load(os.path.join(d, f)) for f in files]


def _compare(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape == (4096, 9), (what, got.dtype, got.shape)
    d_dir, d_rgb = np.abs(got[:, 3:6] - want[:, 3:6]).max(), np.abs(got[:, 6:9] - want[:, 6:9]).max()
    print(f'{what}: origins equal {np.array_equal(got[:, :3], want[:, :3])}, max |directions - golden| {d_dir:.2e}, max |colours - golden| {d_rgb:.2e}')
    assert np.array_equal(got[:, :3], want[:, :3]), what
    assert d_dir <= TOL and d_rgb <= TOL, (what, d_dir, d_rgb)


@pytest.mark.parametrize('suffix', list(RUNS))
def test_shards_match_the_reference_converter(CD, scene, golden_dir, suffix):
    args = CD.parse_args(['--splits', 'train', '--datadir', scene, '--seed', '1234'] + RUNS[suffix])
    lines = []
    paths = CD.convert(args, log=lines.append)
    want_files, want = _shards(os.path.join(golden_dir, 'convert', f'scene_real_train{suffix}'))
    got_files, got = _shards(f'{scene}_real_train{suffix}')
    assert got_files == want_files and [os.path.basename(p) for p in paths] == want_files
    assert len(got_files) == {'': 1, '_full': 5, '_ign': 3}[suffix]
    for f, g, w in zip(got_files, got, want):
        _compare(g, w, f'scene_real_train{suffix}/{f}')
    n = len(got_files)
    assert lines[0].startswith('Read all images and poses, done. all_imgs shape (') and lines[1].startswith('Resize, done. all_imgs shape torch.Size([')
    assert lines[2].startswith('Collect all rays, done. all_data shape torch.Size([')
    assert lines[3:-1] == [f'[{k}/{n}] save_path: {scene}_real_train{suffix}/train_{k}.npy' for k in range(1, n + 1)]
    assert lines[-1] == f'All data saved at "{scene}_real_train{suffix}"'


def test_three_channel_images_are_not_composited(CD, scene, golden_dir, tmp_path):
    """alpha stripped: colours are bytes / 255 (half resolution: their 2 x 2 mean), rays as for the RGBA scene"""
    from efficient_nerf_amd import blender
    from efficient_nerf_amd.frontend import write_png
    rgb_scene = tmp_path / 'rgb'
    (rgb_scene / 'train').mkdir(parents=True)
    shutil.copy(os.path.join(scene, 'transforms_train.json'), str(rgb_scene))
    imgs = []
    for k in range(5):
        im = blender.read_png(os.path.join(scene, 'train', f'r_{k}.png'))[..., :3]
        write_png(str(rgb_scene / 'train' / f'r_{k}.png'), np.ascontiguousarray(im))
        imgs.append(im.astype(np.float64) / 255.)
    imgs = np.array(imgs)
    for full, suffix in ((True, '_full'), (False, '')):
        args = CD.parse_args(['--splits', 'train', '--datadir', str(rgb_scene), '--seed', '1234'] + (['--full_res'] if full else []))
        CD.convert(args, log=lambda *a: None)
        _, got = _shards(f'{rgb_scene}_real_train')
        _, gold = _shards(os.path.join(golden_dir, 'convert', f'scene_real_train{suffix}'))
        px = imgs if full else (imgs[:, 0::2, 0::2] + imgs[:, 0::2, 1::2] + imgs[:, 1::2, 0::2] + imgs[:, 1::2, 1::2]) / 4.
        order = CD.draw_order(px.shape[0] * px.shape[1] * px.shape[2], 1234)
        want_rgb = px.reshape(-1, 3)[order]
        assert len(got) == len(gold)
        for k, (g, w) in enumerate(zip(got, gold)):
            d_rgb = np.abs(g[:, 6:9] - want_rgb[k * 4096:(k + 1) * 4096]).max()
            print(f'RGB scene, full_res={full}, shard {k + 1}: max |colours - bytes / 255| {d_rgb:.2e}')
            assert d_rgb <= TOL
            assert np.array_equal(g[:, :3], w[:, :3]) and np.abs(g[:, 3:6] - w[:, 3:6]).max() <= TOL
        shutil.rmtree(f'{rgb_scene}_real_train')


def test_an_index_outside_the_images_leaves_a_row_of_nan(CD, scene):
    from efficient_nerf_amd import blender
    imgs = np.array([blender.read_png(os.path.join(scene, 'train', f'r_{k}.png')) for k in range(2)])
    poses = np.tile(np.eye(4, dtype=np.float32)[None], (2, 1, 1))
    n = 2 * 32 * 32
    order = np.array([0, n - 1, n, -1, 5], dtype=np.int64)
    out = CD.rays_from_images(imgs, poses, 50., True, order).cpu().numpy()
    assert np.isfinite(out[[0, 1, 4]]).all() and np.isnan(out[[2, 3]]).all()
    with pytest.raises(Exception, match='uint8'):
        CD.rays_from_images(imgs.astype(np.float32), poses, 50., True, order)


def test_command_line_writes_the_same_files(CD, scene, tmp_path):
    """convert_data.py as a child process: the files of the in-process run, bit for bit, and the reference's progress lines"""
    cli_scene = tmp_path / 'scene'
    shutil.copytree(scene, str(cli_scene))
    r = subprocess.run(['timeout', '-k', '10', '120', sys.executable, os.path.join(ROOT, 'convert_data.py'), '--splits', 'train', '--datadir',
                        str(cli_scene), '--seed', '1234'], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f'[1/1] save_path: {cli_scene}_real_train/train_1.npy' in r.stdout and f'All data saved at "{cli_scene}_real_train"' in r.stdout
    CD.convert(CD.parse_args(['--splits', 'train', '--datadir', scene, '--seed', '1234']), log=lambda *a: None)
    _, a = _shards(f'{cli_scene}_real_train')
    _, b = _shards(f'{scene}_real_train')
    assert len(a) == len(b) == 1 and np.array_equal(a[0], b[0])
