"""CPU: the LLFF loader (efficient-nerf_amd/llff.py) against the reference's own run on the fixture scene
(tests/golden/make_golden_llff.py -> tests/golden/llff), the hold-out split, the random poses `create_data rand` draws and the
stream that draws them, the loader's refusals, the new flags, the refusal of an LLFF student without its scene, and the layout
helpers of `convert_data.py --dataset_type llff`.

The loader restates the reference's numpy arithmetic step for step, so every array is compared for equality, to the last bit."""
import os
import shutil

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'llff')
SCENE = os.path.join(GOLD, 'scene')


@pytest.fixture(scope='module')
def L(pkg):
    from efficient_nerf_amd import llff
    return llff


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(GOLD, 'llff_loader.npz')))


def test_loader_matches_the_reference_to_the_last_bit(L, gold):
    images, poses, bds, render_poses, i_test = L.load_llff_data(SCENE, factor=8, n_pose_video=8)
    for name, got in (('images', images), ('poses', poses), ('bds', bds), ('render_poses', render_poses)):
        assert got.dtype == np.float32 and got.shape == gold[name].shape, name
        assert np.array_equal(got, gold[name]), (name, np.abs(got - gold[name]).max())
    assert images.shape == (10, 30, 40, 3) and poses.shape == (10, 3, 5) and bds.shape == (10, 2) and render_poses.shape == (8, 3, 5)
    assert i_test == int(gold['i_test'])
    assert np.array_equal(poses[0, :3, -1], gold['hwf']) and tuple(gold['hwf']) == (30., 40., 37.5)      # focal 300 / factor 8
    # the rescale: the nearest bound of the scene becomes 1 / 0.75
    assert abs(float(bds.min()) - 1. / .75) < 1e-6
    scene = L.load_scene(SCENE)                                # the default path: the loader's own 120 views
    assert scene.hwf == (30, 40, 37.5) and scene.render_poses.shape == (120, 3, 5) and scene.bytes.dtype == np.uint8
    assert np.array_equal(scene.images, images) and np.array_equal(scene.poses, poses)
    assert L.n_pose_video_from_flag('20,4,1') == 120 and L.n_pose_video_from_flag('8') == 8


def test_split_indices(L):
    i_train, i_val, i_test = L.split_indices(10, 8)
    assert list(i_test) == [0, 8] and list(i_val) == [0, 8] and list(i_train) == [1, 2, 3, 4, 5, 6, 7, 9]
    i_train, _, i_test = L.split_indices(20, 8)
    assert list(i_test) == [0, 8, 16] and len(i_train) == 17 and not set(i_train) & set(i_test)
    assert list(L.split_indices(5, 1)[2]) == [0, 1, 2, 3, 4] and len(L.split_indices(5, 1)[0]) == 0
    with pytest.raises(L.LLFFError):
        L.split_indices(10, 0)


def test_random_poses_and_the_stream_that_draws_them(L, gold, pkg):
    """16 get_rand_pose_v2 poses of the reference after np.random.seed(0), each followed by its focal draw: six + one draws per
    pose, and no draws before the first (the LLFF loader consumes none)"""
    from efficient_nerf_amd.create_data import LLFFRandStream
    state = L.load_scene(SCENE).rand_state
    rs = np.random.RandomState(0)
    stream = LLFFRandStream(state)
    for k in range(16):
        pose = L.rand_pose(state, rs)
        assert pose.dtype == np.float32 and np.array_equal(pose, gold['rand_poses'][k]), k
        assert rs.rand() + 1 == gold['rand_focal'][k]
        p = stream.rand_pose()
        assert torch.is_tensor(p) and p.dtype == torch.float32 and np.array_equal(p.numpy(), gold['rand_poses'][k])
        assert stream.rand_focal_scale() == gold['rand_focal'][k]
    assert np.array_equal(stream.rs.get_state()[1], rs.get_state()[1]) and stream.rs.get_state()[2] == rs.get_state()[2]
    # the draws in order: position x, y, z, then viewing axis x, y, z
    u = np.random.RandomState(0).rand(6)
    assert np.array_equal(L.pose_in_boxes(state, u[:3], u[3:]), gold['rand_poses'][0])
    assert not np.array_equal(L.pose_in_boxes(state, u[3:], u[:3]), gold['rand_poses'][0])
    # a pose at the middle of both boxes sits inside the position box; the corners are 1.1 x as far from its middle
    (lo, hi), _ = state.boxes()
    mid = L.pose_in_boxes(state, (.5, .5, .5), (.5, .5, .5), scale=1.1)
    c0, c1 = (L.pose_in_boxes(state, (v,) * 3, (.5, .5, .5))[:3, 3] for v in (0., 1.))
    assert np.all(mid[:3, 3] > lo) and np.all(mid[:3, 3] < hi)
    assert np.allclose(c1 - c0, state.c2w[:3, :3] @ ((hi - lo) * 1.1), atol=1e-6)


def _copy_scene(tmp_path):
    d = tmp_path / 'scene'
    shutil.copytree(SCENE, d)
    return d


def test_the_three_loader_errors(L, tmp_path):
    d = _copy_scene(tmp_path)
    # 1. the folder of the asked factor is not there: named, with the command that makes it, in one line
    with pytest.raises(L.LLFFError) as e:
        L.load_llff_data(str(d), factor=4)
    assert 'images_4' in str(e.value) and 'mogrify -resize 25% -format png' in str(e.value) and '\n' not in str(e.value)
    os.rename(d / 'images_8', d / 'images_x')
    with pytest.raises(L.LLFFError) as e:
        L.load_llff_data(str(d))
    assert 'images_8' in str(e.value) and 'mogrify -resize 12.5% -format png' in str(e.value) and '\n' not in str(e.value)
    os.rename(d / 'images_x', d / 'images_8')
    # 2. a JPEG in the folder is refused by name
    (d / 'images_8' / '004.jpg').write_bytes(b'\xff\xd8\xff')
    with pytest.raises(L.LLFFError) as e:
        L.load_llff_data(str(d))
    assert '004.jpg' in str(e.value) and '\n' not in str(e.value)
    os.remove(d / 'images_8' / '004.jpg')
    # 3. a count that differs from poses_bounds.npy is an error, not a None
    os.remove(d / 'images_8' / '009.png')
    with pytest.raises(L.LLFFError) as e:
        L.load_llff_data(str(d))
    assert '9 PNG' in str(e.value) and '10 pose' in str(e.value) and '\n' not in str(e.value)
    # and --spherify is not built
    with pytest.raises(L.LLFFError, match='not built') as e:
        L.load_llff_data(SCENE, spherify=True)
    assert '\n' not in str(e.value)


def test_loader_writes_nothing(L, tmp_path):
    d = _copy_scene(tmp_path)
    cwd = os.getcwd()
    work = tmp_path / 'cwd'
    work.mkdir()
    os.chdir(work)
    try:
        L.load_llff_data(str(d))
    finally:
        os.chdir(cwd)
    assert os.listdir(work) == [] and sorted(os.listdir(d)) == ['images_8', 'poses_bounds.npy'] and len(os.listdir(d / 'images_8')) == 10


def test_new_flags_and_the_test_set(pkg, gold):
    from efficient_nerf_amd import frontend as fe
    a = fe.parse_args([])
    assert (a.factor, a.llffhold, a.spherify) == (8, 8, False)                 # option.py's defaults
    b = fe.parse_args(['--factor', '4', '--llffhold', '3', '--spherify'])
    assert (b.factor, b.llffhold, b.spherify) == (4, 3, True)
    base = ['--dataset_type', 'llff', '--datadir', SCENE]
    t = fe.parse_args(base + ['--render_test'])
    assert fe.has_llff_scene(t)
    poses, hwf, gt = fe.load_test_set(t)
    assert hwf == (30, 40, 37.5) and poses.shape == (2, 3, 4) and gt.shape == (2, 30, 40, 3) and gt.dtype == torch.float32
    assert np.array_equal(poses.numpy(), gold['poses'][[0, 8]][:, :3, :4]) and np.array_equal(gt.numpy(), gold['images'][[0, 8]])
    # --llffhold 0: the loader's own hold-out, the view nearest the average pose
    poses, _, gt = fe.load_test_set(fe.parse_args(base + ['--render_test', '--llffhold', '0']))
    k = int(gold['i_test'])
    assert poses.shape == (1, 3, 4) and np.array_equal(gt.numpy()[0], gold['images'][k]) and np.array_equal(poses.numpy()[0], gold['poses'][k, :3, :4])
    # without --render_test: the spiral path, no ground truth, no --testskip; an integer --n_pose_video is its length
    poses, hwf, gt = fe.load_test_set(fe.parse_args(base + ['--n_pose_video', '8']))
    assert gt is None and hwf == (30, 40, 37.5) and np.array_equal(poses.numpy(), gold['render_poses'][:, :3, :4])
    assert fe.load_test_set(fe.parse_args(base))[0].shape == (120, 3, 4)        # the Blender triple default: the loader's own 120
    # --synthetic_poses and an unmounted scene keep the synthetic circle
    s = fe.parse_args(base + ['--render_test', '--synthetic_poses', '3', '--H', '10', '--W', '14'])
    assert not fe.has_llff_scene(s)
    poses, hwf, gt = fe.load_test_set(s)
    assert poses.shape == (3, 4, 4) and hwf[:2] == (10, 14) and gt is None
    assert not fe.has_llff_scene(fe.parse_args(['--dataset_type', 'llff', '--datadir', GOLD]))
    assert not fe.has_llff_scene(fe.parse_args(['--dataset_type', 'blender', '--datadir', SCENE]))


def test_llff_student_needs_its_scene(pkg):
    """build_engine without the caller's bounds still refuses an LLFF student, naming why; --no_ndc is as it was"""
    from efficient_nerf_amd import R2LError
    from efficient_nerf_amd import frontend as fe
    base = ['--model_name', 'R2L', '--dataset_type', 'llff', '--netdepth', '88', '--n_sample_per_ray', '16', '--trial.ON',
            '--trial.body_arch', 'resmlp', '--use_residual']
    with pytest.raises(R2LError) as e:
        fe.build_engine(fe.parse_args(base), (30, 40, 37.5), {})
    assert 'poses_bounds.npy' in str(e.value) and 'loaded scene' in str(e.value) and '\n' not in str(e.value)
    with pytest.raises(R2LError, match='--trial.near'):
        fe.build_engine(fe.parse_args(base + ['--no_ndc']), (30, 40, 37.5), {})


def test_training_bounds_and_test_split(pkg, gold, tmp_path):
    from efficient_nerf_amd import train as T
    from efficient_nerf_amd import frontend as fe
    a = fe.parse_args(['--model_name', 'R2L', '--dataset_type', 'llff', '--datadir', SCENE])
    (poses, hwf, gt), missing = T.load_test_split(a)
    assert missing is None and hwf == (30, 40, 37.5) and np.array_equal(poses.numpy(), gold['poses'][[0, 8]][:, :3, :4])
    assert np.array_equal(gt.numpy(), gold['images'][[0, 8]])
    test, missing = T.load_test_split(fe.parse_args(['--model_name', 'R2L', '--dataset_type', 'llff', '--datadir', str(tmp_path)]))
    assert test is None and 'poses_bounds.npy' in missing and 'llff' in missing and '\n' not in missing


def test_converter_layout(pkg):
    from efficient_nerf_amd import convert_data as CD
    a = CD.parse_args(['--dataset_type', 'llff', '--splits', 'train', '--datadir', 'data/nerf_llff_data/fern/'])
    assert a.dataset_type == 'llff' and CD.save_layout(a) == (['train'], 'train', 'data/nerf_llff_data/fern_real_train')
    assert CD.parse_args(['--splits', 'train', '--datadir', 'x']).dataset_type == 'blender'
    b = CD.parse_args(['--dataset_type', 'llff', '--splits', 'train,val', '--datadir', 'd', '--suffix', '_v2', '--ignore', '1', '--seed', '3'])
    assert CD.save_layout(b) == (['train', 'val'], 'trainval', 'd_real_trainval_v2') and b.seed == 3
    assert (CD.LLFF_FACTOR, CD.LLFF_HOLD, CD.SPLIT_SIZE) == (8, 8, 4096)
    assert CD.llff_views(10, ['train']) == [1, 2, 3, 4, 5, 6, 7, 9] and CD.llff_views(10, ['val']) == [0, 8] == CD.llff_views(10, ['test'])
    assert CD.llff_views(10, ['train', 'val', 'test']) == [1, 2, 3, 4, 5, 6, 7, 9, 0, 8] and CD.llff_views(10, ['video']) == []
    assert CD.saved_rows(8 * 30 * 40) == 8192                                    # 2 shards, 1,408 rays dropped
    for flag in ('--full_res', '--donerf'):
        with pytest.raises(SystemExit) as e:
            CD.parse_args(['--dataset_type', 'llff', '--splits', 'train', '--datadir', 'd', flag])
        assert 'llff' in str(e.value).lower() and '\n' not in str(e.value)
    imgs, poses, hwf = CD.load_llff_images(SCENE, ['train'])
    assert imgs.dtype == np.uint8 and imgs.shape == (8, 30, 40, 3) and poses.shape == (8, 3, 4) and poses.dtype == np.float32 and hwf == (30, 40, 37.5)
    with pytest.raises(SystemExit, match='poses_bounds.npy'):                     # a folder that is no scene: the loader's one line
        CD.load_llff_images(os.path.join(GOLD, 'scene_real_train'), ['train'])


def test_byte_to_float_two_ways_differ_by_one_ulp_at_most():
    """the loader computes float32(b / 255.) (the reference's float64 division, then the cast); the conversion kernel divides in
    float32, float32(b) / 255: one correctly rounded operation against two roundings, so at most 1 ulp apart for every byte.  That
    is what the converter's 5e-7 colour bound has to cover (1 ulp below 1 is 6e-8)."""
    b = np.arange(256)
    one = (b / 255.).astype(np.float32)
    two = b.astype(np.float32) / np.float32(255.)
    assert two.dtype == np.float32
    ulp = np.spacing(np.maximum(one, two))
    assert np.all(np.abs(one.astype(np.float64) - two.astype(np.float64)) <= ulp)
    print(f'{int((one != two).sum())} of 256 bytes differ, largest difference {np.abs(one - two).max():.2e}')
