"""CPU: the command lines of steps 4 and 5 of the reference's README -- the converter's argument handling
(efficient-nerf_amd/convert_data.py) and the two training flags step 5 needs -- and the C-ABI entry of the conversion kernel."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# README "Step 5" of the reference, as printed there (CUDA_VISIBLE_DEVICES=0 python main.py ...)
STEP5 = ('--model_name R2L --config configs/lego_noview.txt --n_sample_per_ray 16 --netwidth 256 --netdepth 88 --datadir_kd '
         'data/nerf_synthetic/lego_real_train --n_pose_video 20,1,1 --N_iters 1600000 --N_rand 20 --data_mode rays --hard_ratio 0.2 --hard_mul 20 '
         '--use_residual --cache_ignore data,__pycache__,torchsearchsorted,imgs --screen --trial.ON --trial.body_arch resmlp --num_worker 8 '
         '--warmup_lr 0.0001,200 --save_intermediate_models --pretrained_ckpt Experiments/R2L__blender_lego_SERVER/weights/ckpt_1200000.tar '
         '--resume --project R2L__blender_lego__ft')


@pytest.fixture(scope='module')
def CD(pkg):
    from efficient_nerf_amd import convert_data
    return convert_data


def test_step5_command_line_parses(pkg):
    from efficient_nerf_amd.frontend import parse_args
    argv = STEP5.replace('configs/lego_noview.txt', os.path.join(ROOT, 'configs', 'lego_noview.txt')).split()
    a = parse_args(argv)
    assert a.save_intermediate_models is True and a.resume and a.N_iters == 1600000 and a.N_rand == 20 and a.test_pretrained is False
    assert a.datadir_kd == 'data/nerf_synthetic/lego_real_train' and a.i_testset == 2000 and a.dataset_type == 'blender'
    b = parse_args([x for x in argv if x != '--save_intermediate_models'] + ['--test_pretrained'])
    assert b.save_intermediate_models is False and b.test_pretrained is True


def test_save_directory_and_file_names(CD):
    a = CD.parse_args(['--splits', 'train', '--datadir', 'data/nerf_synthetic/lego/'])
    assert CD.save_layout(a) == (['train'], 'train', 'data/nerf_synthetic/lego_real_train')
    assert a.ignore == '' and not a.full_res and a.seed is None
    b = CD.parse_args(['--splits', 'train,val', '--datadir', './data/x', '--suffix', '_v2', '--full_res', '--seed', '7'])
    assert CD.save_layout(b) == (['train', 'val'], 'trainval', 'data/x_real_trainval_v2')
    assert b.full_res and b.seed == 7


def test_ficus_rule_and_ignore_filter(CD):
    a = CD.parse_args(['--splits', 'train', '--datadir', 'data/nerf_synthetic/ficus', '--ignore', '1,2'])
    assert a.ignore == CD.FICUS_IGNORE and len(CD.FICUS_IGNORE.split(',')) == 34 and CD.FICUS_IGNORE.startswith('10,13,14,24,') \
        and CD.FICUS_IGNORE.endswith(',94,97,99')
    frames = [{'file_path': f'./train/r_{k}'} for k in range(100)]
    kept = CD.kept_frames(frames, a.ignore)
    assert len(kept) == 66 and not any(f['file_path'].split('_')[-1] in a.ignore.split(',') for f in kept)
    b = CD.parse_args(['--splits', 'train', '--datadir', 'data/lego', '--ignore', '1,3'])
    assert [f['file_path'] for f in CD.kept_frames(frames[:5], b.ignore)] == ['./train/r_0', './train/r_2', './train/r_4']
    assert len(CD.kept_frames(frames, '')) == 100                      # the default: nothing is ignored (index '1' is not in [''])


def test_the_two_refusals(CD):
    with pytest.raises(SystemExit) as e:
        CD.parse_args(['--splits', 'train', '--datadir', 'd', '--donerf'])
    assert '--donerf' in str(e.value) and '\n' not in str(e.value)
    with pytest.raises(SystemExit) as e:
        CD.output_grid(600, 800, 0.6911, True)
    assert '600 x 800' in str(e.value) and '\n' not in str(e.value)
    H, W, f = CD.output_grid(600, 800, 0.6911, False)                  # at full resolution nothing is resized
    assert (H, W) == (600, 800) and f == .5 * 800 / np.tan(.5 * 0.6911)
    H, W, f2 = CD.output_grid(800, 800, 0.6911, True)
    assert (H, W) == (400, 400) and f2 == f / 2.


def test_order_is_the_two_permutations_composed(CD):
    n = 5 * 32 * 32
    order = CD.draw_order(n, 1234)
    np.random.seed(1234)
    ix1 = np.random.permutation(n)
    ix2 = np.random.permutation(n)
    assert order.dtype == np.int64 and np.array_equal(order, ix1[ix2])
    data = np.arange(n) * 3
    assert np.array_equal(data[ix1][ix2], data[order])                  # all_data[rand_ix1][rand_ix2]
    # without a seed the global stream goes on from where it stands
    np.random.seed(5)
    np.random.rand(3)
    want = np.random.permutation(10)
    want = want[np.random.permutation(10)]
    np.random.seed(5)
    np.random.rand(3)
    assert np.array_equal(CD.draw_order(10), want)


def test_remainder_is_dropped(CD):
    assert CD.SPLIT_SIZE == 4096
    assert [CD.saved_rows(n) for n in (0, 4095, 4096, 5120, 20480, 16000000)] == [0, 0, 4096, 4096, 20480, 3906 * 4096]


def test_entry_point_in_header_and_library(pkg, built_lib):
    src = open(os.path.join(ROOT, 'include', 'r2l_hip.h')).read()
    assert re.search(r'\bint r2l_rays_from_images\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S))
    assert hasattr(ctypes.CDLL(built_lib), 'r2l_rays_from_images')
    from efficient_nerf_amd import _lib
    assert 'r2l_rays_from_images' in _lib.SIGNATURES
    L = _lib.lib()
    buf = ctypes.c_void_p(0x1000)
    assert L.r2l_rays_from_images(None, 1, 8, 8, 4, buf, 10., 0, buf, 4, buf, None) == -1
    assert L.r2l_rays_from_images(buf, 1, 8, 8, 2, buf, 10., 0, buf, 4, buf, None) == -1 and 'channels' in L.r2l_last_error().decode()
    assert L.r2l_rays_from_images(buf, 1, 1, 1, 4, buf, 10., 1, buf, 4, buf, None) == -1 and 'half resolution' in L.r2l_last_error().decode()


def test_a_test_split_without_its_images_is_an_error(pkg, tmp_path):
    """transforms_test.json there, its PNGs not: training must not go on silently without the validation the scene asks for; no
    transforms_test.json, or another dataset type: no test split, and what is missing is named"""
    import json
    from efficient_nerf_amd import train as T
    from efficient_nerf_amd._lib import R2LError
    from efficient_nerf_amd.frontend import parse_args
    base = ['--model_name', 'R2L', '--dataset_type', 'blender', '--datadir', str(tmp_path), '--testskip', '1']
    assert T.load_test_split(parse_args(base)) == (None, f'"{tmp_path}/transforms_test.json"')
    with open(tmp_path / 'transforms_test.json', 'w') as fp:
        json.dump({'camera_angle_x': 0.6911, 'frames': [{'file_path': './test/r_0', 'transform_matrix': np.eye(4).tolist()}]}, fp)
    with pytest.raises(R2LError, match='r_0.png'):
        T.load_test_split(parse_args(base))
    test, missing = T.load_test_split(parse_args(base + ['--dataset_type', 'llff']))
    assert test is None and 'llff' in missing
