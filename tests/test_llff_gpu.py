"""GPU: an LLFF scene through every step of the student pipeline -- converter, student engine at near = 0 on a non-square frame,
the two render command lines, three training iterations with a test render, and `create_data rand` on the NDC teacher.

The scene is tests/golden/llff/scene (tests/golden/make_golden_llff.py): 10 views of 30 x 40, focal 37.5; with every 8th view held
out the test views are {0, 8}.  A frame is 1,200 rays = 9.375 ray tiles of 128: no launch here is a whole number of tiles.  The
expected values are the reference's own shards, and the CPU oracle (oracle/r2l_oracle.py) at near, far = 0, 1."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'llff')
SCENE = os.path.join(GOLD, 'scene')
H, W, FOCAL = 30, 40, 37.5
TEST_VIEWS = [0, 8]
R2L_NET = ['--model_name', 'R2L', '--n_sample_per_ray', '16', '--netwidth', '256', '--use_residual', '--trial.ON', '--trial.body_arch', 'resmlp']
TEACHER_NET = ['--model_name', 'nerf', '--use_viewdirs', '--N_importance', '128']
CHUNK = 100
LLFF = ['--dataset_type', 'llff', '--factor', '8', '--llffhold', '8', '--datadir', SCENE]


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(os.path.join(GOLD, 'llff_loader.npz')))


@pytest.fixture(scope='module')
def test_poses(gold):
    return torch.from_numpy(gold['poses'][TEST_VIEWS][:, :3, :4].copy())


@pytest.fixture(scope='module')
def teacher():
    return O.make_teacher_state(1), O.make_teacher_state(2)


def run(script, args, cwd):
    r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def ndc_teacher(teacher, rays_o, rays_d, focal):
    """the reference's render(..., ndc=True) of given world-space rays: view directions first, then ndc_rays(H, W, focal, 1., ...) and
    the two passes over [0, 1] (main.py:148-162, 624-756)"""
    vd = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
    o, d = O.ndc_rays(H, W, focal, 1., rays_o, rays_d)
    with torch.no_grad():       # 100 rays at a time: the layer outputs of a chunk stay in the cache, 2.5 x the speed of one call
        return torch.cat([O.render_rays(teacher[0], teacher[1], o[s:s + CHUNK], d[s:s + CHUNK], near=0., far=1., white_bkgd=False,
                                        viewdirs=vd[s:s + CHUNK])['rgb_map'] for s in range(0, o.shape[0], CHUNK)], 0)


# ---- converter -------------------------------------------------------------------------------------------------------------------
def test_converter_against_the_reference_shards(pkg, built_lib, tmp_path):
    """convert_data.py --dataset_type llff on the fixture against the reference's two shards, row for row: origins bit-equal,
    directions and colours within 5e-7 (tests/test_convert_gpu.py's bounds)"""
    from efficient_nerf_amd import convert_data as CD
    scene = tmp_path / 'scene'
    shutil.copytree(SCENE, scene)
    lines = []
    paths = CD.convert(CD.parse_args(['--dataset_type', 'llff', '--splits', 'train', '--datadir', str(scene), '--seed', '1234']), log=lines.append)
    assert paths == [f'{scene}_real_train/train_1.npy', f'{scene}_real_train/train_2.npy']
    assert sorted(os.listdir(f'{scene}_real_train')) == ['train_1.npy', 'train_2.npy']            # 9,600 rays: 1,408 dropped
    assert any('all_data shape torch.Size([9600, 9])' in ln for ln in lines)
    for k, p in enumerate(paths, 1):
        got, want = np.load(p), np.load(os.path.join(GOLD, 'scene_real_train', f'train_{k}.npy'))
        assert got.dtype == np.float32 and got.shape == want.shape == (4096, 9)
        d = np.abs(got - want)
        print(f'train_{k}: origins {d[:, :3].max():.1e} directions {d[:, 3:6].max():.1e} colours {d[:, 6:].max():.1e}')
        assert np.array_equal(got[:, :3], want[:, :3])
        assert d[:, 3:6].max() <= 5e-7 and d[:, 6:].max() <= 5e-7


# ---- student engine --------------------------------------------------------------------------------------------------------------
def test_student_engine_at_near_zero_on_a_ragged_frame(pkg, built_lib, test_poses):
    """R2LEngine(30, 40, focal, 0., 1.): 1,200 rays = 9.375 tiles, depths from 0, full depth; fp16x3 and the rung `auto` chooses
    against the CPU oracle, every ray within the README's 1e-4"""
    from efficient_nerf_amd import R2LEngine
    sd = O.make_r2l_state()
    c2w = test_poses[0]
    ref = O.r2l_render(sd, H, W, FOCAL, c2w, near=0., far=1.)
    assert ref.shape == (H * W, 3)
    eng = R2LEngine(H, W, FOCAL, 0., 1.).load_state_dict(sd)
    assert torch.equal(eng.z_vals, torch.linspace(0., 1., 16))
    got = eng.render(c2w).cpu()
    e3 = (got - ref).abs().max().item()
    name, _ = eng.choose_precision(c2w=c2w)
    auto = eng.render_checked(lambda: eng.render(c2w))[0].cpu()
    ea = (auto - ref).abs().max().item()
    eng.close()
    print(f'L_inf against the CPU oracle: fp16x3 {e3:.2e}, auto -> {name} {ea:.2e}')
    assert got.shape == (H * W, 3) and torch.isfinite(got).all() and torch.isfinite(auto).all()
    assert e3 <= 1e-4 and ea <= 1e-4


# ---- student command line --------------------------------------------------------------------------------------------------------
def test_student_render_test_command_line(pkg, built_lib, gold, test_poses, tmp_path):
    """main.py --model_name R2L --render_only --render_test on the mounted scene: the two held-out views as 30 x 40 frames equal to
    the engine's own, PSNR and SSIM against the fixture's images on the [TEST] line"""
    from efficient_nerf_amd import R2LEngine, PRECISIONS
    from efficient_nerf_amd import frontend as fe
    from efficient_nerf_amd.blender import read_png
    sd = O.make_r2l_state(seed=4, netdepth=6)
    ck = str(tmp_path / 'r2l.tar')
    fe.save_checkpoint(ck, sd)
    out = str(tmp_path / 'out')
    log = run('main.py', R2L_NET + ['--netdepth', '6', '--render_only', '--render_test', '--pretrained_ckpt', ck, '--precision', 'fp16x3', '--outdir', out] + LLFF,
              cwd=str(tmp_path))
    rgbs = np.load(os.path.join(out, 'rgbs.npy'))
    assert rgbs.shape == (2, H, W, 3)
    eng = R2LEngine(H, W, FOCAL, 0., 1., n_block=2, precision=PRECISIONS['fp16x3']).load_state_dict(sd)
    mine = eng.render_batch(test_poses.cuda()).cpu().numpy().reshape(2, H, W, 3)
    eng.close()
    assert np.array_equal(rgbs, mine)
    for k in range(2):
        ref = O.r2l_render(sd, H, W, FOCAL, test_poses[k], near=0., far=1.).view(H, W, 3).numpy()
        assert np.abs(rgbs[k] - ref).max() <= 1e-4
        png = read_png(os.path.join(out, f'{k:03d}.png'))
        assert png.shape == (H, W, 3) and np.array_equal(png, fe.to8b(rgbs[k]))
        assert np.array_equal(read_png(os.path.join(out, f'{k:03d}_gt.png')), fe.to8b(gold['images'][TEST_VIEWS[k]]))
    m = re.search(r'^\[TEST\] TestPSNR (\S+) TestPSNRv2 (\S+) TestSSIM (\S+)$', log, re.M)
    assert m, log[-3000:]
    gt = gold['images'][TEST_VIEWS]
    psnr = -10. * np.log10(np.mean((rgbs.astype(np.float64) - gt) ** 2))
    v2 = np.mean([-10. * np.log10(np.mean((rgbs[k].astype(np.float64) - gt[k]) ** 2)) for k in range(2)])
    assert abs(float(m.group(1)) - psnr) <= 1e-3 and abs(float(m.group(2)) - v2) <= 1e-3 and -1. <= float(m.group(3)) <= 1.
    assert f'{H}x{W}' in log


# ---- teacher command line --------------------------------------------------------------------------------------------------------
def test_teacher_render_test_command_line(pkg, built_lib, gold, test_poses, teacher, tmp_path):
    """the same command with --model_name nerf --precision fp16x3: the NDC teacher on the scene's own held-out poses, every ray
    within 1e-4 of the oracle (the bound test_teacher_llff_ndc_cli holds its frame to)"""
    from efficient_nerf_amd import frontend as fe
    ck = str(tmp_path / 'nerf.tar')
    fe.save_checkpoint(ck, *teacher)
    out = str(tmp_path / 'out')
    log = run('main.py', TEACHER_NET + ['--render_only', '--render_test', '--pretrained_ckpt', ck, '--precision', 'fp16x3', '--outdir', out] + LLFF,
              cwd=str(tmp_path))
    rgbs = np.load(os.path.join(out, 'rgbs.npy'))
    assert rgbs.shape == (2, H, W, 3)
    for k in range(2):
        ref = O.teacher_render(teacher[0], teacher[1], H, W, FOCAL, test_poses[k], chunk=CHUNK, ndc=True, near=0., far=1., white_bkgd=False)['rgb_map'].numpy()
        d = np.abs(rgbs[k].reshape(-1, 3) - ref).max()
        print(f'view {TEST_VIEWS[k]}: L_inf against the oracle {d:.2e}')
        assert d <= 1e-4
    assert re.search(r'^\[TEST\] TestPSNR (\S+) TestPSNRv2 (\S+) TestSSIM (\S+)$', log, re.M), log[-3000:]


# ---- training --------------------------------------------------------------------------------------------------------------------
def test_three_iterations_with_a_test_render(pkg, built_lib, tmp_path):
    """three iterations on the reference's two shards with a small generic network: depths linspace(0, 1, n); --i_testset 2 renders
    the two held-out views once, and the weights at the end are those of a run that never rendered, bit for bit"""
    from efficient_nerf_amd import train as T
    from efficient_nerf_amd.blender import read_png
    from efficient_nerf_amd.frontend import parse_args
    net = ['--model_name', 'R2L', '--netdepth', '8', '--netwidth', '64', '--n_sample_per_ray', '4', '--multires', '4', '--use_residual', '--trial.ON',
           '--trial.body_arch', 'resmlp']
    base = net + LLFF + ['--data_mode', 'rays', '--datadir_kd', os.path.join(GOLD, 'scene_real_train'), '--N_rand', '1', '--N_iters', '3',
                         '--i_weights', '3', '--i_print', '1', '--basedir', str(tmp_path)]
    tr = T.trainer_from_args(parse_args(base), 64)
    assert torch.equal(tr.z_vals, torch.linspace(0., 1., 4))

    def train(expname, i_testset):
        lines = []
        np.random.seed(11)
        torch.manual_seed(11)
        T.train(parse_args(base + ['--expname', expname, '--i_testset', str(i_testset)]), log=lines.append)
        return lines

    with_test, without = train('a', 2), train('b', 0)
    tests = [ln for ln in with_test if ln.startswith('[TEST] Iter')]
    assert len(tests) == 1 and tests[0].startswith('[TEST] Iter 2 TestPSNR '), with_test
    assert any(ln.startswith('Test split: 2 view(s) 30 x 40') for ln in with_test)
    assert not any(ln.startswith('[TEST]') for ln in without)
    d = tmp_path / 'a' / 'testset_iter2'
    assert sorted(os.listdir(d)) == ['000.png', '001.png'] and all(read_png(str(d / f)).shape == (H, W, 3) for f in os.listdir(d))
    a = torch.load(tmp_path / 'a' / 'weights' / 'ckpt.tar', weights_only=False)
    b = torch.load(tmp_path / 'b' / 'weights' / 'ckpt.tar', weights_only=False)
    sa, sb = a['network_fn_state_dict'], b['network_fn_state_dict']
    assert a['global_step'] == b['global_step'] == 3 and list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert os.path.exists(tmp_path / 'a' / 'weights' / 'ckpt_best.tar') and not os.path.exists(tmp_path / 'b' / 'weights' / 'ckpt_best.tar')


# ---- create_data -----------------------------------------------------------------------------------------------------------------
def test_create_data_rand_on_the_ndc_teacher(pkg, built_lib, gold, teacher, tmp_path):
    """create_data.py --create_data rand on the scene: 4 poses in groups of 2, shards of 512 rays (2,400 rays a group: 4 shards, 352
    rays dropped).  With the stream's two permutations undone, the ray columns are get_rays at the reference's random poses and
    focals, bit for bit, and rgb is the NDC teacher projected with the BASE focal (utils/create_data.py:819-831 hands render
    `focal`, not `focal_`): within 1e-4 of the oracle on every row, and far from a projection with the pose's own focal"""
    from efficient_nerf_amd import frontend as fe
    from efficient_nerf_amd import llff
    ck = str(tmp_path / 'nerf.tar')
    fe.save_checkpoint(ck, *teacher)
    out = str(tmp_path / 'pseudo')
    log = run('create_data.py', ['--create_data', 'rand', '--teacher_ckpt', ck, '--n_pose_kd', '4', '--datadir_kd', f'unused:{out}', '--create_data_chunk', '2',
                                 '--split_size', '512', '--precision', 'fp16x3'] + TEACHER_NET + LLFF, cwd=str(tmp_path))
    assert 'wrote 8 shard(s) of 512 rays; 4 poses in' in log, log[-1500:]
    assert sorted(f for f in os.listdir(out) if f.endswith('.npy')) == [f'data_{k}.npy' for k in range(1, 9)]
    state = llff.load_scene(SCENE).rand_state
    rs = np.random.RandomState(0)
    n = 2 * H * W
    worst, apart = 0., []
    for g in range(2):
        poses = []
        for j in range(2):
            pose = llff.rand_pose(state, rs)
            focal_k = FOCAL * (rs.rand() + 1)
            if g == 0:          # the first group's draws are the first of the reference's stream
                assert np.array_equal(pose, gold['rand_poses'][j]) and focal_k == FOCAL * gold['rand_focal'][j]
            poses.append((torch.from_numpy(pose[:3, :4].copy()), focal_k))
        ix1, ix2 = rs.permutation(n), rs.permutation(n)
        order = ix1[ix2][:4 * 512]
        got = np.concatenate([np.load(os.path.join(out, f'data_{4 * g + k}.npy')) for k in range(1, 5)], 0)
        assert got.shape == (2048, 9) and got.dtype == np.float32
        rows = np.full((n, 9), np.nan, dtype=np.float32)
        rows[order] = got                                         # the permutations undone: pose-major, row-major inside a pose
        for j, (pose, focal_k) in enumerate(poses):
            kept = np.nonzero(~np.isnan(rows[j * H * W:(j + 1) * H * W, 0]))[0]
            mine = rows[j * H * W:(j + 1) * H * W][kept]
            ro, rd = (t.reshape(-1, 3).float()[kept] for t in O.get_rays(H, W, focal_k, pose))
            assert np.array_equal(mine[:, :3], ro.numpy()) and np.array_equal(mine[:, 3:6], rd.numpy())
            d = np.abs(mine[:, 6:] - ndc_teacher(teacher, ro, rd, FOCAL).numpy()).max()
            worst = max(worst, d)
            if j == 0:          # the other reading of the reference's loop, on every 5th kept row of the pose
                base = ndc_teacher(teacher, ro[::5], rd[::5], FOCAL).numpy()
                other = ndc_teacher(teacher, ro[::5], rd[::5], focal_k).numpy()
                apart.append((np.abs(base - other).max(), np.abs(mine[::5, 6:] - other).max()))
            print(f'group {g} pose {j}: {len(kept)} rows kept, focal x {focal_k / FOCAL:.3f}, rgb L_inf against the oracle at the base focal {d:.2e}' +
                  (f'; the two projections are {apart[-1][0]:.2e} apart in the oracle, the shard is {apart[-1][1]:.2e} from the other one' if j == 0 else ''))
            assert d <= 1e-4
    # the oracle's two projections differ by several times the 1e-4 bound on these poses (focal x 1.4 and more), so a shard
    # within 1e-4 of one is at least that much less than their distance from the other: it follows the base-focal projection
    for sep, far in apart:
        assert sep >= 3e-4 and far >= sep - 1e-4, apart


def test_auto_measures_on_poses_of_the_scene(pkg, built_lib, gold, teacher):
    """create_data's `--precision auto` on an LLFF scene: the probe rays are get_rays of the average pose and of two opposite corners
    of the 1.1-scaled position box at focal x 1, 1.5 and 2; the NDC engine it builds ends on a rung of the ladder and renders a random
    pose of the stream inside the 1e-4 contract"""
    from efficient_nerf_amd import create_data as CDm
    from efficient_nerf_amd import frontend as fe
    from efficient_nerf_amd import llff
    state = llff.load_scene(SCENE).rand_state
    sets = CDm.llff_probe_rays(state, H, W, FOCAL, 'cuda')
    assert len(sets) == 3 and all(o.shape == d.shape == (H * W, 3) for o, d in sets)
    want = [(state.c2w[:3, :4].astype(np.float32), 1.), (llff.pose_in_boxes(state, (0., 0., 0.), (.5, .5, .5))[:3, :4], 1.5),
            (llff.pose_in_boxes(state, (1., 1., 1.), (.5, .5, .5))[:3, :4], 2.)]
    for (o, d), (pose, fs) in zip(sets, want):
        ro, rd = (t.reshape(-1, 3) for t in O.get_rays(H, W, FOCAL * fs, torch.from_numpy(np.ascontiguousarray(pose))))
        assert torch.equal(o.cpu(), ro) and torch.equal(d.cpu(), rd)
    (lo, hi), _ = state.boxes()
    corners = np.stack([w[0][:, 3] for w in want[1:]])
    assert np.all(corners[0] < state.c2w[:3, :3] @ lo + state.c2w[:3, 3] + 1e-6) and np.all(corners[1] > state.c2w[:3, :3] @ hi + state.c2w[:3, 3] - 1e-6)
    lines = []
    eng = CDm.build_llff_teacher_engine(fe.parse_args(TEACHER_NET + LLFF), {'network_fn_state_dict': teacher[0], 'network_fine_state_dict': teacher[1]},
                                        (H, W, FOCAL), state, log=lines.append)
    assert eng.ndc and eng.precision_name in eng.LADDER and len(lines) == 1 and lines[0].startswith('[precision] auto:'), lines
    pose, focal_k = torch.from_numpy(gold['rand_poses'][0][:3, :4].copy()), FOCAL * gold['rand_focal'][0]
    ro, rd = (t.reshape(-1, 3).float() for t in O.get_rays(H, W, focal_k, pose))
    got = eng.render_rays(ro.cuda(), rd.cuda())['rgb_map'].cpu()
    d = (got - ndc_teacher(teacher, ro, rd, FOCAL)).abs().max().item()
    print(f'auto -> {eng.precision_name}: rgb L_inf against the oracle {d:.2e} ({lines[0]})')
    eng.close()
    assert d <= 1e-4
