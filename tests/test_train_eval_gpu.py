"""GPU: test renders while the student trains (efficient-nerf_amd/train.py: R2LTrainer.render_rays / render, the --i_testset loop of
train(), ckpt_best.tar, --save_intermediate_models, best_psnr under --resume).

render_rays launches the kernels generic.GenericR2L launches, and their arithmetic is per row: the yardstick is bit-identity.  The
runs that are compared bit for bit are made in this process on seeded generators (the command line seeds nothing, as the reference's
does not); the command line itself runs once as a child process for its log, its files and main.py --render_only on what it wrote."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, N_TRAIN, N_TEST, ANGLE = 16, 32, 3, 0.6911
NET = ['--model_name', 'R2L', '--dataset_type', 'blender', '--white_bkgd', '--testskip', '1', '--netdepth', '8', '--netwidth', '64',
       '--n_sample_per_ray', '4', '--multires', '4', '--use_residual', '--trial.ON', '--trial.body_arch', 'resmlp']
TRAIN = ['--data_mode', 'rays', '--N_rand', '2', '--N_iters', '6', '--i_testset', '3', '--i_weights', '3', '--save_intermediate_models', '--i_print', '1']
TEST_LINE = re.compile(r'^\[TEST\] Iter (\d+) TestPSNR (\S+) TestPSNRv2 (\S+) BestPSNRv2 (\S+) \(Iter (\d+)\) TestSSIM (\S+) TrainHistPSNR (\S+) '
                       r'LR (\d\.\d{8}) Time (\S+)s$')


# ---- 1. render_rays ----------------------------------------------------------------------------------------------------------
def _rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0., 0., 4.]) + 0.2 * torch.randn(n, 3, generator=g)
    d = -o + 0.8 * torch.randn(n, 3, generator=g)
    return o.cuda(), (d / d.norm(dim=-1, keepdim=True)).cuda(), torch.rand(n, 3, generator=g).cuda()


def test_render_rays_is_generic_r2l_bit_for_bit(pkg, built_lib):
    """n = 2 max_rays + 37 rays (three chunks, the last one ragged) on a W64 netdepth-8 ResMLP with the global skip, before and
    after a training step; the step's state (weights, gradients, moments, loss, per-ray error) is as the step left it"""
    from efficient_nerf_amd.generic import GenericR2L
    from efficient_nerf_amd.train import R2LTrainer, init_state_dict
    kw = dict(n_sample=4, L=4, netdepth=8, netwidth=64, use_residual=True, trial=dict(body_arch='resmlp'))
    max_rays = 256
    n = 2 * max_rays + 37
    tr = R2LTrainer(max_rays=max_rays, **kw)
    tr.load_state_dict(init_state_dict(tr.plan, seed=3))
    ro, rd, _ = _rays(n, 1)
    H = W = 16
    focal = .5 * W / np.tan(.5 * ANGLE)
    c2w = torch.tensor([[1., 0, 0, 0.1], [0, 0.8, -0.6, 2.4], [0, 0.6, 0.8, 3.2]])

    def compare():
        gen = GenericR2L(H, W, focal, **kw).load_state_dict(tr.state_dict())
        rng = torch.cuda.get_rng_state()
        got = tr.render_rays(ro, rd)
        assert got.shape == (n, 3) and torch.isfinite(got).all() and torch.equal(rng, torch.cuda.get_rng_state())      # no draws
        assert torch.equal(got, gen.render_rays(ro, rd))
        assert torch.equal(tr.render(c2w, H, W, focal), gen.render(c2w))

    compare()
    bo, bd, tgt = _rays(200, 2)
    loss, err = tr.step(bo, bd, tgt, 1e-3, perturb=0.)
    keep = [t.clone() for t in (tr._param, tr._grad, tr._m, tr._v, loss, err)]
    compare()                                                           # the live weights, not the loaded ones
    assert all(torch.equal(a, b) for a, b in zip(keep, (tr._param, tr._grad, tr._m, tr._v, loss, err)))
    with pytest.raises(Exception, match='expected'):
        tr.render_rays(ro, rd[:5])


# ---- 2. the loop -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene(pkg, built_lib, tmp_path_factory):
    """16 x 16 RGBA views of a soft-edged disc on cameras around the origin: 32 train views (two shards of 4096 rays from
    convert_data) and three test views"""
    from efficient_nerf_amd import convert_data as CD
    from efficient_nerf_amd.frontend import pose_spherical, write_png
    root = tmp_path_factory.mktemp('train_eval')
    d = root / 'scene'
    y, x = np.meshgrid(np.arange(SIZE), np.arange(SIZE), indexing='ij')
    for split, n in (('train', N_TRAIN), ('test', N_TEST)):
        (d / split).mkdir(parents=True)
        frames = []
        for k in range(n):
            theta = 360. * k / n + (0. if split == 'train' else 17.)
            img = np.zeros((SIZE, SIZE, 4), dtype=np.uint8)
            for c in range(3):
                img[..., c] = np.clip(127.5 + 127.5 * np.sin(0.4 * x + 0.3 * y * (c + 1) + np.radians(theta) + c), 0, 255)
            img[..., 3] = np.clip(255. * (7.5 - np.hypot(x - 7.5, y - 7.5)) / 3., 0, 255)
            write_png(str(d / split / f'r_{k}.png'), img)
            frames.append({'file_path': f'./{split}/r_{k}', 'transform_matrix': pose_spherical(theta, -30., 4.).tolist()})
        with open(d / f'transforms_{split}.json', 'w') as fp:
            json.dump({'camera_angle_x': ANGLE, 'frames': frames}, fp)
    paths = CD.convert(CD.parse_args(['--splits', 'train', '--datadir', str(d), '--full_res', '--seed', '1']), log=lambda *a: None)
    assert len(paths) == 2
    (root / 'empty').mkdir()
    return {'root': str(root), 'datadir': str(d), 'shards': f'{d}_real_train', 'empty': str(root / 'empty')}


def _argv(scene, expname, datadir=None, extra=()):
    return NET + TRAIN + ['--datadir', datadir or scene['datadir'], '--datadir_kd', scene['shards'], '--basedir', scene['root'],
                          '--expname', expname] + list(extra)


def _weights(path):
    ck = torch.load(path, map_location='cpu', weights_only=False)
    return ck, ck['network_fn_state_dict']


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.fixture(scope='module')
def cli(scene):
    r = subprocess.run(['timeout', '-k', '10', '240', sys.executable, os.path.join(ROOT, 'main.py')] + _argv(scene, 'cli'), cwd=scene['root'],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_prints_test_lines_and_writes_the_best_checkpoint(scene, cli):
    lines = [TEST_LINE.match(ln) for ln in cli.splitlines() if ln.startswith('[TEST] Iter')]
    assert len(lines) == 2 and all(lines), cli[-3000:]
    assert [int(m.group(1)) for m in lines] == [3, 6] and 'Iter 3 Testing...' in cli and 'Iter 6 Testing...' in cli
    assert all(np.isfinite(float(m.group(g))) for m in lines for g in (2, 3, 4, 6, 7, 9))
    exp = os.path.join(scene['root'], 'cli')
    w = os.path.join(exp, 'weights')
    assert sorted(os.listdir(w)) == ['ckpt_3.tar', 'ckpt_6.tar', 'ckpt_best.tar']
    for it in (3, 6):
        assert sorted(os.listdir(os.path.join(exp, f'testset_iter{it}'))) == [f'{k:03d}.png' for k in range(N_TEST)]
    from efficient_nerf_amd.blender import read_png
    assert read_png(os.path.join(exp, 'testset_iter6', '002.png')).shape == (SIZE, SIZE, 3)
    v2 = [float(m.group(3)) for m in lines]
    best, best_sd = _weights(os.path.join(w, 'ckpt_best.tar'))
    step = 3 if v2[0] >= v2[1] else 6                                   # a later render replaces the best only when it is better
    assert abs(best['best_psnr'] - max(v2)) <= 5e-5 and best['best_psnr_step'] == step == best['global_step']
    assert _same(best_sd, _weights(os.path.join(w, f'ckpt_{step}.tar'))[1])
    assert float(lines[1].group(4)) == max(v2) and int(lines[1].group(5)) == step
    last, _ = _weights(os.path.join(w, 'ckpt_6.tar'))
    assert last['best_psnr'] == best['best_psnr'] and last['best_psnr_step'] == step and last['global_step'] == 6


def test_render_only_reports_the_same_test_psnr(scene, cli):
    ck = os.path.join(scene['root'], 'cli', 'weights', 'ckpt_6.tar')
    r = subprocess.run(['timeout', '-k', '10', '240', sys.executable, os.path.join(ROOT, 'main.py')] + NET + [
        '--datadir', scene['datadir'], '--render_only', '--render_test', '--precision', 'fp32', '--pretrained_ckpt', ck, '--basedir', scene['root'],
        '--expname', 'render'], cwd=scene['root'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = re.search(r'^\[TEST\] TestPSNR (\S+) TestPSNRv2 (\S+) TestSSIM (\S+)$', r.stdout, re.M)
    want = [TEST_LINE.match(ln) for ln in cli.splitlines() if ln.startswith('[TEST] Iter 6 ')][0]
    assert got, r.stdout[-3000:]
    print(f'Iter 6 while training: TestPSNR {want.group(2)} TestPSNRv2 {want.group(3)} TestSSIM {want.group(6)}; --render_only: {got.groups()}')
    assert abs(float(got.group(1)) - float(want.group(2))) <= 1e-4
    assert abs(float(got.group(2)) - float(want.group(3))) <= 1e-4 and abs(float(got.group(3)) - float(want.group(6))) <= 1e-4


def _train(scene, expname, datadir=None, extra=(), rng=None, seed=11):
    """train() in this process on seeded generators (or the given numpy / device generator states); returns the log lines and
    the generator states at the moment 'Iter 3 Save checkpoint' was logged"""
    from efficient_nerf_amd import train as T
    from efficient_nerf_amd.frontend import parse_args
    lines, at3 = [], []

    def log(msg):
        lines.append(msg)
        if msg.startswith('Iter 3 Save checkpoint'):
            at3.append((np.random.get_state(), torch.cuda.get_rng_state()))

    np.random.seed(seed)
    torch.manual_seed(seed)
    if rng is not None:
        np.random.set_state(rng[0])
        torch.cuda.set_rng_state(rng[1])
    T.train(parse_args(_argv(scene, expname, datadir, extra)), log=log)
    return lines, (at3[0] if at3 else None)


@pytest.fixture(scope='module')
def with_tests(scene):
    return _train(scene, 'a')


def test_without_a_test_split_training_is_unchanged(scene, with_tests):
    """--datadir without transforms_test.json: one notice, no [TEST] line, and the weights of the run with test renders bit for bit"""
    lines, _ = _train(scene, 'b', datadir=scene['empty'])
    notice = [ln for ln in lines if ln.startswith('No test renders')]
    assert len(notice) == 1 and 'transforms_test.json' in notice[0] and '\n' not in notice[0]
    assert not any(ln.startswith('[TEST]') or 'Testing...' in ln for ln in lines)
    assert sum(ln.startswith('[TEST] Iter') for ln in with_tests[0]) == 2
    w = lambda e, f: os.path.join(scene['root'], e, 'weights', f)
    assert sorted(os.listdir(os.path.dirname(w('b', '')))) == ['ckpt_3.tar', 'ckpt_6.tar']          # no ckpt_best.tar
    for f in ('ckpt_3.tar', 'ckpt_6.tar'):
        a, b = torch.load(w('a', f), weights_only=False), torch.load(w('b', f), weights_only=False)
        assert _same(a['network_fn_state_dict'], b['network_fn_state_dict'])
        sa, sb = a['optimizer_state_dict']['state'], b['optimizer_state_dict']['state']
        assert all(torch.equal(sa[k][m], sb[k][m]) for k in sa for m in ('exp_avg', 'exp_avg_sq'))
        assert b['best_psnr'] == 0 and b['best_psnr_step'] == 0
    other = _weights(w('b', 'ckpt_6.tar'))[1]
    assert not _same(other, _weights(w('b', 'ckpt_3.tar'))[1])          # and training moved them
    # another dataset type: the same notice, naming it
    from efficient_nerf_amd import train as T
    from efficient_nerf_amd.frontend import parse_args
    test, missing = T.load_test_split(parse_args(_argv(scene, 'x', extra=['--dataset_type', 'llff'])))
    assert test is None and 'llff' in missing


def test_resume_restores_the_best_psnr_and_ends_where_the_whole_run_ends(scene, with_tests):
    lines_a, at3 = with_tests
    w = lambda e, f: os.path.join(scene['root'], e, 'weights', f)
    ck3 = torch.load(w('a', 'ckpt_3.tar'), weights_only=False)
    assert ck3['best_psnr'] > 0 and ck3['best_psnr_step'] == 3
    lines_c, _ = _train(scene, 'c', extra=['--pretrained_ckpt', w('a', 'ckpt_3.tar'), '--resume'], rng=at3)
    assert 'Resume optimizer successfully.' in lines_c and not any(ln.startswith('[TRAIN] Iter 3 ') for ln in lines_c)
    ta = [TEST_LINE.match(ln) for ln in lines_a if ln.startswith('[TEST] Iter 6 ')][0]
    tc = [TEST_LINE.match(ln) for ln in lines_c if ln.startswith('[TEST] Iter')]
    assert len(tc) == 1 and tc[0].group(1) == '6'
    assert tc[0].groups()[1:5] == ta.groups()[1:5]                     # TestPSNR, TestPSNRv2, BestPSNRv2, (Iter s)
    assert abs(float(tc[0].group(6)) - float(ta.group(6))) <= 1e-4     # TestSSIM: a library convolution, to the print's resolution
    a, c = torch.load(w('a', 'ckpt_6.tar'), weights_only=False), torch.load(w('c', 'ckpt_6.tar'), weights_only=False)
    assert _same(a['network_fn_state_dict'], c['network_fn_state_dict'])
    sa, sc = a['optimizer_state_dict']['state'], c['optimizer_state_dict']['state']
    assert all(torch.equal(sa[k][m], sc[k][m]) for k in sa for m in ('exp_avg', 'exp_avg_sq', 'step'))
    assert (c['best_psnr'], c['best_psnr_step'], c['global_step']) == (a['best_psnr'], a['best_psnr_step'], 6)
    if a['best_psnr_step'] == 3:                                        # the best is the checkpoint's: the resumed run wrote no better one
        assert not os.path.exists(w('c', 'ckpt_best.tar')) and c['best_psnr'] == ck3['best_psnr']


def test_test_pretrained(scene, with_tests):
    w = os.path.join(scene['root'], 'a', 'weights', 'ckpt_6.tar')
    lines, _ = _train(scene, 'd', extra=['--pretrained_ckpt', w, '--test_pretrained', '--N_iters', '0'])
    got = [re.match(r'^Pretrained test: TestPSNR (\S+) TestPSNRv2 (\S+)$', ln) for ln in lines if ln.startswith('Pretrained test')]
    want = [TEST_LINE.match(ln) for ln in with_tests[0] if ln.startswith('[TEST] Iter 6 ')][0]
    assert len(got) == 1 and got[0].groups() == want.groups()[1:3]
    with pytest.raises(SystemExit) as e:
        _train(scene, 'e', datadir=scene['empty'], extra=['--pretrained_ckpt', w, '--test_pretrained'])
    assert 'transforms_test.json' in str(e.value) and '\n' not in str(e.value)


def test_i_testset_zero_renders_nothing(scene):
    lines, _ = _train(scene, 'f', extra=['--i_testset', '0', '--N_iters', '2'])
    assert any('--i_testset 0' in ln for ln in lines if ln.startswith('Test split'))
    assert not any(ln.startswith('[TEST]') for ln in lines) and any(ln.startswith('[TRAIN] Iter 2 ') for ln in lines)
