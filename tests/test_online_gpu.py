"""GPU: online distillation (csrc/r2l_online.hip, efficient-nerf_amd/online.py, the --kd_online branch of train.train).

The kernel against the numpy mirror of tests/test_online_cpu.py and the package's get_rays, bit for bit; the source against the
engine it wraps (bit for bit) and the CPU oracle's teacher (the 1e-4 rgb contract); the loop through frontend.main against a
hand-written loop over source.batch -> R2LTrainer.step, against itself, and across --resume, bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from test_online_cpu import host_rays, rand_pixels

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. r2l_rand_rays --------------------------------------------------------------------------------------------------------------
H5, W7 = 5, 7
FOCALS = (6.0, 9.5, 12.0)


@pytest.fixture(scope='module')
def cams(pkg, built_lib):
    """three random orthonormal poses; get_rays of each at its own focal, computed once"""
    from efficient_nerf_amd.teacher import get_rays
    rs = np.random.RandomState(11)
    poses = np.empty((3, 3, 4), dtype=np.float32)
    for p in range(3):
        q, _ = np.linalg.qr(rs.randn(3, 3))
        poses[p, :, :3], poses[p, :, 3] = q, rs.randn(3) * 2
    poses = torch.from_numpy(poses)
    grids = [tuple(t.reshape(-1, 3).cpu().numpy() for t in get_rays(H5, W7, FOCALS[p], poses[p])) for p in range(3)]
    return poses, grids


def _launch(poses, focals, H, W, seed, step, n, want_pixels=True):
    import ctypes as C
    from efficient_nerf_amd._lib import check, current_stream, dptr, lib
    po = poses.cuda().contiguous()
    fo = torch.tensor(focals, dtype=torch.float64).to(torch.float32).cuda()
    ro, rd = (torch.full((n + 1, 3), -7., dtype=torch.float32, device='cuda') for _ in range(2))      # a guard row behind the last ray
    pix = torch.full((n + 1,), -7, dtype=torch.int64, device='cuda') if want_pixels else None
    check(lib().r2l_rand_rays(dptr(po), dptr(fo), len(focals), H, W, seed, step, n, dptr(ro), dptr(rd),
                              C.c_void_p(pix.data_ptr()) if want_pixels else None, current_stream()))
    torch.cuda.synchronize()
    assert (ro[n] == -7).all() and (rd[n] == -7).all() and (pix is None or pix[n] == -7)              # nothing written behind row n - 1
    return ro[:n].cpu().numpy(), rd[:n].cpu().numpy(), None if pix is None else pix[:n].cpu().numpy()


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 1000])
def test_rand_rays_bit_for_bit(cams, n):
    """the wave edge, the block tail, n % n_pose != 0: the pixels are the mirror's, the rays get_rays' rays of those pixels"""
    poses, grids = cams
    seed, step = 5, 9
    ro, rd, pix = _launch(poses, FOCALS, H5, W7, seed, step, n)
    want = rand_pixels(seed, step, n, H5 * W7)
    assert np.array_equal(pix, want)
    p = np.arange(n) % 3
    for k in range(3):
        sel = p == k
        assert np.array_equal(ro[sel], grids[k][0][want[sel]]) and np.array_equal(rd[sel], grids[k][1][want[sel]])
    mo, md, _ = host_rays(poses.numpy(), np.asarray(FOCALS, dtype=np.float32), H5, W7, seed, step, n)
    assert np.array_equal(ro, mo) and np.array_equal(rd, md)
    if n == 1000:
        assert len(set(pix.tolist())) == H5 * W7                                 # every one of the 35 pixels occurs
        again = _launch(poses, FOCALS, H5, W7, seed, step, n)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((ro, rd, pix), again))          # the same arguments, the same bytes
        for other in ((seed, step + 1), (seed + 1, step), (seed + (1 << 32), step), (seed, step + (1 << 32))):
            o_pix = _launch(poses, FOCALS, H5, W7, other[0], other[1], n)[2]
            assert np.array_equal(o_pix, rand_pixels(other[0], other[1], n, H5 * W7)) and not np.array_equal(o_pix, pix)
        ro2, rd2, none = _launch(poses, FOCALS, H5, W7, seed, step, n, want_pixels=False)      # pixel_dev = NULL
        assert none is None and np.array_equal(ro2, ro) and np.array_equal(rd2, rd)


def test_rand_rays_empty_launch(cams):
    ro, rd, pix = _launch(cams[0], FOCALS, H5, W7, 0, 0, 0)
    assert ro.shape == (0, 3) and pix.shape == (0,)


# ---- 2. OnlineTeacherSource ----------------------------------------------------------------------------------------------------
def test_source_targets_are_the_teachers(pkg, built_lib):
    from efficient_nerf_amd import NeRFEngine, PREC_FP16_FP8
    from efficient_nerf_amd.online import OnlineTeacherSource
    seed, H, n_pose, n, t = 3, 16, 3, 600, 4
    focal = O.focal_from_angle(H)
    sd0, sd1 = O.make_teacher_state(seed), O.make_teacher_state(seed + 1)
    eng = NeRFEngine(H, H, focal, precision=PREC_FP16_FP8).load_state_dicts(sd0, sd1)
    lines = []
    src = OnlineTeacherSource(eng, H, H, focal, n_pose=n_pose, seed=seed, watch_every=2, log=lines.append)
    ro, rd, target = src.batch(t, n)                                             # a watched step
    assert all(x.shape == (n, 3) and x.is_cuda and x.dtype == torch.float32 for x in (ro, rd, target))
    # fp16_fp8 is a watched mode: the check rendered a sample again in fp16x3 and compared (NeRFEngine counts those); one line per fallback
    assert src.checks >= 1 and getattr(eng, 'watch_checks', 0) == src.checks and len(lines) == len(src.fallbacks)
    # the rays: the mirror's, from this step's host draws
    poses, focals = src.draws(t)
    assert ((focals >= focal) & (focals < 2 * focal)).all()
    mo, md, _ = host_rays(poses.numpy(), focals.astype(np.float32), H, H, seed, t, n)
    assert np.array_equal(ro.cpu().numpy(), mo) and np.array_equal(rd.cpu().numpy(), md)
    # the target: the engine's render of those rays bit for bit, and the oracle's teacher within the rgb contract
    keep = [x.clone() for x in (ro, rd, target)]
    assert torch.equal(target, eng.render_rays(ro, rd)['rgb_map'])
    ref = O.render_rays(sd0, sd1, ro.cpu(), rd.cpu(), white_bkgd=True)['rgb_map']
    diff = (target.cpu() - ref).abs().max().item()
    print(f'online target vs CPU oracle on {n} rays: L_inf {diff:.3e} ({eng.precision_name})')
    assert diff <= 1e-4
    # a batch is a function of (seed, step): step t + 1 differs, and step t comes back after it
    nxt = src.batch(t + 1, n)
    assert not torch.equal(nxt[1], keep[1])
    assert all(torch.equal(a, b) for a, b in zip(src.batch(t, n), keep))
    fixed = OnlineTeacherSource(eng, H, H, focal, n_pose=n_pose, seed=seed, use_rand_focal=False, watch_every=0)
    fo, fd, _ = fixed.batch(t, 64)
    mo, md, _ = host_rays(fixed.draws(t)[0].numpy(), np.full(n_pose, focal).astype(np.float32), H, H, seed, t, 64)
    assert np.array_equal(fo.cpu().numpy(), mo) and np.array_equal(fd.cpu().numpy(), md)
    eng.close()


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------------
NET = ['--model_name', 'R2L', '--dataset_type', 'blender', '--white_bkgd', '--netdepth', '6', '--netwidth', '32', '--n_sample_per_ray', '4',
       '--multires', '4', '--use_residual', '--trial.ON', '--trial.body_arch', 'resmlp']
SPLIT, N_RAND = 256, 2


@pytest.fixture(scope='module')
def setup(pkg, built_lib, tmp_path_factory):
    """a synthetic 8 x 256 teacher's checkpoint, the student's first weights as a checkpoint (no run draws its own), an empty scene"""
    from efficient_nerf_amd import frontend as fe, train as T
    root = tmp_path_factory.mktemp('online')
    (root / 'empty').mkdir()
    teacher = str(root / 'teacher.tar')
    fe.save_checkpoint(teacher, O.make_teacher_state(1), O.make_teacher_state(2))
    s = {'root': str(root), 'empty': str(root / 'empty'), 'teacher': teacher, 'init': str(root / 'init.tar')}
    tr = T.trainer_from_args(fe.parse_args(_argv(s, 'x')), 8)
    fe.save_checkpoint(s['init'], T.init_state_dict(tr.plan, seed=7))
    return s


def _argv(s, expname, n_iters=4, extra=()):
    return NET + ['--kd_online', '--teacher_ckpt', s['teacher'], '--teacher_config', os.path.join(ROOT, 'configs', 'lego.txt'), '--H', '32',
                  '--synthetic_poses', '1', '--datadir', s['empty'], '--N_rand', str(N_RAND), '--kd_online_split', str(SPLIT),
                  '--kd_online_poses', '3', '--kd_online_seed', '4', '--kd_online_watch', '2', '--N_iters', str(n_iters), '--perturb', '0',
                  '--precision', 'fp16x3', '--i_print', '1', '--i_testset', '2', '--basedir', s['root'], '--expname', expname,
                  '--pretrained_ckpt', s.get('init', '')] + list(extra)


def _main(s, expname, capsys, **kw):
    from efficient_nerf_amd import frontend as fe
    capsys.readouterr()
    assert fe.main(_argv(s, expname, **kw)) == 0
    out = capsys.readouterr().out
    return out.splitlines(), torch.load(os.path.join(s['root'], expname, 'weights', 'ckpt.tar'), map_location='cpu', weights_only=False)


def _same_state(a, b):
    wa, wb = a['network_fn_state_dict'], b['network_fn_state_dict']
    sa, sb = a['optimizer_state_dict']['state'], b['optimizer_state_dict']['state']
    return (list(wa) == list(wb) and all(torch.equal(wa[k], wb[k]) for k in wa) and sorted(sa) == sorted(sb) and len(sa) > 0 and
            all(torch.equal(sa[k][m], sb[k][m]) for k in sa for m in ('exp_avg', 'exp_avg_sq', 'step')))


@pytest.fixture(scope='module')
def whole(setup):
    """the uninterrupted four-step run, once for the tests that compare with it: (its log lines, its ckpt.tar)"""
    from efficient_nerf_amd import frontend as fe, train as T
    lines = []
    T.train(fe.parse_args(_argv(setup, 'whole')), log=lines.append)
    return lines, torch.load(os.path.join(setup['root'], 'whole', 'weights', 'ckpt.tar'), map_location='cpu', weights_only=False)


def test_loop_start_up_and_train_lines(setup, whole):
    lines, ck = whole
    start = [ln for ln in lines if ln.startswith('Online distillation')]
    assert len(start) == 1 and '\n' not in start[0]
    f = O.focal_from_angle(32) / 2
    for part in (f'teacher "{setup["teacher"]}" in fp16x3', '3 random poses of 16 x 16 per step', f'focal {f:.2f} .. {2 * f:.2f}', 'seed 4',
                 'watched every 2 steps', f'{N_RAND * SPLIT} rays per step + 0 hard rays'):
        assert part in start[0], (part, start[0])
    assert not any(ln.startswith('Found ') for ln in lines)
    # no test split under --datadir: the line of today, and no [TEST] line at --i_testset 2
    tf = os.path.join(setup['empty'], 'transforms_test.json')
    assert f'No test renders during this run: "{tf}" is not there.' in lines and not any(ln.startswith('[TEST]') for ln in lines)
    train = [re.match(r'^\[TRAIN\] Iter (\d+) data_time (\S+) batch_time (\S+) loss (\S+) psnr (\S+) hist_psnr (\S+) LR (\d\.\d{10})$', ln)
             for ln in lines if ln.startswith('[TRAIN]')]
    assert len(train) == 4 and all(train) and [int(m.group(1)) for m in train] == [1, 2, 3, 4]
    assert all(np.isfinite(float(m.group(4))) and 0 <= float(m.group(2)) <= float(m.group(3)) for m in train)
    assert ck['global_step'] == 4 and sorted(ck) == ['best_psnr', 'best_psnr_step', 'global_step', 'network_fn_state_dict', 'optimizer_state_dict']


def test_loop_is_source_batch_then_trainer_step(setup, whole):
    """weights and Adam moments after four steps of the command line = a hand-written loop over source.batch(i) -> R2LTrainer.step"""
    from efficient_nerf_amd import frontend as fe, online, train as T
    args = fe.parse_args(_argv(setup, 'hand'))
    tr = T.trainer_from_args(args, N_RAND * SPLIT)
    tr.load_state_dict(fe.load_checkpoint(setup['init'])['network_fn_state_dict'])
    src, _ = online.source_from_args(args, log=lambda *a: None)
    for i in range(1, 5):
        ro, rd, tg = src.batch(i, N_RAND * SPLIT)
        tr.step(ro, rd, tg, T.learning_rate(i, args.lrate, args.lrate_decay, args.warmup_lr), perturb=0.)
    hand = {'network_fn_state_dict': dict(tr.state_dict()), 'optimizer_state_dict': tr.optimizer_state_dict()}
    assert _same_state(whole[1], hand)
    init = fe.load_checkpoint(setup['init'])['network_fn_state_dict']
    assert not all(torch.equal(init[k], hand['network_fn_state_dict'][k]) for k in init)      # and training moved them
    src.engine.close()


def test_two_runs_and_a_resumed_run_end_on_the_same_bits(setup, whole, capsys):
    """through frontend.main: the same command line again; and two steps, then --resume to four (the jitter is off: the only random
    input is the source, a function of (seed, step))"""
    lines, again = _main(setup, 'again', capsys)
    assert _same_state(whole[1], again) and sum(ln.startswith('[TRAIN] Iter') for ln in lines) == 4
    _, first = _main(setup, 'first', capsys, n_iters=2)
    assert first['global_step'] == 2 and not _same_state(whole[1], first)
    ck2 = os.path.join(setup['root'], 'first', 'weights', 'ckpt.tar')
    argv = [a for a in _argv(setup, 'resumed')]
    argv[argv.index('--pretrained_ckpt') + 1] = ck2
    from efficient_nerf_amd import frontend as fe
    capsys.readouterr()
    assert fe.main(argv + ['--resume']) == 0
    out = capsys.readouterr().out.splitlines()
    assert 'Resume optimizer successfully.' in out and [ln.split()[2] for ln in out if ln.startswith('[TRAIN] Iter')] == ['3', '4']
    resumed = torch.load(os.path.join(setup['root'], 'resumed', 'weights', 'ckpt.tar'), map_location='cpu', weights_only=False)
    assert resumed['global_step'] == 4 and _same_state(whole[1], resumed)


def test_hard_ray_pool_on_online_batches(setup, capsys, monkeypatch):
    """--hard_ratio 0.2 --hard_mul 2 at 512 rays: 102 rays in and out, the pool is full after 11 steps (1,122 >= 1,024 rows) and steps
    12 and 13 carry 614 rows"""
    from efficient_nerf_amd import train as T
    rows, step = [], T.R2LTrainer.step
    monkeypatch.setattr(T.R2LTrainer, 'step', lambda self, rays_o, *a, **k: (rows.append(rays_o.shape[0]), step(self, rays_o, *a, **k))[1])
    lines, ck = _main(setup, 'hard', capsys, n_iters=13, extra=['--hard_ratio', '0.2', '--hard_mul', '2'])
    start = [ln for ln in lines if ln.startswith('Online distillation')]
    assert len(start) == 1 and f'{N_RAND * SPLIT} rays per step + 102 hard rays' in start[0]
    assert rows == [N_RAND * SPLIT] * 11 + [N_RAND * SPLIT + 102] * 2
    losses = [float(ln.split(' loss ')[1].split()[0]) for ln in lines if ln.startswith('[TRAIN] Iter')]
    assert len(losses) == 13 and np.isfinite(losses).all() and ck['global_step'] == 13
